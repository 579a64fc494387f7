"""Ambient occlusion and sun shadows traced from the feature planes (include/minipath_secondary.h,
secondary/libminipath_secondary.so).

A library of its own beside libminipath_hip.so, like the denoiser's: it turns the image-major [h, w, 4] "position" and "normal"
planes FrameRenderer.untile_plane produces into the SoA ray buffers mp_occluded_rays takes and reduces that query's answers to a
visibility plane.  It is loaded on first use, so ``import minipath_amd`` works where it was not built; there is no other compute
path (a missing library raises).
"""
from __future__ import annotations

import ctypes as C
import math
import os

from . import _lib as _hip
from . import _postlib
from ._lib import MP_OK, MinipathError

_HERE = os.path.dirname(os.path.abspath(__file__))
# MINIPATH_SECONDARY_SO: experiment builds of the same library; default = the in-tree build
SECONDARY_SO_PATH = os.environ.get("MINIPATH_SECONDARY_SO") or os.path.join(_HERE, "secondary", "libminipath_secondary.so")

MPS_MODE_AO, MPS_MODE_SUN = 0, 1
MPS_FLAG_ACCUMULATE = 1
MPS_MAX_SAMPLES = 65536
RAY_ARRAYS = ("ox", "oy", "oz", "dx", "dy", "dz", "tmax")


class SecondarySettings(C.Structure):
    """mps_settings."""

    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("mode", C.c_uint32), ("flags", C.c_uint32),
                ("sample_count", C.c_uint32), ("sample_begin", C.c_uint32), ("batch", C.c_uint32), ("seed", C.c_uint64),
                ("eye", C.c_float * 3), ("light", C.c_float * 3), ("radius", C.c_float), ("bias", C.c_float), ("spread", C.c_float)]


# name -> (restype, argtypes); every symbol include/minipath_secondary.h declares
SIGNATURES = {
    "mps_last_error": (C.c_char_p, []),
    "mps_settings_size": (C.c_uint32, []),
    "mps_check_settings": (C.c_int, [C.POINTER(SecondarySettings)]),
    "mps_generate": (C.c_int, [C.c_int, C.POINTER(SecondarySettings)] + [C.c_void_p] * 10),
    "mps_resolve": (C.c_int, [C.c_int, C.POINTER(SecondarySettings)] + [C.c_void_p] * 5),
    "mps_last_kernels": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
}

_lib = None


def lib() -> C.CDLL:
    """Load libminipath_secondary.so.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        _lib = _postlib.load(SECONDARY_SO_PATH, SIGNATURES, "the secondary rays have no CPU fallback")
    return _lib


def check(rc: int) -> None:
    if rc != MP_OK:
        msg = lib().mps_last_error()
        raise MinipathError(rc, msg.decode() if msg else "")


def last_kernels() -> list:
    """mps_last_kernels: the kernel of the calling thread's last launching call."""
    return _postlib.last_kernels(lib().mps_last_kernels, check)


class SecondaryVisibility:
    """Deferred secondary visibility (include/minipath_secondary.h) for one scene and one resolution (width, height): rays start
    on the surfaces the "position" and "normal" planes describe, go through the scene's occlusion query (mp_occluded_rays) and come
    back as a visibility plane {v, v, v, alpha}: v = the fraction of a pixel's counted samples that reached `radius` unoccluded,
    alpha = 0 where nothing was counted (misses), so the plane passes through TemporalAccumulator and AtrousDenoiser as a colour.

    It owns the ray buffers of `batch` samples per pixel (29 bytes per ray) and the counts plane {visible, counted, 0, 0}.  A call
    runs ceil(samples / batch) batches of  mps_generate -> mp_occluded_rays -> mps_resolve  on the current torch stream without a
    host synchronisation; the last batch is smaller when samples % batch != 0.  The result does not depend on `batch`.

        fr = mp.FrameRenderer(scene, camera, settings)
        planes = fr.new_aov_planes(position=True)
        fr.render_aov_pass(planes)                                              # render_aov_pass
        position, normal = fr.untile_plane(planes["position"]), fr.untile_plane(planes["normal"])   # untile_plane
        sv = mp.SecondaryVisibility(scene, resolution)
        ao, counts = sv.ambient_occlusion(position, normal, camera, samples=8, radius=1.5, seed=frame)
        out, var = acc.accumulate(ao, position, normal, fr.untile_plane(planes["ids"]),
                                  mp.TemporalAccumulator.view_of(camera, resolution))   # TemporalAccumulator.accumulate
        clean, _ = dn.denoise(out, normal, variance=var)                        # AtrousDenoiser.denoise

    `ao` and `counts` are this object's own planes: the next call overwrites them, so copy what has to live longer.
    """

    def __init__(self, scene, resolution, device=None, batch: int = 4):
        obj = getattr(scene, "object", scene)
        if obj.ctx is None:
            raise MinipathError(1, "host-only BVH cannot be traced: pass a Context to with_obj/build")
        if device is None:
            device = obj.ctx.device_id
        self.device, self.device_id = _postlib.resolve_device(device, "the secondary rays run on the GPU")
        if self.device_id != obj.ctx.device_id:
            raise ValueError(f"the scene lives on device {obj.ctx.device_id}, not {self.device_id}")
        self.scene, self.object = scene, obj
        self.width, self.height = int(resolution[0]), int(resolution[1])
        self.batch = int(batch)
        check(lib().mps_check_settings(C.byref(self._settings(MPS_MODE_AO, 0, self.batch, 0, self.batch, 0, (0, 0, 0), (0, 0, 1), 1.0, 0.0, 0.0))))
        self._buffers = None  # made on first use

    @staticmethod
    def eye_of(camera):
        """The `eye` of a Camera: its lens centre, the first of Camera.center_forward_up_right() (what TemporalAccumulator.view_of
        calls `center`)."""
        return [float(v) for v in camera.center_forward_up_right()[0]]

    def _settings(self, mode, flags, samples, begin, batch, seed, eye, light, radius, bias, spread) -> SecondarySettings:
        st = SecondarySettings(C.sizeof(SecondarySettings), self.width, self.height, mode, flags, int(samples), int(begin), int(batch),
                               int(seed) & 0xFFFFFFFFFFFFFFFF)
        st.eye[:], st.light[:] = [float(v) for v in eye], [float(v) for v in light]
        st.radius, st.bias, st.spread = float(radius), float(bias), float(spread)
        return st

    def _stream(self):
        return _postlib.stream_of(self.device)

    def _plane(self, t, name):
        return _postlib.expect_plane(t, name, self.device, self.device_id, (self.height, self.width, 4))

    def _make_buffers(self):
        import torch

        if self._buffers is None:
            n = self.width * self.height * self.batch
            b = {k: torch.empty(n, dtype=torch.float32, device=self.device) for k in RAY_ARRAYS}
            b["occluded"] = torch.empty(n, dtype=torch.uint8, device=self.device)
            b["counts"] = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=self.device)
            b["out"] = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=self.device)
            self._buffers = b
        return self._buffers

    def _run(self, mode, position, normal, eye, light, samples, radius, seed, bias, spread):
        position, normal = self._plane(position, "position"), self._plane(normal, "normal")
        if hasattr(eye, "center_forward_up_right"):
            eye = self.eye_of(eye)
        samples = int(samples)
        if not 0 < samples <= MPS_MAX_SAMPLES:
            raise ValueError(f"samples: 1 .. {MPS_MAX_SAMPLES} is expected")
        b = self._make_buffers()
        rays = [b[k].data_ptr() for k in RAY_ARRAYS]
        stream = self._stream()
        hip, ctx = _hip.lib(), self.object.ctx
        for begin in range(0, samples, self.batch):
            n = min(self.batch, samples - begin)
            last = begin + n == samples
            st = self._settings(mode, MPS_FLAG_ACCUMULATE if begin else 0, samples, begin, n, seed, eye, light, radius, bias, spread)
            check(lib().mps_generate(self.device_id, C.byref(st), position.data_ptr(), normal.data_ptr(), *rays, stream))
            # the SoA buffers as they are: no transposes, and rays with tmax <= 0 are not walked
            _hip.check(hip.mp_occluded_rays(ctx.handle, self.object.handle, *rays, self.width * self.height * n, b["occluded"].data_ptr(),
                                            stream))
            check(lib().mps_resolve(self.device_id, C.byref(st), b["tmax"].data_ptr(), b["occluded"].data_ptr(), b["counts"].data_ptr(),
                                    b["out"].data_ptr() if last else None, stream))
        return b["out"], b["counts"]

    def ambient_occlusion(self, position, normal, eye, samples: int, radius: float, seed: int = 0, bias: float = 1e-4):
        """(out, counts): `samples` cosine-distributed rays of length `radius` per hit pixel from position + n * bias, n the normal
        turned towards `eye` (a Camera, or the three coordinates of its lens centre: eye_of).  out = {v, v, v, alpha}, v = the
        unoccluded fraction; counts = {unoccluded, counted, 0, 0}.  position {p.x, p.y, p.z, alpha} and normal {n.x, n.y, n.z, t}
        are untiled float32 planes and are only read."""
        return self._run(MPS_MODE_AO, position, normal, eye, (0.0, 0.0, 1.0), samples, radius, seed, bias, 0.0)

    def sun_visibility(self, position, normal, eye, light, samples: int, spread: float = 0.0, radius: float = math.inf, seed: int = 0,
                       bias: float = 1e-4):
        """(out, counts): `samples` shadow rays per hit pixel towards the directional light `light` (a unit vector TOWARDS the
        light, used as given), drawn over a disc of radius `spread` at distance 1 about it (0 = a hard shadow).  Pixels that face
        away from the light count every sample as not visible without tracing it.  out and counts as ambient_occlusion's."""
        return self._run(MPS_MODE_SUN, position, normal, eye, light, samples, radius, seed, bias, spread)

    def last_kernels(self) -> list:
        """The kernel the calling thread's last launching call of this library launched (mps_last_kernels)."""
        return last_kernels()
