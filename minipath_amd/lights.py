"""Point and sphere lights traced from the feature planes (include/minipath_lights.h, lights/libminipath_lights.so).

A library of its own beside libminipath_hip.so, like the secondary rays': it turns the image-major [h, w, 4] "position" and "normal"
planes FrameRenderer.untile_plane produces into bounded shadow rays, one per light and sample, in the SoA buffers mp_occluded_rays
takes, and reduces that query's answers to an irradiance plane.  It is loaded on first use, so ``import minipath_amd`` works where
it was not built; there is no other compute path (a missing library raises).
"""
from __future__ import annotations

import ctypes as C
import os

from . import _lib as _hip
from . import _postlib
from ._lib import MP_OK, MinipathError

_HERE = os.path.dirname(os.path.abspath(__file__))
# MINIPATH_LIGHTS_SO: experiment builds of the same library; default = the in-tree build
LIGHTS_SO_PATH = os.environ.get("MINIPATH_LIGHTS_SO") or os.path.join(_HERE, "lights", "libminipath_lights.so")

MPL_FLAG_ACCUMULATE = 1
MPL_MAX_LIGHTS = 8
MPL_MAX_SAMPLES = 65536
TRACED_ARRAYS = ("ox", "oy", "oz", "dx", "dy", "dz", "tmax")  # what mp_occluded_rays takes
RAY_ARRAYS = TRACED_ARRAYS + ("weight",)


class Light(C.Structure):
    """mpl_light."""

    _fields_ = [("position", C.c_float * 3), ("radius", C.c_float), ("intensity", C.c_float * 3), ("reserved", C.c_float)]


class LightsSettings(C.Structure):
    """mpl_settings."""

    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32),
                ("sample_count", C.c_uint32), ("sample_begin", C.c_uint32), ("batch", C.c_uint32), ("light_count", C.c_uint32),
                ("seed", C.c_uint64), ("eye", C.c_float * 3), ("bias", C.c_float), ("margin", C.c_float)]


# name -> (restype, argtypes); every symbol include/minipath_lights.h declares
SIGNATURES = {
    "mpl_last_error": (C.c_char_p, []),
    "mpl_settings_size": (C.c_uint32, []),
    "mpl_check_settings": (C.c_int, [C.POINTER(LightsSettings), C.c_void_p]),
    "mpl_generate": (C.c_int, [C.c_int, C.POINTER(LightsSettings), C.c_void_p] + [C.c_void_p] * 11),
    "mpl_resolve": (C.c_int, [C.c_int, C.POINTER(LightsSettings), C.c_void_p] + [C.c_void_p] * 6),
    "mpl_last_kernels": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
}

_lib = None


def lib() -> C.CDLL:
    """Load libminipath_lights.so.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        _lib = _postlib.load(LIGHTS_SO_PATH, SIGNATURES, "the lights have no CPU fallback")
    return _lib


def check(rc: int) -> None:
    if rc != MP_OK:
        msg = lib().mpl_last_error()
        raise MinipathError(rc, msg.decode() if msg else "")


def last_kernels() -> list:
    """mpl_last_kernels: the kernel of the calling thread's last launching call."""
    return _postlib.last_kernels(lib().mpl_last_kernels, check)


def light_table(lights):
    """The host array of mpl_light for a sequence of (position, radius, intensity) or an [L, 8] array of
    {p.x, p.y, p.z, radius, i.r, i.g, i.b, reserved} rows.  The values are checked by the library, the count here."""
    rows = []
    for lt in lights:
        if len(lt) == 3:
            position, radius, intensity = lt
            rows.append([float(v) for v in position] + [float(radius)] + [float(v) for v in intensity] + [0.0])
        else:
            rows.append([float(v) for v in lt])
        if len(rows[-1]) != 8:
            raise ValueError("lights: (position, radius, intensity) or eight numbers per light are expected")
    if not 0 < len(rows) <= MPL_MAX_LIGHTS:
        raise ValueError(f"lights: 1 .. {MPL_MAX_LIGHTS} lights are expected")
    table = (Light * len(rows))()
    for rec, row in zip(table, rows):
        rec.position[:], rec.radius, rec.intensity[:], rec.reserved = row[:3], row[3], row[4:7], row[7]
    return table


class LocalLights:
    """Direct light of point and sphere lights (include/minipath_lights.h) for one scene and one resolution (width, height):
    shadow rays start on the surfaces the "position" and "normal" planes describe, end at the light (less `margin`), go through the
    scene's occlusion query (mp_occluded_rays) with their own tmax and come back as an irradiance plane {E.r, E.g, E.b, alpha}:
    E = the mean over a pixel's samples of  sum over the lights seen  of intensity * cos / distance^2, alpha = 0 where nothing was
    counted (misses), so the plane passes through TemporalAccumulator and AtrousDenoiser as a colour.  A sphere light of radius R
    is sampled over the disc it shows to the surface (soft shadows); radius 0 is a point light.

    It owns the ray buffers of `batch` samples per pixel and light (33 bytes per ray) and the sums plane {E.r, E.g, E.b, counted},
    both sized on first use for the number of lights of the call.  A call runs ceil(samples / batch) batches of  mpl_generate ->
    mp_occluded_rays -> mpl_resolve  on the current torch stream without a host synchronisation.  The result does not depend on
    `batch`.  With GuidedResampler's low-resolution planes and a LocalLights of the low resolution it runs at half resolution.

        ll = mp.LocalLights(scene, resolution)
        lamp = [((0.0, 3.0, 0.0), 0.2, (40.0, 36.0, 30.0)), ((2.0, 1.0, 1.0), 0.0, (5.0, 5.0, 8.0))]
        light, sums = ll.irradiance(position, normal, camera, lamp, samples=8, seed=frame + 1000, margin=0.25)

    `light` and `sums` are this object's own planes: the next call overwrites them, so copy what has to live longer.  The same
    `seed` as a SecondaryVisibility pass gives the same disc samples: offset one of them.
    """

    def __init__(self, scene, resolution, device=None, batch: int = 2):
        obj = getattr(scene, "object", scene)
        if obj.ctx is None:
            raise MinipathError(1, "host-only BVH cannot be traced: pass a Context to with_obj/build")
        if device is None:
            device = obj.ctx.device_id
        self.device, self.device_id = _postlib.resolve_device(device, "the lights run on the GPU")
        if self.device_id != obj.ctx.device_id:
            raise ValueError(f"the scene lives on device {obj.ctx.device_id}, not {self.device_id}")
        self.scene, self.object = scene, obj
        self.width, self.height = int(resolution[0]), int(resolution[1])
        self.batch = int(batch)
        one = light_table([((0.0, 0.0, 0.0), 0.0, (1.0, 1.0, 1.0))])
        check(lib().mpl_check_settings(C.byref(self._settings(0, self.batch, 0, self.batch, 1, 0, (0, 0, 0), 0.0, 0.0)), one))
        self._buffers, self._rays = None, 0  # made on first use

    @staticmethod
    def eye_of(camera):
        """The `eye` of a Camera: its lens centre (SecondaryVisibility.eye_of)."""
        return [float(v) for v in camera.center_forward_up_right()[0]]

    def _settings(self, flags, samples, begin, batch, light_count, seed, eye, bias, margin) -> LightsSettings:
        st = LightsSettings(C.sizeof(LightsSettings), self.width, self.height, flags, int(samples), int(begin), int(batch), int(light_count),
                            int(seed) & 0xFFFFFFFFFFFFFFFF)
        st.eye[:] = [float(v) for v in eye]
        st.bias, st.margin = float(bias), float(margin)
        return st

    def _stream(self):
        return _postlib.stream_of(self.device)

    def _plane(self, t, name):
        return _postlib.expect_plane(t, name, self.device, self.device_id, (self.height, self.width, 4))

    def _make_buffers(self, light_count: int):
        import torch

        n = self.width * self.height * self.batch * light_count
        if self._buffers is None or self._rays < n:
            planes = None if self._buffers is None else {k: self._buffers[k] for k in ("sums", "out")}
            b = {k: torch.empty(n, dtype=torch.float32, device=self.device) for k in RAY_ARRAYS}
            b["occluded"] = torch.empty(n, dtype=torch.uint8, device=self.device)
            for k in ("sums", "out"):
                b[k] = planes[k] if planes else torch.empty((self.height, self.width, 4), dtype=torch.float32, device=self.device)
            self._buffers, self._rays = b, n
        return self._buffers

    def irradiance(self, position, normal, eye, lights, samples: int, seed: int = 0, bias: float = 1e-4, margin: float = 0.0):
        """(out, sums): `samples` shadow rays per hit pixel and light from position + n * bias, n the normal turned towards `eye` (a
        Camera, or the three coordinates of its lens centre: eye_of), to the light, `margin` short of it.  `lights`: a sequence of
        (position, radius, intensity) or an [L, 8] array, at most 8.  out = {E.r, E.g, E.b, alpha}; sums = {sum.r, sum.g, sum.b,
        counted}.  Surfaces that face away from a light, or lie inside it or within `margin` of it, get nothing from it without a
        trace.  position {p.x, p.y, p.z, alpha} and normal {n.x, n.y, n.z, t} are untiled float32 planes and are only read."""
        position, normal = self._plane(position, "position"), self._plane(normal, "normal")
        if hasattr(eye, "center_forward_up_right"):
            eye = self.eye_of(eye)
        samples = int(samples)
        if not 0 < samples <= MPL_MAX_SAMPLES:
            raise ValueError(f"samples: 1 .. {MPL_MAX_SAMPLES} is expected")
        table = light_table(lights)
        L = len(table)
        b = self._make_buffers(L)
        rays = [b[k].data_ptr() for k in RAY_ARRAYS]
        stream = self._stream()
        hip, ctx = _hip.lib(), self.object.ctx
        for begin in range(0, samples, self.batch):
            n = min(self.batch, samples - begin)
            last = begin + n == samples
            st = self._settings(MPL_FLAG_ACCUMULATE if begin else 0, samples, begin, n, L, seed, eye, bias, margin)
            check(lib().mpl_generate(self.device_id, C.byref(st), table, position.data_ptr(), normal.data_ptr(), *rays, stream))
            # the SoA buffers as they are, each ray with its own tmax; rays with tmax <= 0 are not walked
            _hip.check(hip.mp_occluded_rays(ctx.handle, self.object.handle, *rays[:7], self.width * self.height * n * L,
                                            b["occluded"].data_ptr(), stream))
            check(lib().mpl_resolve(self.device_id, C.byref(st), table, b["tmax"].data_ptr(), b["weight"].data_ptr(), b["occluded"].data_ptr(),
                                    b["sums"].data_ptr(), b["out"].data_ptr() if last else None, stream))
        return b["out"], b["sums"]

    def last_kernels(self) -> list:
        """The kernel the calling thread's last launching call of this library launched (mpl_last_kernels)."""
        return last_kernels()
