"""Sky lighting from the feature planes (include/minipath_sky.h, sky/libminipath_sky.so).

A library of its own beside libminipath_hip.so, like the lights': it reduces the answers of the occlusion query on the
cosine-distributed rays of the ambient occlusion (mps_generate of libminipath_secondary.so) once more, with the rays' directions:
every ray that escapes looks its direction up in an octahedral environment map.  It is loaded on first use, so ``import
minipath_amd`` works where it was not built; there is no other compute path (a missing library raises).
"""
from __future__ import annotations

import ctypes as C
import math
import os

from . import _lib as _hip
from . import _postlib
from . import secondary as _sec
from ._lib import MP_OK, MinipathError

_HERE = os.path.dirname(os.path.abspath(__file__))
# MINIPATH_SKY_SO: experiment builds of the same library; default = the in-tree build
SKY_SO_PATH = os.environ.get("MINIPATH_SKY_SO") or os.path.join(_HERE, "sky", "libminipath_sky.so")

MPE_FLAG_ACCUMULATE = 1
MPE_MAX_MAP = 8192
MPE_MAX_SAMPLES = 65536
RAY_ARRAYS = _sec.RAY_ARRAYS           # what mps_generate writes and mp_occluded_rays takes
READ_ARRAYS = ("dx", "dy", "dz", "tmax")  # what mpe_resolve reads of them


class SkySettings(C.Structure):
    """mpe_settings."""

    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32),
                ("sample_count", C.c_uint32), ("sample_begin", C.c_uint32), ("batch", C.c_uint32), ("map_size", C.c_uint32),
                ("pole", C.c_uint32)]


_F3 = C.c_float * 3
# name -> (restype, argtypes); every symbol include/minipath_sky.h declares
SIGNATURES = {
    "mpe_last_error": (C.c_char_p, []),
    "mpe_settings_size": (C.c_uint32, []),
    "mpe_check_settings": (C.c_int, [C.POINTER(SkySettings)]),
    "mpe_resolve": (C.c_int, [C.c_int, C.POINTER(SkySettings)] + [C.c_void_p] * 9),
    "mpe_fill_gradient": (C.c_int, [C.c_int, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p,
                                    C.c_void_p]),
    "mpe_last_kernels": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
}

_lib = None


def lib() -> C.CDLL:
    """Load libminipath_sky.so.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        _lib = _postlib.load(SKY_SO_PATH, SIGNATURES, "the sky lighting has no CPU fallback")
    return _lib


def check(rc: int) -> None:
    if rc != MP_OK:
        msg = lib().mpe_last_error()
        raise MinipathError(rc, msg.decode() if msg else "")


def last_kernels() -> list:
    """mpe_last_kernels: the kernel of the calling thread's last launching call."""
    return _postlib.last_kernels(lib().mpe_last_kernels, check)


def _colour(c, name):
    c = [float(v) for v in c]
    if len(c) != 3:
        raise ValueError(f"{name}: three numbers (r, g, b) are expected")
    return _F3(*c)


def gradient_sky(n: int, zenith, horizon, ground, device=0):
    """An [n, n, 4] float32 octahedral environment map on `device` (mpe_fill_gradient): `horizon` at the horizon blending to `zenith`
    straight up, linearly in the sine of the elevation, and `ground` everywhere below the horizon.  The colours are (r, g, b), finite.
    The call is asynchronous on the current torch stream."""
    import torch

    device, device_id = _postlib.resolve_device(device, "the sky lighting runs on the GPU")
    n = int(n)
    if not 0 < n <= MPE_MAX_MAP:
        raise ValueError(f"n: 1 .. {MPE_MAX_MAP} is expected")
    fill = lib().mpe_fill_gradient  # a missing library raises before anything is allocated
    env = torch.empty((n, n, 4), dtype=torch.float32, device=device)
    check(fill(device_id, n, _colour(zenith, "zenith"), _colour(horizon, "horizon"), _colour(ground, "ground"), env.data_ptr(),
               _postlib.stream_of(device)))
    return env


class SkyLight:
    """Light from an environment map (include/minipath_sky.h) for one scene and one resolution (width, height): the rays of the
    ambient occlusion -- cosine-distributed about the normal, from the surfaces the "position" and "normal" planes describe -- go
    through the scene's occlusion query (mp_occluded_rays), and every ray that escapes looks its direction up in the map.  The
    result is a plane {E.r, E.g, E.b, alpha}: the mean over a pixel's samples of the radiance the sample saw (0 where it was
    occluded), that is the sky's irradiance / pi, alpha = 0 where nothing was counted (misses), so the plane passes through
    TemporalAccumulator and AtrousDenoiser as a colour.

    `env` is an octahedral map: any 16-byte aligned contiguous [N, N, 4] float32 tensor on the device, 1 <= N <= 8192 --
    gradient_sky makes one, and an image loaded with io.load_exr_f32 and resampled to the octahedral layout by the caller is
    another.  `pole` is the world axis (0, 1, 2 = x, y, z) that is the map's +z, the zenith of a sky: 1 for a y-up scene.

    It owns the ray buffers of `batch` samples per pixel (29 bytes per ray) and its planes.  A call runs ceil(samples / batch)
    batches of  mps_generate (MPS_MODE_AO) -> mp_occluded_rays -> mpe_resolve  on the current torch stream without a host
    synchronisation.  The result does not depend on `batch`.  With visibility=True each batch also runs mps_resolve on the same
    trace and the call returns the ambient-occlusion plane of SecondaryVisibility.ambient_occlusion for the same seed as well: one
    trace for both.  With GuidedResampler's low-resolution planes and a SkyLight of the low resolution it runs at half resolution.

        sky_map = mp.gradient_sky(64, zenith=(0.2, 0.4, 1.0), horizon=(1.0, 0.9, 0.8), ground=(0.05, 0.04, 0.03), device=0)
        sl = mp.SkyLight(scene, resolution)
        sky, sums = sl.light(position, normal, camera, sky_map, samples=8, seed=frame)
        sky, sums, ao, counts = sl.light(position, normal, camera, sky_map, samples=8, seed=frame, visibility=True)

    The planes returned are this object's own: the next call overwrites them, so copy what has to live longer.
    """

    def __init__(self, scene, resolution, device=None, batch: int = 2):
        obj = getattr(scene, "object", scene)
        if obj.ctx is None:
            raise MinipathError(1, "host-only BVH cannot be traced: pass a Context to with_obj/build")
        if device is None:
            device = obj.ctx.device_id
        self.device, self.device_id = _postlib.resolve_device(device, "the sky lighting runs on the GPU")
        if self.device_id != obj.ctx.device_id:
            raise ValueError(f"the scene lives on device {obj.ctx.device_id}, not {self.device_id}")
        self.scene, self.object = scene, obj
        self.width, self.height = int(resolution[0]), int(resolution[1])
        self.batch = int(batch)
        check(lib().mpe_check_settings(C.byref(self._settings(0, self.batch, 0, self.batch, 1, 1))))
        self._buffers = None  # made on first use

    @staticmethod
    def eye_of(camera):
        """The `eye` of a Camera: its lens centre (SecondaryVisibility.eye_of)."""
        return [float(v) for v in camera.center_forward_up_right()[0]]

    def _settings(self, flags, samples, begin, batch, map_size, pole) -> SkySettings:
        return SkySettings(C.sizeof(SkySettings), self.width, self.height, flags, int(samples), int(begin), int(batch), int(map_size),
                           int(pole))

    def _ao_settings(self, flags, samples, begin, batch, seed, eye, radius, bias):
        st = _sec.SecondarySettings(C.sizeof(_sec.SecondarySettings), self.width, self.height, _sec.MPS_MODE_AO, flags, int(samples),
                                    int(begin), int(batch), int(seed) & 0xFFFFFFFFFFFFFFFF)
        st.eye[:], st.light[:] = [float(v) for v in eye], (0.0, 0.0, 1.0)
        st.radius, st.bias, st.spread = float(radius), float(bias), 0.0
        return st

    def _stream(self):
        return _postlib.stream_of(self.device)

    def _plane(self, t, name):
        return _postlib.expect_plane(t, name, self.device, self.device_id, (self.height, self.width, 4))

    def _env(self, env):
        import torch

        n = env.shape[0] if isinstance(env, torch.Tensor) and env.dim() == 3 else 0
        if not 0 < n <= MPE_MAX_MAP:
            raise ValueError(f"env: a contiguous float32 [N, N, 4] tensor on {self.device}, 1 <= N <= {MPE_MAX_MAP}, is expected")
        return _postlib.expect_plane(env, "env", self.device, self.device_id, (n, n, 4)), n

    def _make_buffers(self):
        import torch

        if self._buffers is None:
            n = self.width * self.height * self.batch
            b = {k: torch.empty(n, dtype=torch.float32, device=self.device) for k in RAY_ARRAYS}
            b["occluded"] = torch.empty(n, dtype=torch.uint8, device=self.device)
            for k in ("sums", "out", "counts", "ao"):
                b[k] = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=self.device)
            self._buffers = b
        return self._buffers

    def light(self, position, normal, camera, env, samples: int, seed: int = 0, pole: int = 1, radius: float = math.inf,
              bias: float = 1e-4, visibility: bool = False):
        """(out, sums), or (out, sums, ao, counts) with visibility=True: `samples` cosine-distributed rays of length `radius` per hit
        pixel from position + n * bias, n the normal turned towards the eye (`camera`: a Camera, or the three coordinates of its
        lens centre: eye_of); a ray that reaches `radius` unoccluded adds the map's radiance in its direction.  out = {E.r, E.g, E.b, alpha};
        sums = {sum.r, sum.g, sum.b, counted}; ao and counts are those of SecondaryVisibility.ambient_occlusion with the same
        `samples`, `radius`, `seed` and `bias`.  position {p.x, p.y, p.z, alpha}, normal {n.x, n.y, n.z, t} and env are only read."""
        position, normal = self._plane(position, "position"), self._plane(normal, "normal")
        env, n_map = self._env(env)
        eye = self.eye_of(camera) if hasattr(camera, "center_forward_up_right") else camera
        samples = int(samples)
        if not 0 < samples <= MPE_MAX_SAMPLES:
            raise ValueError(f"samples: 1 .. {MPE_MAX_SAMPLES} is expected")
        # a bad pole is refused here, before the first batch's rays are written
        check(lib().mpe_check_settings(C.byref(self._settings(0, samples, 0, min(self.batch, samples), n_map, pole))))
        b = self._make_buffers()
        rays = [b[k].data_ptr() for k in RAY_ARRAYS]
        read = [b[k].data_ptr() for k in READ_ARRAYS]
        stream = self._stream()
        hip, sec, ctx = _hip.lib(), _sec.lib(), self.object.ctx
        for begin in range(0, samples, self.batch):
            n = min(self.batch, samples - begin)
            last = begin + n == samples
            st = self._settings(MPE_FLAG_ACCUMULATE if begin else 0, samples, begin, n, n_map, pole)
            ao_st = self._ao_settings(_sec.MPS_FLAG_ACCUMULATE if begin else 0, samples, begin, n, seed, eye, radius, bias)
            _sec.check(sec.mps_generate(self.device_id, C.byref(ao_st), position.data_ptr(), normal.data_ptr(), *rays, stream))
            # the SoA buffers as they are: no transposes, and rays with tmax <= 0 are not walked
            _hip.check(hip.mp_occluded_rays(ctx.handle, self.object.handle, *rays, self.width * self.height * n, b["occluded"].data_ptr(),
                                            stream))
            check(lib().mpe_resolve(self.device_id, C.byref(st), env.data_ptr(), *read, b["occluded"].data_ptr(), b["sums"].data_ptr(),
                                    b["out"].data_ptr() if last else None, stream))
            if visibility:
                _sec.check(sec.mps_resolve(self.device_id, C.byref(ao_st), b["tmax"].data_ptr(), b["occluded"].data_ptr(),
                                           b["counts"].data_ptr(), b["ao"].data_ptr() if last else None, stream))
        if visibility:
            return b["out"], b["sums"], b["ao"], b["counts"]
        return b["out"], b["sums"]

    def last_kernels(self) -> list:
        """The kernel the calling thread's last launching call of this library launched (mpe_last_kernels)."""
        return last_kernels()
