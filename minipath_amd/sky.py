"""Sky lighting from the feature planes (include/minipath_sky.h, sky/libminipath_sky.so).

A library of its own beside libminipath_hip.so, like the lights': it reduces the answers of the occlusion query on the
cosine-distributed rays of the ambient occlusion (mps_generate of libminipath_secondary.so) once more, with the rays' directions:
every ray that escapes looks its direction up in an octahedral environment map.  It is loaded on first use, so ``import
minipath_amd`` works where it was not built; there is no other compute path (a missing library raises).
"""
from __future__ import annotations

import ctypes as C
import math

from . import _postlib
from . import secondary as _sec
from ._traced import TracedStage

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

LIBRARY = _postlib.PostLibrary("sky", "mpe", SIGNATURES, "the sky lighting has no CPU fallback")
lib, check, last_kernels = LIBRARY.load, LIBRARY.check, LIBRARY.last_kernels


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


class SkyLight(TracedStage):
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

    library, runs_on = LIBRARY, "the sky lighting runs on the GPU"
    planes, max_samples = ("sums", "out", "counts", "ao"), MPE_MAX_SAMPLES

    def __init__(self, scene, resolution, device=None, batch: int = 2):
        super().__init__(scene, resolution, device, batch)
        check(lib().mpe_check_settings(C.byref(self.batch_settings(self.batch, 0, self.batch, 1, 1))))

    def batch_settings(self, samples, begin, batch, map_size, pole) -> SkySettings:
        """The mpe_settings of the batch [begin, begin + batch) of `samples` samples; it accumulates iff begin != 0.  The batch's
        rays are those of secondary.batch_settings(width, height, MPS_MODE_AO, samples, begin, batch, ...)."""
        return SkySettings(C.sizeof(SkySettings), self.width, self.height, MPE_FLAG_ACCUMULATE if begin else 0, int(samples), int(begin),
                           int(batch), int(map_size), int(pole))

    def _env(self, env):
        import torch

        n = env.shape[0] if isinstance(env, torch.Tensor) and env.dim() == 3 else 0
        if not 0 < n <= MPE_MAX_MAP:
            raise ValueError(f"env: a contiguous float32 [N, N, 4] tensor on {self.device}, 1 <= N <= {MPE_MAX_MAP}, is expected")
        return _postlib.expect_plane(env, "env", self.device, self.device_id, (n, n, 4)), n

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
        samples = self._samples(samples)
        # a bad pole is refused here, before the first batch's rays are written
        check(lib().mpe_check_settings(C.byref(self.batch_settings(samples, 0, min(self.batch, samples), n_map, pole))))

        def settings(begin, n):  # the pair: this library's, and the ambient occlusion's for the rays and the visibility
            return (self.batch_settings(samples, begin, n, n_map, pole),
                    _sec.batch_settings(self.width, self.height, _sec.MPS_MODE_AO, samples, begin, n, seed, eye, radius=radius, bias=bias))

        def resolve(st, b, last, stream):
            check(lib().mpe_resolve(self.device_id, C.byref(st[0]), env.data_ptr(), *[b[k].data_ptr() for k in READ_ARRAYS],
                                    b["occluded"].data_ptr(), b["sums"].data_ptr(), b["out"].data_ptr() if last else None, stream))

        def resolve_visibility(st, b, last, stream):
            _sec.resolve(self.device_id, st[1], b, b["ao"] if last else None, stream)

        b = self._trace(samples, 1, settings, lambda st, b, stream: _sec.generate(self.device_id, st[1], position, normal, b, stream),
                        resolve, *([resolve_visibility] if visibility else []))
        if visibility:
            return b["out"], b["sums"], b["ao"], b["counts"]
        return b["out"], b["sums"]
