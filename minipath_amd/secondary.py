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

from ._postlib import PostLibrary
from ._traced import TRACED_ARRAYS, TracedStage

MPS_MODE_AO, MPS_MODE_SUN = 0, 1
MPS_FLAG_ACCUMULATE = 1
MPS_MAX_SAMPLES = 65536
RAY_ARRAYS = TRACED_ARRAYS


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

LIBRARY = PostLibrary("secondary", "mps", SIGNATURES, "the secondary rays have no CPU fallback")
lib, check, last_kernels = LIBRARY.load, LIBRARY.check, LIBRARY.last_kernels


def batch_settings(width, height, mode, samples, begin, batch, seed, eye, light=(0.0, 0.0, 1.0), radius=math.inf, bias=1e-4,
                   spread=0.0) -> SecondarySettings:
    """The mps_settings of the batch [begin, begin + batch) of `samples` samples; it accumulates iff begin != 0."""
    st = SecondarySettings(C.sizeof(SecondarySettings), width, height, mode, MPS_FLAG_ACCUMULATE if begin else 0, int(samples), int(begin),
                           int(batch), int(seed) & 0xFFFFFFFFFFFFFFFF)
    st.eye[:], st.light[:] = [float(v) for v in eye], [float(v) for v in light]
    st.radius, st.bias, st.spread = float(radius), float(bias), float(spread)
    return st


def generate(device_id, st, position, normal, b, stream) -> None:
    """mps_generate: the batch's rays from the planes into the RAY_ARRAYS of the buffers `b`"""
    check(lib().mps_generate(device_id, C.byref(st), position.data_ptr(), normal.data_ptr(), *[b[k].data_ptr() for k in RAY_ARRAYS], stream))


def resolve(device_id, st, b, out, stream) -> None:
    """mps_resolve: the batch's answers in `b` into b["counts"] and, unless `out` is None, the visibility plane `out`"""
    check(lib().mps_resolve(device_id, C.byref(st), b["tmax"].data_ptr(), b["occluded"].data_ptr(), b["counts"].data_ptr(),
                            None if out is None else out.data_ptr(), stream))


class SecondaryVisibility(TracedStage):
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

    library, runs_on = LIBRARY, "the secondary rays run on the GPU"
    planes, max_samples = ("counts", "out"), MPS_MAX_SAMPLES

    def __init__(self, scene, resolution, device=None, batch: int = 4):
        super().__init__(scene, resolution, device, batch)
        check(lib().mps_check_settings(C.byref(batch_settings(self.width, self.height, MPS_MODE_AO, self.batch, 0, self.batch, 0, (0, 0, 0),
                                                              radius=1.0, bias=0.0))))

    def _run(self, mode, position, normal, eye, light, samples, radius, seed, bias, spread):
        position, normal = self._plane(position, "position"), self._plane(normal, "normal")
        if hasattr(eye, "center_forward_up_right"):
            eye = self.eye_of(eye)
        samples = self._samples(samples)
        b = self._trace(samples, 1,
                        lambda begin, n: batch_settings(self.width, self.height, mode, samples, begin, n, seed, eye, light, radius, bias, spread),
                        lambda st, b, stream: generate(self.device_id, st, position, normal, b, stream),
                        lambda st, b, last, stream: resolve(self.device_id, st, b, b["out"] if last else None, stream))
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
