"""Point and sphere lights traced from the feature planes (include/minipath_lights.h, lights/libminipath_lights.so).

A library of its own beside libminipath_hip.so, like the secondary rays': it turns the image-major [h, w, 4] "position" and "normal"
planes FrameRenderer.untile_plane produces into bounded shadow rays, one per light and sample, in the SoA buffers mp_occluded_rays
takes, and reduces that query's answers to an irradiance plane.  It is loaded on first use, so ``import minipath_amd`` works where
it was not built; there is no other compute path (a missing library raises).
"""
from __future__ import annotations

import ctypes as C

from ._postlib import PostLibrary
from ._traced import TRACED_ARRAYS, TracedStage

MPL_FLAG_ACCUMULATE = 1
MPL_MAX_LIGHTS = 8
MPL_MAX_SAMPLES = 65536
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

LIBRARY = PostLibrary("lights", "mpl", SIGNATURES, "the lights have no CPU fallback")
lib, check, last_kernels = LIBRARY.load, LIBRARY.check, LIBRARY.last_kernels


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


class LocalLights(TracedStage):
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

    library, runs_on = LIBRARY, "the lights run on the GPU"
    ray_arrays, planes, max_samples = RAY_ARRAYS, ("sums", "out"), MPL_MAX_SAMPLES

    def __init__(self, scene, resolution, device=None, batch: int = 2):
        super().__init__(scene, resolution, device, batch)
        one = light_table([((0.0, 0.0, 0.0), 0.0, (1.0, 1.0, 1.0))])
        check(lib().mpl_check_settings(C.byref(self.batch_settings(self.batch, 0, self.batch, 1, 0, (0, 0, 0), 0.0, 0.0)), one))

    def batch_settings(self, samples, begin, batch, light_count, seed, eye, bias, margin) -> LightsSettings:
        """The mpl_settings of the batch [begin, begin + batch) of `samples` samples; it accumulates iff begin != 0."""
        st = LightsSettings(C.sizeof(LightsSettings), self.width, self.height, MPL_FLAG_ACCUMULATE if begin else 0, int(samples), int(begin),
                            int(batch), int(light_count), int(seed) & 0xFFFFFFFFFFFFFFFF)
        st.eye[:] = [float(v) for v in eye]
        st.bias, st.margin = float(bias), float(margin)
        return st

    def irradiance(self, position, normal, eye, lights, samples: int, seed: int = 0, bias: float = 1e-4, margin: float = 0.0):
        """(out, sums): `samples` shadow rays per hit pixel and light from position + n * bias, n the normal turned towards `eye` (a
        Camera, or the three coordinates of its lens centre: eye_of), to the light, `margin` short of it.  `lights`: a sequence of
        (position, radius, intensity) or an [L, 8] array, at most 8.  out = {E.r, E.g, E.b, alpha}; sums = {sum.r, sum.g, sum.b,
        counted}.  Surfaces that face away from a light, or lie inside it or within `margin` of it, get nothing from it without a
        trace.  position {p.x, p.y, p.z, alpha} and normal {n.x, n.y, n.z, t} are untiled float32 planes and are only read."""
        position, normal = self._plane(position, "position"), self._plane(normal, "normal")
        if hasattr(eye, "center_forward_up_right"):
            eye = self.eye_of(eye)
        samples = self._samples(samples)
        table = light_table(lights)

        def generate(st, b, stream):
            check(lib().mpl_generate(self.device_id, C.byref(st), table, position.data_ptr(), normal.data_ptr(),
                                     *[b[k].data_ptr() for k in RAY_ARRAYS], stream))

        def resolve(st, b, last, stream):
            check(lib().mpl_resolve(self.device_id, C.byref(st), table, b["tmax"].data_ptr(), b["weight"].data_ptr(), b["occluded"].data_ptr(),
                                    b["sums"].data_ptr(), b["out"].data_ptr() if last else None, stream))

        b = self._trace(samples, len(table), lambda begin, n: self.batch_settings(samples, begin, n, len(table), seed, eye, bias, margin),
                        generate, resolve)
        return b["out"], b["sums"]
