"""Edge-avoiding a-trous denoiser over the feature planes (include/minipath_denoise.h, denoise/libminipath_denoise.so).

A library of its own beside libminipath_hip.so: it filters image-major [h, w, 4] float32 planes as FrameRenderer.untile /
untile_plane produce them and needs no Context and no scene.  It is loaded on first use, so ``import minipath_amd`` works where
only libminipath_hip.so was built; there is no other compute path (a missing library raises).
"""
from __future__ import annotations

import ctypes as C

from . import _postlib

MPD_FLAG_DEMODULATE_ALBEDO = 1
MPD_MAX_ITERATIONS = 8


class DenoiseSettings(C.Structure):
    """mpd_settings."""

    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32),
                ("sigma_normal_pow2", C.c_float), ("sigma_depth", C.c_float), ("sigma_luminance", C.c_float), ("flags", C.c_uint32)]


# name -> (restype, argtypes); every symbol include/minipath_denoise.h declares
SIGNATURES = {
    "mpd_last_error": (C.c_char_p, []),
    "mpd_settings_size": (C.c_uint32, []),
    "mpd_scratch_floats": (C.c_size_t, [C.POINTER(DenoiseSettings), C.c_int]),
    "mpd_atrous": (C.c_int, [C.c_int, C.POINTER(DenoiseSettings)] + [C.c_void_p] * 8),
    "mpd_variance_from_moments": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4),
    "mpd_last_kernels": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
}

LIBRARY = _postlib.PostLibrary("denoise", "mpd", SIGNATURES, "the denoiser has no CPU fallback")
lib, check, last_kernels = LIBRARY.load, LIBRARY.check, LIBRARY.last_kernels


class AtrousDenoiser(_postlib.Stage):
    """The filter of include/minipath_denoise.h for one resolution (width, height) on one device; owns the scratch planes.

    iterations passes with tap spacing 1, 2, 4, ...; the normal weight is max(0, n_p . n_q) squared sigma_normal_pow2 times, the
    depth weight 1 / (1 + (|t_p - t_q| / (sigma_depth * spacing))^2), the luminance weight 1 / (1 + (|l_p - l_q| / den)^2) with
    den = sigma_luminance (sums of r + g + b) or, with a variance plane, sigma_luminance standard deviations of the pixel.
    sigma_depth is in the scene's length unit per pixel of spacing; the defaults suit scenes a few units across, seen as in the tests.
    demodulate_albedo: filter colour / albedo and multiply the albedo back (keeps texture detail out of the filter).

        fr = mp.FrameRenderer(scene, camera, settings)
        planes = fr.new_aov_planes(ids=False, shade_sq=True)
        fr.render_aov_pass(planes)                                   # the guides of the beauty frame's primary hits
        beauty = fr.untile(fr.render(), want_u8=False)[0]            # [h, w, 4], any max_depth
        dn = mp.AtrousDenoiser(settings.resolution, fr.device, demodulate_albedo=True)
        clean = dn.denoise(beauty, fr.untile_plane(planes["normal"]), albedo=fr.untile_plane(planes["albedo"]))
        # the first-hit shade with its own variance:
        var = dn.variance_from_moments(fr.untile_plane(planes["shade"]), fr.untile_plane(planes["shade_sq"]), settings.sample_count)
        shade, shade_var = dn.denoise(fr.untile_plane(planes["shade"]), fr.untile_plane(planes["normal"]), variance=var)
    """

    library, runs_on, none_passes = LIBRARY, "the denoiser runs on the GPU", True

    def __init__(self, resolution, device=0, iterations: int = 5, sigma_normal_pow2: int = 7, sigma_depth: float = 0.2,
                 sigma_luminance: float = 1.5, demodulate_albedo: bool = False, scratch=None):
        super().__init__(resolution, device)
        self.settings = DenoiseSettings(C.sizeof(DenoiseSettings), self.width, self.height, int(iterations), float(sigma_normal_pow2),
                                        float(sigma_depth), float(sigma_luminance), MPD_FLAG_DEMODULATE_ALBEDO if demodulate_albedo else 0)
        if lib().mpd_scratch_floats(C.byref(self.settings), 0) == 0:
            check(lib().mpd_atrous(self.device_id, C.byref(self.settings), *([None] * 8)))  # raises with the library's reason
        self._owns_scratch = scratch is None
        self._scratch = scratch  # a caller's float32 tensor of scratch_floats(...) elements, or allocated on first use

    def scratch_floats(self, with_variance: bool) -> int:
        return int(lib().mpd_scratch_floats(C.byref(self.settings), 1 if with_variance else 0))

    def denoise(self, color, normal_depth, albedo=None, variance=None, out=None, variance_out=None):
        """mpd_atrous on the current torch stream: `out`, or (`out`, `variance_out`) when a variance plane is given.  The planes
        are image-major [h, w, 4] float32: colour {r, g, b, alpha} (alpha 0 = a miss, passed through), the "normal" plane
        {n.x, n.y, n.z, t}, "albedo" (needed with demodulate_albedo), variance {v, -, -, -}.  The inputs are only read.  `out` /
        `variance_out`: tensors to write into instead of new ones."""
        import torch

        color, normal_depth = self._plane(color, "color"), self._plane(normal_depth, "normal_depth")
        albedo, variance = self._plane(albedo, "albedo"), self._plane(variance, "variance")
        if color is None or normal_depth is None:
            raise ValueError("color and normal_depth are required")
        need = self.scratch_floats(variance is not None)
        if self._scratch is None or (self._owns_scratch and self._scratch.numel() < need):
            self._scratch, self._owns_scratch = torch.empty(need, dtype=torch.float32, device=self.device), True
        if self._scratch.numel() < need:
            raise ValueError(f"scratch: {need} floats are needed")
        if not (self._scratch.dtype == torch.float32 and self._scratch.is_contiguous() and self._scratch.device.index == self.device_id):
            raise ValueError("scratch: a contiguous float32 tensor on the denoiser's device is expected")
        out = torch.empty_like(color) if out is None else self._plane(out, "out")
        if variance is not None and variance_out is None:
            variance_out = torch.empty_like(color)
        variance_out = self._plane(variance_out, "variance_out")
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        check(lib().mpd_atrous(self.device_id, C.byref(self.settings), ptr(color), ptr(normal_depth), ptr(albedo), ptr(variance),
                               self._scratch.data_ptr(), ptr(out), ptr(variance_out), self._stream()))
        return out if variance is None else (out, variance_out)

    def variance_from_moments(self, shade, shade_sq, sample_count: int, out=None):
        """mpd_variance_from_moments on the current torch stream: the variance of each pixel's mean {v, 0, 0, 0} from the "shade"
        and "shade_sq" planes of render_aov_pass() after sample_count samples (untiled)."""
        import torch

        shade, shade_sq = self._plane(shade, "shade"), self._plane(shade_sq, "shade_sq")
        if shade is None or shade_sq is None:
            raise ValueError("shade and shade_sq are required")
        out = torch.empty_like(shade) if out is None else self._plane(out, "out")
        check(lib().mpd_variance_from_moments(self.device_id, self.width, self.height, int(sample_count), shade.data_ptr(),
                                              shade_sq.data_ptr(), out.data_ptr(), self._stream()))
        return out
