"""Guided half-resolution resampling for plane-traced visibility (include/minipath_resample.h,
resample/libminipath_resample.so).

A library of its own beside libminipath_hip.so, like the denoiser's: it picks one real surface point per f x f block of the
image-major [h, w, 4] "position" and "normal" planes FrameRenderer.untile_plane produces, copies the planes there to low resolution,
and brings a low-resolution colour back to full resolution with a 3 x 3 filter guided by the full-resolution geometry.  It is loaded
on first use, so ``import minipath_amd`` works where it was not built; there is no other compute path (a missing library raises).
"""
from __future__ import annotations

import ctypes as C

from . import _postlib

MPR_PICK_PHASE, MPR_PICK_NEAREST = 0, 1
MPR_PICK_NONE = 0xFFFFFFFF
MPR_MAX_PLANES = 4
PICK_MODES = {"phase": MPR_PICK_PHASE, "nearest": MPR_PICK_NEAREST}
# The shipped weights: the best of a CPU sweep of the model on the teapot case of tests/resample_cases.py
# (tools/sweep_resample.py, profiles/resample_notes.md)
DEFAULT_SIGMA_NORMAL_POW2 = 1
DEFAULT_SIGMA_PLANE = 0.01


class ResampleSettings(C.Structure):
    """mpr_settings."""

    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("factor", C.c_uint32),
                ("pick_mode", C.c_uint32), ("phase", C.c_uint32), ("sigma_normal_pow2", C.c_float), ("sigma_plane", C.c_float)]


# name -> (restype, argtypes); every symbol include/minipath_resample.h declares
SIGNATURES = {
    "mpr_last_error": (C.c_char_p, []),
    "mpr_settings_size": (C.c_uint32, []),
    "mpr_check_settings": (C.c_int, [C.POINTER(ResampleSettings)]),
    "mpr_low_size": (C.c_int, [C.POINTER(ResampleSettings), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mpr_downsample": (C.c_int, [C.c_int, C.POINTER(ResampleSettings), C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]),
    "mpr_upsample": (C.c_int, [C.c_int, C.POINTER(ResampleSettings)] + [C.c_void_p] * 8),
    "mpr_last_kernels": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
}

LIBRARY = _postlib.PostLibrary("resample", "mpr", SIGNATURES, "the resampling has no CPU fallback")
lib, check, last_kernels = LIBRARY.load, LIBRARY.check, LIBRARY.last_kernels


def pointer_array(pointers):
    """the host array of device pointers mpr_downsample takes"""
    return (C.c_void_p * max(len(pointers), 1))(*pointers)


class GuidedResampler(_postlib.Stage):
    """Guided resampling (include/minipath_resample.h) between one full resolution (width, height) and its f-th, f = `factor` in
    2..4: `low_resolution` = (ceil(width / f), ceil(height / f)).  Secondary visibility is traced at the low resolution, f * f times
    fewer rays, from real surface points -- one picked pixel per f x f block, never a mean across an edge -- and brought back with a
    3 x 3 filter over the low pixels that weighs each by its pick's distance, by the normals' agreement (the cosine squared
    `sigma_normal_pow2` times) and by the pick's distance from the full pixel's tangent plane (`sigma_plane`, as a fraction of the
    pixel's hit distance).  A full pixel without a usable low neighbour takes the nearest one's colour, or comes out as a miss.

        fr = mp.FrameRenderer(scene, camera, settings)
        planes = fr.new_aov_planes(position=True)
        fr.render_aov_pass(planes)                                              # render_aov_pass
        position, normal, ids = (fr.untile_plane(planes[k]) for k in ("position", "normal", "ids"))   # untile_plane
        rs = mp.GuidedResampler(resolution, factor=2)
        position_lo, normal_lo, ids_lo = rs.downsample(position, normal, ids, phase=frame % 4)
        sv = mp.SecondaryVisibility(scene, rs.low_resolution)
        ao_lo, _ = sv.ambient_occlusion(position_lo, normal_lo, camera, samples=8, radius=1.5, seed=frame)
        ao = rs.upsample(ao_lo, position, normal)
        out, var = acc.accumulate(ao, position, normal, ids,
                                  mp.TemporalAccumulator.view_of(camera, resolution))   # TemporalAccumulator.accumulate
        clean, _ = dn.denoise(out, normal, variance=var)                        # AtrousDenoiser.denoise, at full resolution

    Advancing `phase` by one per frame picks another pixel of every block, so the temporal stage sees every pixel of a block traced
    over f * f frames.  pick="nearest" takes each block's valid pixel of the smallest hit distance instead (the foreground).

    Both calls run on the current torch stream without a host synchronisation.  The low planes, `picks` and the upsampled plane are
    this object's own: the next call overwrites them, so copy what has to live longer.  upsample uses the picks and the low position
    and normal of the last downsample.
    """

    library, runs_on = LIBRARY, "the resampling runs on the GPU"

    def __init__(self, resolution, factor: int = 2, device=None, sigma_normal_pow2: int = DEFAULT_SIGMA_NORMAL_POW2,
                 sigma_plane: float = DEFAULT_SIGMA_PLANE):
        import torch

        if device is None:
            device = torch.cuda.current_device()
        super().__init__(resolution, device)
        self.factor = int(factor)
        self.sigma_normal_pow2, self.sigma_plane = float(sigma_normal_pow2), float(sigma_plane)
        lw, lh = C.c_uint32(), C.c_uint32()
        check(lib().mpr_low_size(C.byref(self._settings(MPR_PICK_PHASE, 0)), C.byref(lw), C.byref(lh)))
        self.low_resolution = (lw.value, lh.value)
        self.picks = None   # uint32 [h, w] as int32 words, made by downsample
        self._low = []      # the low planes of the last downsample: position, normal, extras
        self._out = None

    def _settings(self, pick_mode, phase) -> ResampleSettings:
        return ResampleSettings(C.sizeof(ResampleSettings), self.width, self.height, self.factor, int(pick_mode), int(phase),
                                self.sigma_normal_pow2, self.sigma_plane)

    def _plane(self, t, name, low=False, words=False):
        import torch

        # words: uint32 is taken too, the message names the two kinds callers have
        dtypes, kinds = ((torch.float32, torch.int32, torch.uint32), "float32 or int32") if words else (None, None)
        return super()._plane(t, name, dtypes, kinds, self.low_resolution if low else None)

    def downsample(self, position, normal, *extra, phase: int = 0, pick: str = "phase"):
        """(position_lo, normal_lo, *extra_lo): the planes at each block's picked pixel, bit for bit, zeros where a block has no
        valid pixel; `picks` (int32 words [h, w]: y * width + x, or -1) is kept for upsample.  position {p.x, p.y, p.z, alpha} and
        normal {n.x, n.y, n.z, t} are untiled float32 planes; up to two `extra` planes of 4-byte words (the int32 "ids") are taken
        along.  All are only read.  pick = "phase": the pixel (phase % f, phase / f) of the block, or its first valid pixel;
        "nearest": the valid pixel of the smallest hit distance."""
        import torch

        if pick not in PICK_MODES:
            raise ValueError(f"pick: one of {sorted(PICK_MODES)} is expected")
        if len(extra) + 2 > MPR_MAX_PLANES:
            raise ValueError(f"at most {MPR_MAX_PLANES - 2} extra planes")
        position, normal = self._plane(position, "position"), self._plane(normal, "normal")
        sources = [position, normal] + [self._plane(t, f"extra[{i}]", words=True) for i, t in enumerate(extra)]
        lw, lh = self.low_resolution
        if self.picks is None:
            self.picks = torch.empty((lh, lw), dtype=torch.int32, device=self.device)
        for i, s in enumerate(sources):  # this object's planes, made once per dtype
            if i == len(self._low):
                self._low.append(None)
            if self._low[i] is None or self._low[i].dtype != s.dtype:
                self._low[i] = torch.empty((lh, lw, 4), dtype=s.dtype, device=self.device)
        low = self._low[:len(sources)]
        st = self._settings(PICK_MODES[pick], phase)
        check(lib().mpr_downsample(self.device_id, C.byref(st), position.data_ptr(), normal.data_ptr(), len(sources),
                                   pointer_array([s.data_ptr() for s in sources]), pointer_array([d.data_ptr() for d in low]),
                                   self.picks.data_ptr(), self._stream()))
        return tuple(low)

    def upsample(self, color_lo, position, normal):
        """out {r, g, b, 1} [height, width, 4]: the low-resolution colour {r, g, b, alpha} (alpha == 0: not used) filtered to the
        full-resolution pixels the position and normal planes describe, with the picks and the low planes of the last downsample;
        zeros at misses and where no low neighbour is usable."""
        import torch

        if self.picks is None:
            raise ValueError("upsample needs the picks of a downsample")
        color_lo = self._plane(color_lo, "color_lo", low=True)
        position, normal = self._plane(position, "position"), self._plane(normal, "normal")
        if self._out is None:
            self._out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=self.device)
        st = self._settings(MPR_PICK_PHASE, 0)
        check(lib().mpr_upsample(self.device_id, C.byref(st), position.data_ptr(), normal.data_ptr(), self._low[0].data_ptr(),
                                 self._low[1].data_ptr(), self.picks.data_ptr(), color_lo.data_ptr(), self._out.data_ptr(), self._stream()))
        return self._out
