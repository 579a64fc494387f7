"""Temporal reprojection across camera moves (include/minipath_temporal.h, temporal/libminipath_temporal.so).

A library of its own beside libminipath_hip.so, like the denoiser's: it works on image-major [h, w, 4] planes as
FrameRenderer.untile / untile_plane produce them and needs no Context and no scene.  It is loaded on first use, so
``import minipath_amd`` works where it was not built; there is no other compute path (a missing library raises).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _postlib

MPT_FLAG_MATCH_PRIM = 1


class TemporalView(C.Structure):
    """mpt_view."""

    _fields_ = [("center", C.c_float * 3), ("forward", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3), ("k", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float)]


class TemporalSettings(C.Structure):
    """mpt_settings."""

    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32),
                ("sigma_position", C.c_float), ("normal_min", C.c_float), ("max_history", C.c_float), ("alpha_color", C.c_float),
                ("alpha_moments", C.c_float), ("min_variance_history", C.c_float)]


# name -> (restype, argtypes); every symbol include/minipath_temporal.h declares
SIGNATURES = {
    "mpt_last_error": (C.c_char_p, []),
    "mpt_settings_size": (C.c_uint32, []),
    "mpt_check_settings": (C.c_int, [C.POINTER(TemporalSettings)]),
    "mpt_reproject": (C.c_int, [C.c_int, C.POINTER(TemporalSettings), C.POINTER(TemporalView)] + [C.c_void_p] * 14),
    "mpt_reset": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5),
    "mpt_last_kernels": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
}

LIBRARY = _postlib.PostLibrary("temporal", "mpt", SIGNATURES, "the reprojection has no CPU fallback")
lib, check, last_kernels = LIBRARY.load, LIBRARY.check, LIBRARY.last_kernels


class TemporalAccumulator(_postlib.Stage):
    """The temporal stage of include/minipath_temporal.h for one resolution (width, height) on one device: it owns the history
    (two ping-pong sets of colour, luminance moments, position, normal and ids), remembers the last view, and carries every pixel's
    accumulated colour over to the next frame through its world-space hit point.

    A tap of the previous frame is taken when it shows the same instance and material (match_prim: the same triangle too), its hit
    point lies within sigma_position * (hit distance) of the pixel's, and its normal's cosine to the pixel's is at least
    normal_min.  A pixel whose history has length N takes the new colour with the weight max(1 / N, alpha_color), N growing by one
    per frame up to max_history; the luminance moments likewise with alpha_moments.  Below a history of min_variance_history frames
    the variance handed on is the caller's `variance` (when given) instead of the temporal one.

        acc = mp.TemporalAccumulator(resolution, device)
        dn = mp.AtrousDenoiser(resolution, device)
        for i, camera_i in enumerate(cameras):                              # static scene, moving camera
            st = mp.RenderSettings(tile_size, spp, resolution, seed=seed + i, max_depth=3)
            fr = mp.FrameRenderer(scene, camera_i, st)
            planes = fr.new_aov_planes(shade=False, albedo=False, position=True)
            fr.render_aov_pass(planes)                                      # the guides of the frame's primary hits
            color = fr.untile(fr.render(), want_u8=False)[0]
            normal = fr.untile_plane(planes["normal"])
            out, var = acc.accumulate(color, fr.untile_plane(planes["position"]), normal, fr.untile_plane(planes["ids"]),
                                      mp.TemporalAccumulator.view_of(camera_i, resolution))
            clean, _ = dn.denoise(out, normal, variance=var)

    `out` and `var` are the accumulator's own planes: they are the history of the next call and are overwritten by the call after
    it, so copy what has to live longer.
    """

    library, runs_on, none_passes = LIBRARY, "the reprojection runs on the GPU", True

    def __init__(self, resolution, device=0, sigma_position: float = 0.01, normal_min: float = 0.9, max_history: float = 32.0,
                 alpha_color: float = 0.2, alpha_moments: float = 0.2, min_variance_history: float = 4.0, match_prim: bool = False):
        super().__init__(resolution, device)
        self.settings = TemporalSettings(C.sizeof(TemporalSettings), self.width, self.height, MPT_FLAG_MATCH_PRIM if match_prim else 0,
                                         float(sigma_position), float(normal_min), float(max_history), float(alpha_color),
                                         float(alpha_moments), float(min_variance_history))
        check(lib().mpt_check_settings(C.byref(self.settings)))  # raises with the library's reason
        self._sets = None  # two dicts of planes, made on first use
        self._cur = 0
        self._view = None  # the view of the frame in self._sets[self._cur]; None = no history

    @staticmethod
    def view_of(camera, resolution) -> TemporalView:
        """The mpt_view of a Camera at a resolution: the pinhole through the lens centre of camera.build_sampler(resolution)."""
        center, forward, up, right = camera.center_forward_up_right()
        w, h = int(resolution[0]), int(resolution[1])
        ps = np.float32(camera.build_sampler(resolution).as_array()[12])  # pixel_scale
        v = TemporalView()
        v.center[:], v.forward[:], v.right[:], v.up[:] = center.tolist(), forward.tolist(), right.tolist(), up.tolist()
        v.k = np.float32(camera.focal_length) / ps
        v.cx = np.float32(w - 1) * np.float32(0.5)
        v.cy = np.float32(h - 1) * np.float32(0.5)
        return v

    def _new_set(self):
        import torch

        shape = (self.height, self.width, 4)
        s = {k: torch.empty(shape, dtype=torch.float32, device=self.device) for k in ("color", "moments", "position", "normal", "variance")}
        s["ids"] = torch.empty(shape, dtype=torch.int32, device=self.device)
        return s

    def reset(self) -> None:
        """Forget the history: the next frame is a first frame."""
        self._view = None

    def accumulate(self, color, position, normal, ids, view, variance=None):
        """One frame on the current torch stream: (out, var), both image-major [h, w, 4] float32.  mpt_reset on a first frame (and
        the first after reset()), mpt_reproject with the remembered view and history otherwise.  color {r, g, b, a}, position
        {p.x, p.y, p.z, alpha}, normal {n.x, n.y, n.z, t} are float32 planes, ids {prim, instance, material, hit} int32, all
        untiled; view is view_of() of the frame's camera; variance {v, -, -, -} optionally the frame's own variance for pixels with
        a young history (AtrousDenoiser.variance_from_moments).  The guide planes are copied into the accumulator, so the caller
        may overwrite theirs at once.  var is {v, 0, 0, 0}; beside a first frame, which has no temporal variance, it is `variance`
        as it is while 1 < min_variance_history, else zeros."""
        import torch

        color, position, normal = self._plane(color, "color"), self._plane(position, "position"), self._plane(normal, "normal")
        ids, variance = self._plane(ids, "ids", (torch.int32, torch.uint32)), self._plane(variance, "variance")
        if color is None or position is None or normal is None or ids is None:
            raise ValueError("color, position, normal and ids are required")
        if not isinstance(view, TemporalView):
            raise ValueError("view: TemporalAccumulator.view_of(camera, resolution) is expected")
        if self._sets is None:
            self._sets = [self._new_set(), self._new_set()]
        prev, cur = self._sets[self._cur], self._sets[self._cur ^ 1]
        cur["position"].copy_(position)
        cur["normal"].copy_(normal)
        cur["ids"].copy_(ids.view(torch.int32))
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        if self._view is None:
            check(lib().mpt_reset(self.device_id, self.width, self.height, ptr(color), ptr(cur["position"]), ptr(cur["color"]),
                                  ptr(cur["moments"]), self._stream()))
            if variance is not None and 1.0 < self.settings.min_variance_history:
                cur["variance"].copy_(variance)
            else:
                cur["variance"].zero_()
        else:
            check(lib().mpt_reproject(self.device_id, C.byref(self.settings), C.byref(self._view), ptr(color), ptr(cur["position"]),
                                      ptr(cur["normal"]), ptr(cur["ids"]), ptr(variance), ptr(prev["position"]), ptr(prev["normal"]),
                                      ptr(prev["ids"]), ptr(prev["color"]), ptr(prev["moments"]), ptr(cur["color"]), ptr(cur["moments"]),
                                      ptr(cur["variance"]), self._stream()))
        self._cur ^= 1
        self._view = TemporalView.from_buffer_copy(view)
        return cur["color"], cur["variance"]

    def history_length(self):
        """[h, w] float32: the history length N of every pixel after the last frame (0 at a miss); a view of the moments plane."""
        if self._sets is None or self._view is None:
            raise ValueError("no frame has been accumulated")
        return self._sets[self._cur]["moments"][..., 2]
