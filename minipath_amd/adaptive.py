"""Adaptive sampling: tiles stop drawing samples once the standard error of their shade is below a threshold
(include/minipath_adaptive.h, adaptive/libminipath_adaptive.so).

A library of its own beside libminipath_hip.so, as the denoiser's: it works on the tile-major planes of
FrameRenderer.render_aov_pass and needs no Context.  It is loaded on first use, so ``import minipath_amd`` works where only
libminipath_hip.so was built; there is no other compute path (a missing library raises).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, _postlib
from .renderer import FrameRenderer

# name -> (restype, argtypes); every symbol include/minipath_adaptive.h declares
SIGNATURES = {
    "mpa_last_error": (C.c_char_p, []),
    "mpa_tile_error": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float] + [C.c_void_p] * 6),
    "mpa_move_tiles": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                 C.c_void_p, C.c_void_p]),
    "mpa_finish_tiles": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4),
    "mpa_last_kernels": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
}

LIBRARY = _postlib.PostLibrary("adaptive", "mpa", SIGNATURES, "adaptive sampling has no CPU fallback")
lib, check, last_kernels = LIBRARY.load, LIBRARY.check, LIBRARY.last_kernels


def round_bounds(sample_count: int, min_samples: int, round_samples: int) -> list:
    """The sample boundaries of the rounds: 0, min_samples, min_samples + round_samples, ..., clipped to sample_count (its last
    element).  Round r draws the samples [b[r], b[r + 1]); a convergence check follows every round that ends below sample_count."""
    if sample_count < 1 or min_samples < 1 or round_samples < 1:
        raise ValueError("sample_count, min_samples and round_samples are at least 1")
    b = [0, min(min_samples, sample_count)]
    while b[-1] < sample_count:
        b.append(min(b[-1] + round_samples, sample_count))
    return b


class AdaptiveSampler:
    """Renders the first-hit planes of FrameRenderer.render_aov_pass in rounds and stops each tile at the first round boundary
    at which all of its pixels have a relative standard error of the shade of at most `threshold`:

        e = sqrt(max(E[c^2] - E[c]^2, 0) / k) / (E[c] + floor)          (mpa_tile_error, include/minipath_adaptive.h)

    over all k samples drawn so far, misses included.  The rounds end at round_bounds(sample_count, min_samples, round_samples);
    a tile that never converges draws settings.sample_count samples and is bit for bit the tile of the plain render.  A tile that
    stops after k_i samples holds, after finish(), exactly the preview of the plain render after k_i samples (sums * (1 / k_i)).
    Progressive passes give the same bits for any split, so the frame depends on (settings, threshold, floor, schedule) alone.

        ad = mp.AdaptiveSampler(scene, camera, settings, threshold=0.05, planes=("shade", "shade_sq", "normal", "albedo"))
        ad.render()
        shade = ad.untile_plane("shade")        # [h, w, 4]
        spp = ad.sample_map()                   # [h, w] int32: the samples each pixel drew

    `planes`: "shade" and "shade_sq" always (the test reads them); any other plane of FrameRenderer.AOV_PLANES rides along.
    `self.planes` are the canonical tile-major planes (slot i = tile i of the renderer's full tile list) and are authoritative
    between rounds: they and `samples` are the checkpoint of the render.

    One host synchronisation per round is inherent: the tile list of the next pass is a host argument of
    mp_render_aov_pass_device, so the host reads the round's `open` counts before it can issue the next round.  It is the only one:
    a round without a check (the last) and finish() are enqueued on the current torch stream without waiting for it, once the
    context holds the round's tile list (a list it has not seen is uploaded with a blocking copy, once).  While every tile is
    active the passes render straight into the canonical planes; afterwards the active slots are gathered into compact work planes
    (mpa_move_tiles), rendered and checked there, and scattered back.

    Not supported (ValueError): MP_FLAG_CHUNKED_SUM, MP_FLAG_WAVEFRONT, MP_FLAG_TRAVERSAL_GROUPS in the settings.  MP_FLAG_PATHS is
    ignored by the feature planes, which are those of the primary hits."""

    def __init__(self, scene, camera, settings, threshold: float, floor: float = 0.05, min_samples: int = 16, round_samples: int = 16,
                 planes=("shade", "shade_sq")):
        import torch

        flags = settings.as_struct().flags
        for bit, name in ((_lib.MP_FLAG_CHUNKED_SUM, "MP_FLAG_CHUNKED_SUM"), (_lib.MP_FLAG_WAVEFRONT, "MP_FLAG_WAVEFRONT"),
                          (_lib.MP_FLAG_TRAVERSAL_GROUPS, "MP_FLAG_TRAVERSAL_GROUPS")):
            if flags & bit:
                raise ValueError(f"adaptive sampling does not support {name}")
        if int(min_samples) < 1 or int(round_samples) < 1:
            raise ValueError("min_samples and round_samples are at least 1")
        unknown = set(planes) - set(FrameRenderer.AOV_PLANES)
        if unknown:
            raise ValueError(f"unknown planes: {sorted(unknown)}")
        self.threshold, self.floor = float(threshold), float(floor)
        if self.threshold != self.threshold or not (0.0 < self.floor < float("inf")):
            raise ValueError("threshold must not be NaN, floor must be finite and > 0")
        lib()  # a missing library is an error now, not after the first round
        self.fr = FrameRenderer(scene, camera, settings)
        self.settings, self.device, self.device_id = settings, self.fr.device, self.fr.ctx.device_id
        self.bounds = round_bounds(int(settings.sample_count), int(min_samples), int(round_samples))
        want = {k: (k in planes or k in ("shade", "shade_sq")) for k in FrameRenderer.AOV_PLANES}
        self.planes = self.fr.new_aov_planes(**want)
        self._work = None  # compact work planes, allocated by the first round that needs them
        tiles = self.fr.tiles
        self.n_tiles = len(tiles)
        if self.n_tiles == 0:
            raise ValueError("no tiles")
        self._wh = np.array([[t.width(), t.height()] for t in tiles], np.int32).reshape(-1, 2)
        self._area = self._wh[:, 0].astype(np.int64) * self._wh[:, 1]
        self._d_wh = torch.from_numpy(self._wh).to(self.device)  # u32 [n][2] (int32 tensors carry the bits)
        # the check's two outputs side by side, so that a round reads them back in one copy: open u32[n], then max_err f32[n]
        self._d_check = torch.zeros(2 * self.n_tiles, dtype=torch.int32, device=self.device)
        self._d_open, self._d_err = self._d_check[: self.n_tiles], self._d_check[self.n_tiles:]
        self.samples = np.zeros(self.n_tiles, np.int64)  # k_i: the samples tile i holds
        self.open = self._area.copy()                    # before a tile's first check every pixel of it is open
        self.max_err = np.full(self.n_tiles, np.inf, np.float32)
        self.active = list(range(self.n_tiles))
        self.round = 0
        self.finished = False

    # ---- the three device operations on this sampler's planes -------------------------------------------------------------------
    def _stream(self):
        return _postlib.stream_of(self.device)

    def _upload(self, a):
        """A small host array on the device through pinned memory, asynchronous on the current torch stream.  (A copy from pageable
        memory blocks the calling thread until the stream has drained: a host synchronisation at the head of every compact round
        and in finish().)"""
        import torch

        return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(self.device, non_blocking=True)

    def _move(self, n, src, src_idx, dst, dst_idx):
        check(lib().mpa_move_tiles(self.device_id, int(self.settings.tile_size), n, src.data_ptr(), src.shape[0],
                                   None if src_idx is None else src_idx.data_ptr(), dst.data_ptr(), dst.shape[0],
                                   None if dst_idx is None else dst_idx.data_ptr(), self._stream()))

    def _render(self, planes, tiles_c, n, begin, count):
        """samples [begin, begin + count) of the n tiles of tiles_c into slots 0..n-1 of `planes` (mp_render_aov_pass_device)"""
        fr = self.fr
        st = _lib.SettingsStruct.from_buffer_copy(fr._st)
        st.flags |= _lib.MP_FLAG_ACCUMULATE
        st.pass_begin, st.pass_count = int(begin), int(count)
        pl = _lib.AovPlanesEx(C.sizeof(_lib.AovPlanesEx), *[planes[k].data_ptr() if k in planes else None for k in fr.AOV_PLANES])
        _lib.check(_lib.lib().mp_render_aov_pass_device(fr.ctx.handle, fr.scene.object.handle, C.byref(fr._sampler), C.byref(st), tiles_c,
                                                        n, C.byref(pl), C.byref(fr._extras), self._stream()))

    # ---- the driver ----------------------------------------------------------------------------------------------------------------
    def step(self) -> bool:
        """One round: the next samples of the schedule for every active tile, then (below sample_count) the convergence check.
        Returns False, having done nothing, when no tile is active.  Synchronises with the device once, to read the check's result."""
        import torch

        if not self.active:
            return False
        if self.finished:
            raise RuntimeError("finish() has been called: the planes hold means")
        b0, b1 = self.bounds[self.round], self.bounds[self.round + 1]
        total, n = self.bounds[-1], len(self.active)
        act = np.asarray(self.active, np.int32)
        whole = n == self.n_tiles
        if whole:
            target, tiles_c, d_wh, d_idx = self.planes, self.fr._tiles_c, self._d_wh, None
        else:
            # "ids" is written by the pass that holds sample 0, which is round 0, which is never compact: it stays where it is
            names = [k for k in self.planes if k != "ids"]
            if self._work is None:
                self._work = {k: torch.zeros_like(self.planes[k]) for k in names}
            target = {k: self._work[k] for k in names}
            d_idx = self._upload(act)
            d_wh = self._upload(self._wh[act])
            tiles_c = (_lib.Block * n)(*[self.fr.tiles[i].as_struct() for i in self.active])
            for k in names:
                self._move(n, self.planes[k], d_idx, target[k], None)
        self._render(target, tiles_c, n, b0, b1 - b0)
        checked = b1 < total
        if checked:
            check(lib().mpa_tile_error(self.device_id, int(self.settings.tile_size), n, b1, self.threshold, self.floor,
                                       target["shade"].data_ptr(), target["shade_sq"].data_ptr(), d_wh.data_ptr(),
                                       self._d_open.data_ptr(), self._d_err.data_ptr(), self._stream()))
        if not whole:
            for k in target:
                self._move(n, target[k], None, self.planes[k], d_idx)
        self.samples[act] = b1
        self.round += 1
        if checked:
            got = self._d_check.cpu().numpy()  # the round's synchronisation
            self.open[act] = got[:n]
            self.max_err[act] = got[self.n_tiles:self.n_tiles + n].view(np.float32)
            self.active = [int(i) for i in act[self.open[act] != 0]]
        else:
            self.active = []
        return True

    def finish(self) -> None:
        """Stopped tiles' sums -> means (mpa_finish_tiles on every float plane).  Afterwards FrameRenderer.untile_plane applies to
        the planes as it does to a plain render's."""
        import torch

        if self.finished:
            return
        d_samples = self._upload(self.samples.astype(np.int32))
        for k, p in self.planes.items():
            if p.dtype == torch.float32:
                check(lib().mpa_finish_tiles(self.device_id, int(self.settings.tile_size), self.n_tiles, self.bounds[-1], p.data_ptr(),
                                             d_samples.data_ptr(), self._d_wh.data_ptr(), self._stream()))
        self.finished = True

    def render(self) -> dict:
        """Steps until no tile is active, then finish(); returns the planes."""
        while self.step():
            pass
        self.finish()
        return self.planes

    @property
    def samples_drawn(self) -> int:
        """samples drawn so far: the sum over the tiles of area * k_i"""
        return int(np.sum(self._area * self.samples))

    def sample_map(self) -> np.ndarray:
        """[h, w] int32: the samples each pixel has drawn"""
        w, h = self.settings.resolution
        out = np.zeros((h, w), np.int32)
        for t, k in zip(self.fr.tiles, self.samples):
            out[t.min_y:t.max_y, t.min_x:t.max_x] = k
        return out

    def untile_plane(self, name: str):
        """Image-major [h, w, 4] of a plane (FrameRenderer.untile_plane); the means, once finish() has run."""
        return self.fr.untile_plane(self.planes[name])

    def last_kernels(self) -> list:
        return last_kernels()
