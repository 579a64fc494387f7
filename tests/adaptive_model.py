"""Expectation model of adaptive sampling (include/minipath_adaptive.h, minipath_amd/adaptive.py): the three device operations
restated in numpy float32, one rounding per operation as the header writes them, and the driver over tests/aov_pass_model.Frame --
state_after(k) at every check, the stop decisions, and the final planes (a stopped tile is state_after(k_i) * (1 / k_i), a tile
that ran to the budget is planes()).  The GPU tests compare bit patterns against it with zero differences."""
import functools

import numpy as np

from tests import aov_pass_model
from tests.aov_pass_model import FLOAT_PLANES, PLANES, F, bits  # noqa: F401

U = np.uint32


def round_bounds(sample_count, min_samples, round_samples):
    """0, min_samples, min_samples + round_samples, ..., clipped to sample_count"""
    b = [0, min(min_samples, sample_count)]
    while b[-1] < sample_count:
        b.append(min(b[-1] + round_samples, sample_count))
    return b


def _mx(a, b):
    """the header's max(a, b): a > b ? a : b (b for a NaN a, +0 for max(-0, 0))"""
    return np.where(a > b, a, F(b)).astype(F)


def pixel_error(s, q, k, floor):
    """e of the header for arrays of moments s, q after k samples"""
    s, q = np.asarray(s, F), np.asarray(q, F)
    with np.errstate(all="ignore"):
        r = F(1) / F(k)
        m = (s * r).astype(F)
        m2 = (q * r).astype(F)
        d = (m2 - (m * m).astype(F)).astype(F)
        v = (_mx(d, 0) * r).astype(F)
        return (np.sqrt(v).astype(F) / (m + F(floor)).astype(F)).astype(F)


def _key(e):
    """the order -inf < ... < -0 < +0 < ... < +inf on non-NaN floats, as u32 keys"""
    b = np.asarray(e, F).view(U)
    return np.where(b & U(0x80000000), ~b, b | U(0x80000000)).astype(U)


def _unkey(k):
    k = U(k)
    if k == 0:
        return F(0)
    return np.array([k ^ U(0x80000000) if k & U(0x80000000) else ~k], U).view(F)[0]


def tile_error(shade, shade_sq, wh, k, threshold, floor):
    """(open u32[n], max_err f32[n]) of tile-major state planes [n, ts, ts, 4] with extents wh[n][2]"""
    n, ts = shade.shape[0], shade.shape[1]
    opened, err = np.zeros(n, U), np.zeros(n, F)
    for i in range(n):
        w, h = min(int(wh[i][0]), ts), min(int(wh[i][1]), ts)
        e = pixel_error(shade[i, :h, :w, 0], shade_sq[i, :h, :w, 0], k, floor)
        with np.errstate(invalid="ignore"):
            opened[i] = np.sum(~(e <= F(threshold)))
        e = np.where(np.isnan(e), F(np.inf), e).astype(F)
        err[i] = _unkey(_key(e).max()) if e.size else F(0)
    return opened, err


def move_tiles(src, src_slot, dst, dst_slot, n):
    """dst (changed in place) after mpa_move_tiles; None index arrays are the identity, out-of-range indices are skipped"""
    for j in range(n):
        a = j if src_slot is None else int(src_slot[j])
        b = j if dst_slot is None else int(dst_slot[j])
        if a < src.shape[0] and b < dst.shape[0]:
            dst[b] = src[a]
    return dst


def finish_tiles(plane, samples, wh, sample_count):
    """a copy of the float plane after mpa_finish_tiles"""
    out = plane.copy()
    ts = plane.shape[1]
    for i, k in enumerate(samples):
        k = int(k)
        if 0 < k < sample_count:
            w, h = min(int(wh[i][0]), ts), min(int(wh[i][1]), ts)
            with np.errstate(all="ignore"):
                out[i, :h, :w] = (plane[i, :h, :w] * (F(1) / F(k))).astype(F)
    return out


def tile_major(img, tiles, ts):
    """image-major [h, w, 4] -> tile-major [n, ts, ts, 4]; what a slot does not own is 0"""
    out = np.zeros((len(tiles), ts, ts, 4), img.dtype)
    for i, t in enumerate(tiles):
        out[i, : t.max_y - t.min_y, : t.max_x - t.min_x] = img[t.min_y:t.max_y, t.min_x:t.max_x]
    return out


class Expected:
    """The driver over a Frame: `tiles` is the renderer's full tile list (ScreenBlocks).  samples[i] = k_i; checks = [(k, state
    planes tile-major, active tile indices at the check, open, max_err)] per check; planes = the finished tile-major planes (owned
    pixels; the rest 0); states[k] = the tile-major state after k samples, for every boundary below sample_count."""

    def __init__(self, frame, tiles, ts, threshold, floor, min_samples, round_samples):
        spp = frame.spp
        self.tiles, self.ts, self.bounds = tiles, ts, round_bounds(spp, min_samples, round_samples)
        n = len(tiles)
        self.wh = np.array([[t.max_x - t.min_x, t.max_y - t.min_y] for t in tiles], U)
        self.samples = np.zeros(n, np.int64)
        self.stop_order = {}  # k -> tile indices that stopped at the check after k samples
        self.states, self.checks = {}, []
        done = {k: tile_major(v, tiles, ts) for k, v in frame.planes().items()}
        self.planes = {k: v.copy() for k, v in done.items()}
        active = list(range(n))
        for b in self.bounds[1:]:
            if not active:
                break
            self.samples[active] = b
            if b == spp:
                active = []
                break
            st = {k: tile_major(v, tiles, ts) for k, v in frame.state_after(b).items()}
            self.states[b] = st
            opened, err = tile_error(st["shade"][active], st["shade_sq"][active], self.wh[active], b, threshold, floor)
            self.checks.append((b, list(active), opened, err))
            stopped = [i for i, o in zip(active, opened) if o == 0]
            self.stop_order[b] = stopped
            for name in FLOAT_PLANES:
                fin = finish_tiles(st[name], np.full(n, b), self.wh, spp)
                for i in stopped:
                    self.planes[name][i] = fin[i]
            active = [i for i, o in zip(active, opened) if o != 0]
        self.area = self.wh[:, 0].astype(np.int64) * self.wh[:, 1]
        self.samples_drawn = int(np.sum(self.area * self.samples))

    def sample_map(self, width, height):
        out = np.zeros((height, width), np.int32)
        for t, k in zip(self.tiles, self.samples):
            out[t.min_y:t.max_y, t.min_x:t.max_x] = k
        return out


# the end-to-end case of tests/test_gpu_adaptive.py and its non-vacuity condition in tests/test_adaptive_cpu.py
CASE = dict(res=(72, 40), ts=16, spp=64, seed=2, floor=0.05, threshold=0.2, min_samples=16, round_samples=16)


@functools.lru_cache(maxsize=None)
def teapot_case():
    """(Frame, Expected, tiles) of CASE on the teapot under teapot_view, computed once per process from the oracle alone"""
    import minipath_amd as mp
    from oracle import pyoracle as po
    from tests.conftest import TEAPOT

    w, h = CASE["res"]
    b = po.Bvh.from_obj(TEAPOT)
    smp = po.sampler_from_array(mp.Camera.teapot_view().build_sampler(CASE["res"]).as_array())
    frame = aov_pass_model.Frame(po, b.intersect, smp, w, CASE["spp"], CASE["seed"], (0, 0, w, h))
    tiles = mp.tile_ordering(mp.ScreenBlock(0, 0, w, h), CASE["ts"])
    exp = Expected(frame, tiles, CASE["ts"], CASE["threshold"], CASE["floor"], CASE["min_samples"], CASE["round_samples"])
    return frame, exp, tiles
