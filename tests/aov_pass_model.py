"""Expectation model of the feature planes in passes (mp_render_aov_pass_device, include/minipath_hip.h): tests/aov_model.py's
rules with the two further planes and the state between passes.  Per pixel and sample  mpo_sample_key -> mpo_sample_ray -> the
oracle's intersect (full Hit); twelve float channels -- aov_model's eight, then "position" = Hit.point (the oracle's point_at(t)
of the world ray) and "shade_sq" = F(c * c), ONE np.float32 product of the model's own f32 shade value c -- summed with np.float32
adds in sample order from +0.0 (misses add +0.0).  state_after(k): the unscaled sums and hit counts after the first k samples, as
the planes hold them between passes; planes(): state_after(spp) scaled by np.float32(1) / np.float32(spp).  One ctypes call per
ray: size the cases at a few thousand rays."""
import ctypes as C

import numpy as np

from tests import aov_model
from tests.aov_model import DEFAULT_TABLE, NO_PRIM, F, albedo_of, bits  # noqa: F401  (bits: for the tests)

FLOAT_PLANES = ("shade", "normal", "albedo", "position", "shade_sq")
PLANES = ("shade", "normal", "albedo", "ids", "position", "shade_sq")


def shade_of(d, n):
    """worker.rs:60 in np.float32: |d . n|, products and sums rounded one by one, left to right"""
    d, n = [F(v) for v in d], [F(v) for v in n]
    return np.abs(F(F(F(d[0] * n[0]) + F(d[1] * n[1])) + F(d[2] * n[2])))


def sample_values(c, normal, t, albedo, point):
    """the twelve values one hit adds: shade, n.x, n.y, n.z, t, r, g, b, p.x, p.y, p.z, F(c * c)"""
    v = np.zeros(12, F)
    v[0] = c
    v[1:4] = normal
    v[4] = F(t)
    v[5:8] = albedo
    v[8:11] = point
    v[11] = F(F(c) * F(c))
    return v


def ordered_sum(vals):
    """rows of vals added in order from +0.0 with np.float32 adds (np.sum is pairwise)"""
    acc = np.zeros(vals.shape[1], F)
    for row in vals:
        acc = (acc + row).astype(F)
    return acc


def _pack(acc, hits, scale):
    """the five float planes' pixels from twelve sums and the hit count, every value * scale"""
    m = (acc * scale).astype(F)
    a = F(F(hits) * scale)
    return {"shade": (m[0], m[0], m[0], a), "normal": (m[1], m[2], m[3], m[4]), "albedo": (m[5], m[6], m[7], a),
            "position": (m[8], m[9], m[10], a), "shade_sq": (m[11], m[11], m[11], a)}


class Frame:
    """The per-sample values of the pixels of block = (x0, y0, x1, y1), computed once; planes() and state_after(k) sum them."""

    def __init__(self, oracle, intersect, sampler, width, spp, seed, block, table=None):
        L = oracle.lib()
        rec = oracle.material_records(DEFAULT_TABLE if table is None else table)
        x0, y0, x1, y1 = block
        self.spp, self.h, self.w = spp, y1 - y0, x1 - x0
        self.vals = np.zeros((self.h, self.w, spp, 12), F)  # a miss keeps +0.0
        self.hit = np.zeros((self.h, self.w, spp), bool)
        self.ids = np.zeros((self.h, self.w, 4), np.uint32)
        for y in range(y0, y1):
            for x in range(x0, x1):
                for s in range(spp):
                    key = L.mpo_sample_key(C.c_uint64(seed), width, spp, x, y, s)
                    r = oracle.sample_ray(sampler, x, y, key)
                    hr = intersect(r)
                    if s == 0:
                        self.ids[y - y0, x - x0] = (hr.prim & 0xFFFFFFFF, hr.instance, hr.material, 1) if hr.hit else (NO_PRIM, 0, 0, 0)
                    if not hr.hit:
                        continue
                    self.hit[y - y0, x - x0, s] = True
                    self.vals[y - y0, x - x0, s] = sample_values(shade_of(r.d, hr.normal), [F(v) for v in hr.normal], hr.t, albedo_of(rec, hr),
                                                                 [F(v) for v in hr.point])

    def _sums(self, k, scale):
        out = {name: np.zeros((self.h, self.w, 4), F) for name in FLOAT_PLANES}
        out["ids"] = self.ids.copy()
        for y in range(self.h):
            for x in range(self.w):
                px = _pack(ordered_sum(self.vals[y, x, :k]), int(self.hit[y, x, :k].sum()), scale)
                for name in FLOAT_PLANES:
                    out[name][y, x] = px[name]
        return out

    def state_after(self, k):
        """what the planes hold after passes over samples [0, k), 0 < k < spp: {sum, sum, sum, hits}, "normal" {sum n, sum t}; "ids"
        is sample 0's record from the first pass on"""
        assert 0 < k <= self.spp
        return self._sums(k, F(1))

    def planes(self):
        """the finished planes: sums over all samples * (np.float32(1) / np.float32(spp))"""
        return self._sums(self.spp, F(1) / F(self.spp))


def planes(oracle, intersect, sampler, width, spp, seed, block, table=None):
    """the six planes, as aov_model.planes gives the four"""
    return Frame(oracle, intersect, sampler, width, spp, seed, block, table).planes()


assert aov_model.F is F
