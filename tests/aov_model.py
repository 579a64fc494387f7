"""Expectation model of the first-hit feature planes (mp_render_aov_device, include/minipath_hip.h), in plain numpy over the
oracle: for every pixel and sample  mpo_sample_key -> mpo_sample_ray -> the oracle's intersect (full Hit),  every channel summed
with np.float32 adds in sample order from +0.0 (misses add +0.0) and scaled by np.float32(1) / np.float32(spp); ids = the record
of sample 0.  The albedo is the header's rule restated in np.float32: mp_material.albedo of Hit.material, albedo2 on the odd
cells of a checker material (cell = floor(tx * scale) + floor(ty * scale); odd = (cell * 0.5 - floor(cell * 0.5)) != 0, so a NaN
cell is odd).  One ctypes call per ray: size the cases at tens of thousands of rays."""
import ctypes as C

import numpy as np

F = np.float32
NO_PRIM = 0xFFFFFFFF
DEFAULT_TABLE = [(0.75, 0.0)]  # a scene whose table was never set


def albedo_of(rec, hit):
    """Reflectance at `hit` under the material records `rec` (oracle.material_records): np.float32 [3]."""
    m = rec[int(hit.material)]
    alb = m[0:3]
    if m[9:10].view(np.uint32)[0] == 1:  # MP_TEXTURE_CHECKER
        with np.errstate(invalid="ignore"):
            scale = F(m[10])
            cell = F(np.floor(F(F(hit.tex[0]) * scale)) + np.floor(F(F(hit.tex[1]) * scale)))
            half = F(cell * F(0.5))
            if F(half - np.floor(half)) != F(0.0):
                alb = m[6:9]
    return alb


def planes(oracle, intersect, sampler, width, spp, seed, block, table=None):
    """The four planes of the pixels of block = (x0, y0, x1, y1): dict of [h, w, 4] arrays ("shade", "normal", "albedo" float32,
    "ids" uint32).  intersect(ray) -> oracle.Hit."""
    L = oracle.lib()
    rec = oracle.material_records(DEFAULT_TABLE if table is None else table)
    x0, y0, x1, y1 = block
    h, w = y1 - y0, x1 - x0
    out = {k: np.zeros((h, w, 4), F) for k in ("shade", "normal", "albedo")}
    out["ids"] = np.zeros((h, w, 4), np.uint32)
    inv = F(1) / F(spp)
    for y in range(y0, y1):
        for x in range(x0, x1):
            vals = np.zeros((spp, 8), F)  # shade, n.x, n.y, n.z, t, r, g, b ; a miss keeps +0.0
            hits = 0
            for s in range(spp):
                key = L.mpo_sample_key(C.c_uint64(seed), width, spp, x, y, s)
                r = oracle.sample_ray(sampler, x, y, key)
                hr = intersect(r)
                if s == 0:
                    out["ids"][y - y0, x - x0] = (hr.prim & 0xFFFFFFFF, hr.instance, hr.material, 1) if hr.hit else (NO_PRIM, 0, 0, 0)
                if not hr.hit:
                    continue
                hits += 1
                d, n = [F(v) for v in r.d], [F(v) for v in hr.normal]
                vals[s, 0] = np.abs(F(F(F(d[0] * n[0]) + F(d[1] * n[1])) + F(d[2] * n[2])))  # worker.rs:60
                vals[s, 1:4] = n
                vals[s, 4] = F(hr.t)
                vals[s, 5:8] = albedo_of(rec, hr)
            acc = np.zeros(8, F)
            for s in range(spp):  # strictly in sample order (np.sum is pairwise)
                acc = (acc + vals[s]).astype(F)
            m = (acc * inv).astype(F)
            a = F(F(hits) * inv)
            out["shade"][y - y0, x - x0] = (m[0], m[0], m[0], a)
            out["normal"][y - y0, x - x0] = (m[1], m[2], m[3], m[4])
            out["albedo"][y - y0, x - x0] = (m[5], m[6], m[7], a)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
