#!/usr/bin/env python3
"""The mask cache's unit bounds B from the camera (mask_cache_begin_unit, minipath_amd/csrc/mask_cache.h): a numpy restatement, f32
operation by f32 operation, and the counts that choose its margin.

As a module: corner_header(sampler, jitter_scale, x0, x1, y0, y1, margin) is the header the device function writes (the tests compare
them bit for bit); pass_rule() is mask_cache_begin_pass's widening.  As a program it walks every pass of some work units of the
metric's frame (2x2 pixels x 16 samples per pass, rays from the oracle) through the wide tree once, and replays the cache's
bound-keeping for each rule -- today's (first pass + MP_MCACHE_PAD) and the corner bounds at several margins -- counting per rule:
bound sets per unit, passes that escape B, and the triangle tests / child boxes that B proves missed per pass.

usage: analytic_bounds.py [atrium|teapot] [units] [passes per unit]
"""
import os
import sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

F = np.float32
COORD_CAP = F(2.0 ** 30)
FLT_MAX = np.finfo(F).max
PAD = F(0.25)  # MP_MCACHE_PAD


def jitter_scale():
    """UniformFloat::new_inclusive(-0.5, 0.5).scale"""
    max_rand = F(1.0) - np.finfo(F).eps
    scale = F(1.0) / max_rand
    while F(scale * max_rand) + F(-0.5) > F(0.5):
        scale = np.nextafter(scale, F(0))
    return F(scale)


def camera_rays(s, film_u, film_v, x1, x2):
    """camera_film + camera_lens_ray + ray_new: s = the sampler's 15 floats, the rest f32 arrays of one shape -> o, d, inv [..., 3]"""
    s = np.asarray(s, F)
    center, up, right, foo = s[0:3], s[3:6], s[6:9], s[9:12]
    pixel_scale, lens_radius, lens_weight = s[12], s[13], s[14]
    film_u, film_v, x1, x2 = (np.asarray(a, F) for a in (film_u, film_v, x1, x2))
    fv, fu = film_v * pixel_scale, film_u * pixel_scale
    a, b = lens_radius * x1, lens_radius * x2
    o, d = [], []
    for k in range(3):
        f = (foo[k] + up[k] * fv) - right[k] * fu
        l = right[k] * a + up[k] * b
        o.append(center[k] + l)
        d.append(l * lens_weight - f)
    n = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        u = [(c / n).astype(F) for c in d]
        inv = [np.where(c == 0, F(np.inf), F(1) / c).astype(F) for c in u]
    return np.stack(o, -1).astype(F), np.stack(u, -1), np.stack(inv, -1)


def ray_ok(o, d, inv):
    """mask_cache_ray_ok"""
    return (np.abs(o) <= COORD_CAP).all(-1) & (np.abs(inv) <= FLT_MAX).all(-1) & (np.abs(d) <= F(2)).all(-1)


def widen(lo, hi, frac):
    """the widening of a bounds group [3, 3] (origins, inverse directions, directions) by frac of its extent, with the guards of
    mask_cache_begin_pass"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    with np.errstate(over="ignore", invalid="ignore"):
        pad = (hi - lo) * F(frac)
        wlo, whi = (lo - pad).astype(F), (hi + pad).astype(F)
    for w, b in ((wlo, lo), (whi, hi)):
        bad = ((w[1] < 0) != (b[1] < 0)) | (w[1] == 0) | ~(np.abs(w[1]) < np.inf)
        w[1] = np.where(bad, b[1], w[1])
    for g, cap in ((0, F(2) * COORD_CAP), (2, F(2))):
        wlo[g] = np.maximum(wlo[g], -cap); whi[g] = np.minimum(whi[g], cap)
    return wlo, whi


def corner_header(s, jscale, x0, x1, y0, y1, margin):
    """-> (state, lo[3, 3], hi[3, 3]): state = sign pattern | 0x100 and the widened corner bounds (groups: origins, inverse
    directions, directions), or (0xFFFFFFFF, None, None) where mask_cache_begin_unit declines"""
    c = np.arange(16)
    hi_off = F(jscale) + F(-0.5)
    fu = np.where(c & 1, F(x1) + hi_off, F(x0) + F(-0.5)).astype(F)
    fv = np.where(c & 2, F(y1) + hi_off, F(y0) + F(-0.5)).astype(F)
    o, d, inv = camera_rays(s, fu, fv, np.where(c & 4, F(1), F(-1)).astype(F), np.where(c & 8, F(1), F(-1)).astype(F))
    neg = inv < 0
    if not ray_ok(o, d, inv).all() or not (neg.all(0) | ~neg.any(0)).all():
        return 0xFFFFFFFF, None, None
    oct_ = int(neg[0, 0]) | int(neg[0, 1]) << 1 | int(neg[0, 2]) << 2
    lo, hi = widen(np.stack([o.min(0), inv.min(0), d.min(0)]), np.stack([o.max(0), inv.max(0), d.max(0)]), margin)
    return oct_ | 0x100, lo, hi


def header_words(state, lo, hi):
    """the 19 header dwords as mask_cache.h lays them out (hdr_lo / kHdrState)"""
    w = np.zeros(19, np.uint32)
    w[12] = state
    if lo is not None:
        for g, base in ((0, 0), (1, 6), (2, 13)):
            w[base:base + 3] = lo[g].view(np.uint32); w[base + 3:base + 6] = hi[g].view(np.uint32)
    return w


class Cache:
    """the bound-keeping of one unit under one rule: margin None = today's (no B before the first pass)"""

    def __init__(self, margin, s, jscale, block):
        self.sets = self.escapes = 0
        self.state, self.lo, self.hi = (0xFFFFFFFF, None, None) if margin is None else corner_header(s, jscale, *block, margin)
        if self.state != 0xFFFFFFFF:
            self.sets = 1

    def begin_pass(self, o, d, inv):
        """mask_cache_begin_pass for a pass of one sign pattern whose rays all pass ray_ok"""
        neg = inv[0] < 0
        oct_ = (int(neg[0]) | int(neg[1]) << 1 | int(neg[2]) << 2) | 0x100
        v = np.stack([o, inv, d])  # [3 groups, rays, 3]
        same = self.state == oct_
        if same and ((v >= self.lo[:, None, :]) & (v <= self.hi[:, None, :])).all():
            return
        if self.state != 0xFFFFFFFF:
            self.escapes += 1
        lo, hi = v.min(1), v.max(1)
        if same:
            lo, hi = np.minimum(lo, self.lo), np.maximum(hi, self.hi)
        self.lo, self.hi = widen(lo, hi, PAD)
        self.state = oct_
        self.sets += 1


def box_reject(boxes, lo, hi, neg):
    """bounds_may_hit, negated: [k] bool, no ray inside B passes the child box"""
    omin, omax, imin, imax = lo[0], hi[0], lo[1], hi[1]
    y, z = boxes[:, :3] - omax[None], boxes[:, 3:] - omin[None]
    lsrc, hsrc = np.where(neg[None], z, y), np.where(neg[None], y, z)
    L = np.minimum(lsrc * imin[None], lsrc * imax[None]); U = np.maximum(hsrc * imin[None], hsrc * imax[None])
    t1 = np.maximum(np.maximum(L[:, 0], 0), np.maximum(L[:, 1], L[:, 2])); t2 = np.minimum(U[:, 0], np.minimum(U[:, 1], U[:, 2]))
    return t1 > t2


def main():
    import ctypes as C
    from sim_collapse import RefTree, load, build_device, slab
    import sim_tri_reject as st
    from minipath_amd import scenes
    from oracle import pyoracle as po
    scene = sys.argv[1] if len(sys.argv) > 1 else "atrium"
    units = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    passes = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    w, h, spp = 1920, 1080, 16 * passes
    if scene == "teapot":
        cam = po.teapot_camera()
    else:
        cam = po.Camera(); po.lib().mpo_camera_default(C.byref(cam))
        eye, at, fnum = scenes.ATRIUM_VIEW
        po.lib().mpo_camera_look_at(C.byref(cam), po.vec3(*eye), po.vec3(*at), po.vec3(0, 1, 0)); cam.f_number = fnum
    smp = po.build_sampler(cam, w, h)
    s, js = smp.as_array(), jitter_scale()
    ref = RefTree(*load(scene, 1.0))
    nodes, root, _ = build_device(ref, "area", 8)
    rng = np.random.default_rng(11)
    rules = [("first pass + 1/4 (today)", None)] + [(f"corners + 1/{int(1 / m)}", m) for m in (1 / 64, 1 / 32, 1 / 16, 1 / 8)] + [("corners + 0", 0.0)]
    tot = {name: dict(sets=0, esc=0, tri_rej=0, box_rej=0) for name, _ in rules}
    n_pass = tris = boxes_tested = pushed = hit_some = declined = generic = 0
    for _ in range(units):
        x0, y0 = 2 * int(rng.integers(0, w // 2)), 2 * int(rng.integers(0, h // 2))
        caches = {name: Cache(m, s, js, (x0, x0 + 1, y0, y0 + 1)) for name, m in rules}
        declined += caches[rules[1][0]].state == 0xFFFFFFFF
        for p in range(passes):
            o = np.zeros((64, 3), F); d = np.zeros((64, 3), F); inv = np.zeros((64, 3), F)
            for l in range(64):
                px, py = x0 + (l // 16) % 2, y0 + (l // 16) // 2
                r = po.sample_ray(smp, px, py, po.lib().mpo_sample_key(0x5EED, w, spp, px, py, p * 16 + l % 16))
                o[l] = list(r.o); d[l] = list(r.d); inv[l] = list(r.inv)
            neg = inv < 0
            if not ray_ok(o, d, inv).all() or not (neg.all(0) | ~neg.any(0)).all():
                generic += 1  # a generic walk: no cache
                continue
            n_pass += 1
            for c in caches.values():
                c.begin_pass(o, d, inv)
            best = np.full(64, FLT_MAX, F)
            stack = [(root, np.ones(64, bool), None)]
            while stack:
                link, mask, box = stack.pop()
                if box is not None:
                    t1, _ = slab(box[None, :], o, inv, best); mask = mask & ~(t1[:, 0] > best)
                if not mask.any():
                    continue
                if link >= 0:
                    bxs, links = nodes[link]
                    t1, t2 = slab(bxs, o, inv, best)
                    ok = (t1 <= t2) & mask[:, None]
                    some = ok.any(0)
                    boxes_tested += len(links); pushed += int(some.sum())
                    for name, c in caches.items():
                        rej = box_reject(bxs, c.lo, c.hi, neg[0])
                        assert not (rej & some).any(), "a child some ray passes was rejected"
                        tot[name]["box_rej"] += int(rej.sum())
                    for cc in range(len(links)):
                        if some[cc]:
                            stack.append((int(links[cc]), ok[:, cc].copy(), bxs[cc]))
                else:
                    v0, e1, e2 = ref.leaf[-1 - link]
                    valid, t = st.mt_valid(v0, e1, e2, o, d)
                    valid &= mask[:, None]
                    some = valid.any(0)
                    tris += v0.shape[0]; hit_some += int(some.sum())
                    for name, c in caches.items():
                        rej = st.interval_reject(v0, e1, e2, c.lo[0], c.hi[0], c.lo[2], c.hi[2])
                        assert not (rej & some).any(), "a triangle some ray hits was rejected"
                        tot[name]["tri_rej"] += int(rej.sum())
                    best = np.minimum(best, np.where(valid, t, np.inf).min(axis=1).astype(F))
        for name, c in caches.items():
            tot[name]["sets"] += c.sets; tot[name]["esc"] += c.escapes
    print(f"{scene}: {units} units x {passes} passes of 2x2 pixels x 16 samples; {n_pass} cached passes, {generic} generic; corner bounds declined for {declined} units")
    print(f"per pass: child boxes tested {boxes_tested / n_pass:.1f}, pushed {pushed / n_pass:.1f}; triangle tests {tris / n_pass:.1f}, hit by some ray {hit_some / n_pass:.2f}")
    print(f"{'rule':28s} {'sets/unit':>9s} {'escaping passes':>16s} {'tris rejected/pass':>19s} {'boxes rejected/pass':>20s}")
    for name, _ in rules:
        t = tot[name]
        print(f"{name:28s} {t['sets'] / units:9.3f} {100.0 * t['esc'] / n_pass:15.2f}% {t['tri_rej'] / n_pass:12.1f} ({100.0 * t['tri_rej'] / tris:4.1f}%) "
              f"{t['box_rej'] / n_pass:12.1f} ({100.0 * t['box_rej'] / (boxes_tested - pushed):4.1f}% of unpushed)")


if __name__ == "__main__":
    main()
