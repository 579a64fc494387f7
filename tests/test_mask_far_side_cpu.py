"""The far-side terms of the unit triangle masks (mask_cache.h, tri_may_hit: u.lo > 1 or v.lo > 1 rejects), checked on the CPU through
the model, tools/sim_tri_reject.py's interval_reject, against its per-ray test mt_valid (triangle.rs:183-217 in f32).

Condition A, everywhere: a triangle the rule rejects is accepted by no ray inside its box.
Condition B, so that A says something: at least 1 000 cases that ONLY the new terms reject, and at least 100 cases in which a ray
that computes u == 1 & v == 0, u == 0 & v == 1 or u + v == 1 exactly is accepted -- and the triangle therefore kept.

Cases:
* real units: boxes around the bounds of units of the teapot and of the stand-in at detail 0.5 (the unit's corner bounds scaled about
  their centre), against the scene's triangles; rays = the box's 64 corners, random points inside and the unit's own rays;
* a far family: boxes whose footprint on the triangle's plane lies beyond the edge u = 1 (or v = 1) while the other coordinate
  straddles zero -- what `u.lo + v.lo > 1` cannot reject;
* an exact family: dyadic coordinates, so that the aimed ray's u and v are exact -- aimed at v1, at v2, at points of the edge v1 v2,
  one ulp inside and one ulp outside that edge, with +-0 direction components, with direction bounds that reach into the triangle's
  plane (the determinant interval touches zero) and with a vertex at the 2^30 coordinate cap; the box is the ray alone or extends
  from it, so the ray is one of its corners.
The last two are the cases of the GPU probe (mask_probe.hip, far_kernel), drawn here with numpy."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _st():
    if os.path.join(ROOT, "tools") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sim_tri_reject as st

    return st


def _corners(lo, hi):
    """[64, m, 6]: the corners of m boxes (lo, hi: [m, 6])"""
    bits = ((np.arange(64)[:, None] >> np.arange(6)[None, :]) & 1).astype(bool)
    return np.where(bits[:, None, :], hi[None], lo[None]).astype(F)


def _interior(rng, lo, hi, n):
    t = rng.random((n,) + lo.shape).astype(F)
    return np.clip((lo[None] + (hi - lo)[None] * t).astype(F), lo[None], hi[None]).astype(F)


def _check_cases(v0, e1, e2, lo, hi, rays):
    """m cases, each a triangle and a box of its own (lo, hi: [m, 6] = origin, direction), rays [R, m, 6] inside the boxes:
    (rejected, rejected by the far-side terms only, hit by some ray, accepted per ray [R, m])"""
    st = _st()
    assert np.all((rays >= lo[None]) & (rays <= hi[None])), "a ray outside its box"
    new = st.interval_reject(v0, e1, e2, lo[:, 0:3].T, hi[:, 0:3].T, lo[:, 3:6].T, hi[:, 3:6].T)
    old = st.interval_reject(v0, e1, e2, lo[:, 0:3].T, hi[:, 0:3].T, lo[:, 3:6].T, hi[:, 3:6].T, far=False)
    assert not (old & ~new).any(), "the far-side terms only add rejections"
    # (mt_valid takes component k of ray i as [i, k]: with [R, 3, m] arrays every case gets its own rays, and the result is [R, 1, m])
    ok, _ = st.mt_valid(v0, e1, e2, rays[..., 0:3].transpose(0, 2, 1), rays[..., 3:6].transpose(0, 2, 1))
    ok = ok[:, 0, :]
    return new, new & ~old, ok.any(axis=0), ok


def _to_world(rng, p, llo, lhi, x):
    """local frame -> world axes by a permutation and sign flips of the axes, per case: vertices p [m, 3, 3], box [m, 6], ray x [m, 6]"""
    m = llo.shape[0]
    perms = np.array([[0, 1, 2], [0, 2, 1], [1, 2, 0], [1, 0, 2], [2, 0, 1], [2, 1, 0]])[rng.integers(0, 6, m)]
    sg = np.where(rng.random((m, 3)) < 0.5, F(-1), F(1)).astype(F)
    rows = np.arange(m)[:, None]
    q = p[np.arange(m)[:, None, None], np.arange(3)[None, :, None], perms[:, None, :]] * sg[:, None, :]
    def six(a):
        return np.concatenate([a[rows, perms] * sg, a[rows, 3 + perms] * sg], axis=1).astype(F)
    a, b = six(llo), six(lhi)
    return q.astype(F), np.minimum(a, b), np.maximum(a, b), six(x)


def far_family(rng, m):
    S = F(2.0) ** rng.integers(-8, 21, m).astype(F)
    sx, sy = (S * (F(0.5) + rng.random(m).astype(F))).astype(F), (S * (F(0.5) + rng.random(m).astype(F))).astype(F)
    tilt = np.where(rng.random(m) < 0.25, F(0), F(0.05)) * S
    p0 = (F(4) * S[:, None] * (2 * rng.random((m, 3)) - 1)).astype(F)
    r = lambda: (tilt * (2 * rng.random(m) - 1)).astype(F)  # noqa: E731
    E1, E2 = np.stack([sx, r(), r()], 1), np.stack([r(), sy, r()], 1)
    p = np.stack([p0, (p0 + E1).astype(F), (p0 + E2).astype(F)], 1)
    a0 = (1 + F(2.0) ** -rng.integers(0, 16, m).astype(F) * (F(0.25) + rng.random(m).astype(F))).astype(F)
    a1 = (a0 + 2 * rng.random(m) * rng.random(m)).astype(F)
    b0 = (1 - a0 - (2 * rng.random(m) - 0.5)).astype(F)
    b1 = np.maximum(b0, np.where(rng.random(m) < 0.25, -0.25, 0.5) * rng.random(m)).astype(F)
    swap = rng.random(m) < 0.5
    a0, b0, a1, b1 = np.where(swap, b0, a0), np.where(swap, a0, b0), np.where(swap, b1, a1), np.where(swap, a1, b1)
    H = (S * F(2.0) ** rng.integers(2, 7, m).astype(F)).astype(F)
    am, bm = F(0.5) * (a0 + a1), F(0.5) * (b0 + b1)
    wz = np.where(rng.random(m) < 0.5, 0, H * F(2.0 ** -6) * rng.random(m)).astype(F)
    wd = np.where(rng.random(m) < 0.25, 0, F(2.0) ** -rng.integers(10, 22, m).astype(F)).astype(F)
    by_origin = rng.random(m) < 0.5
    wo = np.where(rng.random(m) < 0.5, 0, S * F(2.0 ** -8) * rng.random(m)).astype(F)
    llo, lhi = np.zeros((m, 6), F), np.zeros((m, 6), F)
    llo[:, 0] = np.where(by_origin, p0[:, 0] + a0 * sx, p0[:, 0] + am * sx - wo); lhi[:, 0] = np.where(by_origin, p0[:, 0] + a1 * sx, p0[:, 0] + am * sx + wo)
    llo[:, 1] = np.where(by_origin, p0[:, 1] + b0 * sy, p0[:, 1] + bm * sy - wo); lhi[:, 1] = np.where(by_origin, p0[:, 1] + b1 * sy, p0[:, 1] + bm * sy + wo)
    llo[:, 2] = p0[:, 2] + H; lhi[:, 2] = p0[:, 2] + H + wz
    llo[:, 3] = np.where(by_origin, -wd, (a0 - am) * sx / H); lhi[:, 3] = np.where(by_origin, wd, (a1 - am) * sx / H)
    llo[:, 4] = np.where(by_origin, -wd, (b0 - bm) * sy / H); lhi[:, 4] = np.where(by_origin, wd, (b1 - bm) * sy / H)
    llo[:, 5] = -1; lhi[:, 5] = -1 + wd
    lhi = np.maximum(llo, lhi)
    return _to_world(rng, p, llo, lhi, llo)[:3]


def exact_family(rng, m):
    """-> vertices, box, the aimed ray, and whether that ray lies exactly on the far boundary (u + v == 1 with u, v >= 0)"""
    cap, plane = rng.random(m) < 0.125, rng.random(m) < 0.125
    q = np.where(cap, F(2.0 ** 20), F(2.0) ** rng.integers(-20, 16, m).astype(F)).astype(F)
    sx, sy = (q * F(2.0) ** rng.integers(4, 9, m).astype(F)).astype(F), (q * F(2.0) ** rng.integers(4, 9, m).astype(F)).astype(F)
    p0 = (q[:, None] * rng.integers(-512, 513, (m, 3)).astype(F)).astype(F)
    p0[:, 0] = np.where(cap, F(2.0 ** 30) - sx, p0[:, 0]); p0[:, 1] = np.where(cap, F(-2.0 ** 30), p0[:, 1])
    p1, p2 = p0.copy(), p0.copy()
    p1[:, 0] = p0[:, 0] + sx; p2[:, 1] = p0[:, 1] + sy
    place = rng.integers(0, 8, m)  # 0, 1: v1; 2, 3: v2; 4, 7: on the edge; 5: one ulp inside; 6: one ulp outside
    a = np.where(place < 2, F(1), np.where(place < 4, F(0), rng.integers(1, 16, m).astype(F) * F(0.0625))).astype(F)
    x = np.zeros((m, 6), F)
    x[:, 0] = p0[:, 0] + a * sx; x[:, 1] = p0[:, 1] + (1 - a) * sy; x[:, 2] = p0[:, 2] + q * rng.integers(1, 4097, m).astype(F)
    # every coordinate so far is exact: the aimed point has u = a and v = 1 - a
    assert np.all((np.float64(x[:, 0]) - np.float64(p0[:, 0])) / np.float64(sx) == np.float64(a))
    assert np.all((np.float64(x[:, 1]) - np.float64(p0[:, 1])) / np.float64(sy) == np.float64(1) - np.float64(a))
    x[:, 3] = np.where(rng.random(m) < 0.5, F(-0.0), F(0.0)); x[:, 4] = np.where(rng.random(m) < 0.5, F(-0.0), F(0.0)); x[:, 5] = -1
    k = np.where(rng.random(m) < 0.5, 0, 1)
    rows = np.arange(m)
    hair = np.where(place == 5, F(-np.inf), F(np.inf)).astype(F)  # towards the triangle is down in x and in y
    moved = np.nextafter(x[rows, k], hair)
    x[rows, k] = np.where((place == 5) | (place == 6), moved, x[rows, k])
    side = rng.integers(0, 8, (m, 6))  # 0..2: the value alone; 3..5: upwards; 6, 7: downwards
    w = np.concatenate([q[:, None] * F(2.0) ** rng.integers(-2, 10, (m, 3)).astype(F), F(2.0) ** rng.integers(-20, -2, (m, 3)).astype(F)], 1).astype(F)
    llo = np.where(side >= 6, x - w, x).astype(F)
    lhi = np.where((side >= 3) & (side < 6), x + w, x).astype(F)
    llo[:, 5] = np.where(plane, F(-1), llo[:, 5]); lhi[:, 5] = np.where(plane, F(0), lhi[:, 5])
    p = np.stack([p0, p1, p2], 1)
    on_boundary = ~((place == 5) | (place == 6))
    return _to_world(rng, p, llo, lhi, x) + (on_boundary,)


def _family_rays(rng, lo, hi, extra=None):
    rays = [_corners(lo, hi), _interior(rng, lo, hi, 32)]
    if extra is not None:
        rays.append(extra[None])
    return np.concatenate(rays, 0)


@functools.lru_cache(maxsize=None)
def family_counts():
    rng = np.random.default_rng(0xFA5)
    m1, m2 = 6000, 3000
    p, lo, hi = far_family(rng, m1)
    v0, e1, e2 = p[:, 0], (p[:, 1] - p[:, 0]).astype(F), (p[:, 2] - p[:, 0]).astype(F)
    rej, only_new, some, _ = _check_cases(v0, e1, e2, lo, hi, _family_rays(rng, lo, hi))
    out = {"far": (int(rej.sum()), int(only_new.sum()), int(some.sum()), int((rej & some).sum()))}
    p, lo, hi, x, on_b = exact_family(rng, m2)
    v0, e1, e2 = p[:, 0], (p[:, 1] - p[:, 0]).astype(F), (p[:, 2] - p[:, 0]).astype(F)
    rays = _family_rays(rng, lo, hi, x)
    assert np.any((rays[:64] == x[None]).all(-1), axis=0).all(), "the aimed ray is a corner of its box"
    rej, only_new, some, ok = _check_cases(v0, e1, e2, lo, hi, rays)
    aimed_ok = ok[-1]
    # an aimed ray exactly on the far boundary is accepted (u, v, t exact: v1, v2 and the edge belong to the triangle) ...
    assert aimed_ok[on_b].all(), "a ray exactly on the far boundary is accepted by the per-ray test"
    out["exact"] = (int(rej.sum()), int(only_new.sum()), int(some.sum()), int((rej & some).sum()))
    out["boundary_kept"] = int((on_b & aimed_ok & ~rej).sum())
    out["boundary_dropped"] = int((on_b & aimed_ok & rej).sum())
    out["hair_outside_rejected"] = int(rej[~on_b].sum())
    return out


def test_constructed_far_and_exact_cases():
    c = family_counts()
    print(c)
    for fam in ("far", "exact"):
        rej, only_new, some, wrong = c[fam]
        assert wrong == 0, f"{fam}: {wrong} rejected triangles are accepted by a ray inside their box"  # condition A
        assert some > 0 and rej > 0
    assert c["boundary_dropped"] == 0
    # condition B
    assert c["far"][1] + c["exact"][1] >= 1000, "too few cases that only the far-side terms reject"
    assert c["boundary_kept"] >= 100, "too few exact-boundary cases that are accepted and kept"
    assert c["hair_outside_rejected"] > 0, "no box one ulp beyond the far edge was rejected"


def _scene_triangles(host, rng, max_leaves):
    from tests import graft_model as gm

    tris = gm.LeafTriangles(host)
    links = sorted(tris.box)
    if len(links) > max_leaves:
        links = [links[i] for i in sorted(rng.choice(len(links), max_leaves, replace=False))]
    o1, d1 = np.zeros((1, 3), F), np.ones((1, 3), F)
    for link in links:
        tris.nearest(link, o1, d1)
    return tuple(np.concatenate([tris.cache[link][k] for link in links]) for k in range(3))


def _unit_boxes(oracle, rng, host, cam, res, spp, seed, n_units):
    """boxes around real units: (lo, hi, rays) with lo, hi [6] and rays [R, 6] inside"""
    from tests import unit_list_model as ul

    sarr = cam.build_sampler(res).as_array()
    out = []
    units_x, units_y = res[0] // 2, res[1] // 2
    tries = 0
    while len(out) < 2 * n_units and tries < 8 * n_units:
        tries += 1
        ux, uy = int(rng.integers(units_x // 4, 3 * units_x // 4)), int(rng.integers(units_y // 4, 3 * units_y // 4))
        up = ul.unit_passes(oracle, sarr, res, spp, seed, uy * units_x + ux, ul.shipped_margin())
        if up is None:
            continue
        (hlo, hhi, _), passes = up
        ulo, uhi = np.concatenate([hlo[0], hlo[2]]).astype(F), np.concatenate([hhi[0], hhi[2]]).astype(F)
        own = np.concatenate([np.concatenate([o, d], 1) for o, d, _ in passes]).astype(F)
        for scale in (F(1.0), F(rng.choice([0.5, 2.0, 4.0]))):
            ctr, half = F(0.5) * (ulo + uhi), F(0.5) * (uhi - ulo) * scale
            lo, hi = (ctr - half).astype(F), (ctr + half).astype(F)
            if scale <= 1:  # never wider than the unit's own bounds there
                lo, hi = np.maximum(lo, ulo), np.minimum(hi, uhi)
            rays = np.concatenate([_corners(lo[None], hi[None])[:, 0], _interior(rng, lo[None], hi[None], 64)[:, 0],
                                   own[((own >= lo) & (own <= hi)).all(1)]])
            out.append((lo, hi, rays))
    assert len(out) >= n_units
    return out


def _scene_counts(oracle, rng, host, cam, res, seed):
    st = _st()
    v0, e1, e2 = _scene_triangles(host, rng, 600)
    rejected = only_new = hit = wrong = 0
    for lo, hi, rays in _unit_boxes(oracle, rng, host, cam, res, 64, seed, 4):
        new = st.interval_reject(v0, e1, e2, lo[0:3], hi[0:3], lo[3:6], hi[3:6])
        old = st.interval_reject(v0, e1, e2, lo[0:3], hi[0:3], lo[3:6], hi[3:6], far=False)
        assert not (old & ~new).any()
        ok, _ = st.mt_valid(v0, e1, e2, rays[:, 0:3], rays[:, 3:6])
        some = ok.any(axis=0)
        rejected += int(new.sum()); only_new += int((new & ~old).sum()); hit += int(some.sum()); wrong += int((new & some).sum())
    return rejected, only_new, hit, wrong


def test_real_units_teapot(oracle):
    import minipath_amd as mp
    from tests.conftest import TEAPOT

    rng = np.random.default_rng(31)
    c = _scene_counts(oracle, rng, mp.TriangleBvh.with_obj(TEAPOT), mp.Camera.teapot_view(), (96, 64), 21)
    print("teapot: rejected %d, by the far-side terms only %d, hit by some ray %d, rejected although hit %d" % c)
    assert c[3] == 0
    assert c[0] > 0 and c[1] > 0 and c[2] > 0


def test_real_units_stand_in(oracle):
    from minipath_amd import scenes
    from tests import graft_model as gm

    rng = np.random.default_rng(37)
    c = _scene_counts(oracle, rng, gm.evict_host(), scenes.atrium_camera(), gm.EVICT_RES, gm.EVICT_SEED)
    print("stand-in: rejected %d, by the far-side terms only %d, hit by some ray %d, rejected although hit %d" % c)
    assert c[3] == 0
    assert c[0] > 0 and c[1] > 0 and c[2] > 0
