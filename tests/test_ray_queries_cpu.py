"""CPU tests of the bounded closest-hit and occlusion queries (mp_trace_rays_bounded / mp_occluded_rays, include/minipath_hip.h
"Bounded and occlusion queries"): the C ABI's signatures and argument checks without a GPU, and the facts the header states,
checked on a numpy model of the reference's walk (ray_bvh_intersection.rs:26-62) with best.t starting at a bound, run on both
device trees.  The model checks the ARGUMENT (what a walk with a starting bound does on these trees), not the kernel: the GPU
tests (tests/test_gpu_ray_queries.py) compare the kernels with the oracle."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib
from tests.conftest import TEAPOT
from tests.test_device_tree_cpu import _host, _leaf_tris, _slots, _walk

F = np.float32
FMAX = np.finfo(F).max


def test_signatures():
    L = _lib.lib()
    for name, n_ptr_args in (("mp_trace_rays_bounded", 7), ("mp_occluded_rays", 7)):
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        a = fn.argtypes
        assert len(a) == 12
        assert a[:2] == [C.c_void_p, C.c_void_p]
        assert a[2:2 + n_ptr_args] == [C.c_void_p] * n_ptr_args  # ox, oy, oz, dx, dy, dz, tmax
        assert a[9] is C.c_uint64 and a[11] is C.c_void_p
    assert L.mp_trace_rays_bounded.argtypes[10] is C.POINTER(_lib.HitsSoA)
    assert L.mp_occluded_rays.argtypes[10] is C.c_void_p


def test_null_context_or_scene_is_invalid():
    L = _lib.lib()
    host = mp.TriangleBvh.with_obj(TEAPOT)
    hits = _lib.HitsSoA()
    occ = (C.c_uint8 * 1)()
    x = (C.c_float * 1)()
    for ctx, scene in ((None, host.handle), (None, None)):
        assert L.mp_trace_rays_bounded(ctx, scene, x, x, x, x, x, x, None, 1, C.byref(hits), None) == 1  # MP_ERR_INVALID
        assert L.mp_occluded_rays(ctx, scene, x, x, x, x, x, x, None, 1, occ, None) == 1
        assert L.mp_last_error()
    # n == 0 passes the ray checks but not the NULL context / scene check
    assert L.mp_occluded_rays(None, None, None, None, None, None, None, None, None, 0, None, None) == 1


def test_host_only_bvh_raises():
    import torch

    host = mp.TriangleBvh.with_obj(TEAPOT)
    o = torch.zeros((4, 3))
    d = torch.ones((4, 3))
    with pytest.raises(_lib.MinipathError):
        host.occluded(o, d, tmax=1.0)
    with pytest.raises(_lib.MinipathError):
        host.intersect(o, d, tmax=1.0)
    with pytest.raises(_lib.MinipathError):
        mp.Sphere((0, 0, 0), 1.0).occluded(o, d)


# ---- the model walk with a starting bound -----------------------------------------------------------------------------
def _slab(boxes, o, inv, best):
    """aabb.rs:254-284 on f32 boxes: (t1, t1 <= t2) with t2 limited by best"""
    with np.errstate(invalid="ignore"):
        a = (boxes[:, :3] - o) * inv
        c = (boxes[:, 3:] - o) * inv
    a = np.where(np.isnan(a), -np.inf, a)
    c = np.where(np.isnan(c), np.inf, c)
    lo, hi = np.minimum(a, c), np.maximum(a, c)
    e1 = np.maximum(np.maximum(lo[:, 0], 0), np.maximum(lo[:, 1], lo[:, 2])).astype(F)
    e2 = np.minimum(np.minimum(hi[:, 0], best), np.minimum(hi[:, 1], hi[:, 2])).astype(F)
    return e1, e1 <= e2


def _walk_bounded(nodes, root, tris_of, o, d, b, any_hit=False):
    """ray_bvh_intersection.rs:26-62 with best.t = b (:34-37): pop test t1 > best (:40), slab limit best (:149-162), leaf test
    t <= best (:125), accept t < best (:59).  any_hit: stop at the first leaf that accepts.  Returns (leaf sequence, t or None)."""
    with np.errstate(divide="ignore"):
        inv = np.where(d == 0, F(np.inf), F(1) / d).astype(F)
    best, hit = F(b), False
    stack = [(root, F(-np.inf))]
    seq = []
    while stack:
        link, t1 = stack.pop()
        if t1 > best:
            continue
        if link & 63:
            seq.append(link)
            ts = tris_of(link, o, d)
            ts = ts[ts <= best]
            if ts.size and ts.min() < best:
                best, hit = F(ts.min()), True
                if any_hit:
                    break
            continue
        sl = _slots(nodes, link >> 6)
        e1, ok = _slab(np.array([bx for bx, _ in sl], F), o, inv, best)
        for k, (_, l) in enumerate(sl):
            if ok[k]:
                stack.append((l, e1[k]))
    return seq, (best if hit else None)


def _max_entry(nodes, root, o, d):
    """largest slab entry t1 over every box of the tree the ray enters (t1 <= exit, no best.t limit): a bound at or above it
    culls nothing (fact 4)"""
    with np.errstate(divide="ignore"):
        inv = np.where(d == 0, F(np.inf), F(1) / d).astype(F)
    m, stack = F(0), [root]
    while stack:
        link = stack.pop()
        if link & 63:
            continue
        sl = _slots(nodes, link >> 6)
        e1, ok = _slab(np.array([bx for bx, _ in sl], F), o, inv, FMAX)
        for k, (_, l) in enumerate(sl):
            if ok[k]:
                m = max(m, e1[k])
                stack.append(l)
    return m


def _tris(host, lit):
    inner, pk = _leaf_tris(host)
    leaf_box = {}
    for n in range(lit.shape[0]):
        for box, l in _slots(lit, n):
            if l & 63:
                leaf_box[l] = box
    cache = {}

    def tris_of(link, o, d):
        """t of every triangle of the leaf, +inf where the test fails (numpy Moeller-Trumbore as in test_device_tree_cpu)"""
        if link not in cache:
            first, nreal = link >> 6, link & 63
            box = leaf_box[link]
            mn, size = box[:3], (box[3:] - box[:3]).astype(F)
            npk = (nreal + 7) // 8
            rel = pk[first:first + npk].astype(F) * (F(1) / F(65535))
            p = (np.float64(size)[None, None, :, None] * np.float64(rel) + np.float64(mn)[None, None, :, None]).astype(F)
            p = p.transpose(0, 3, 1, 2).reshape(npk * 8, 3, 3)[:nreal]
            cache[link] = (p[:, 0], (p[:, 1] - p[:, 0]).astype(F), (p[:, 2] - p[:, 0]).astype(F))
        v0, e1, e2 = cache[link]
        h = np.cross(d, e2)
        det = (e1 * h).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            invd = 1.0 / det
            s = o - v0
            u = invd * (s * h).sum(-1)
            q = np.cross(s, e1)
            v = invd * (d * q).sum(-1)
            t = invd * (e2 * q).sum(-1)
            ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0)
        return np.where(ok, t, np.inf).astype(F)

    return tris_of


def _bounds(ts, mx):
    """the GPU test's bound set for one ray: around t* for a hit, finite values for a miss, f32::MAX, the fact-4 level"""
    if ts is None:
        return [F(0.5), F(3.0), F(50.0), F(1e6), FMAX, mx]
    return [F(ts * F(1 - 2**-8)), F(ts), np.nextafter(F(ts), F(np.inf)), F(ts * F(1 + 2**-8)), F(2 * ts), FMAX, mx,
            np.nextafter(mx, F(np.inf))]


MODEL_SCENES = ["atrium:0.05", "atrium:0.1", "soup_5000", "two_clusters"]


def _model_rays(lit, bmin, bmax):
    """the 120 rays of the model tests: around and inside the box, zero direction components, origins on box planes, rays aimed
    at leaf boxes"""
    rng = np.random.default_rng(9)
    ext = bmax - bmin
    n = 120
    o = (bmin - 0.2 * ext + rng.random((n, 3)) * ext * 1.4).astype(F)
    d = rng.standard_normal((n, 3)).astype(F)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:6, 0] = 0.0  # zero components: the literal tree's NaN patches
    planes = lit[:, :, :6].view(F).reshape(-1, 6)
    planes = planes[np.isfinite(planes).all(1) & (lit[:, :, 6].reshape(-1) != 0xFFFFFFF8)]
    for k in range(6, 30):  # origins on box planes: entry distances 0 and ties
        bx = planes[rng.integers(0, planes.shape[0])]
        o[k] = bx[:3] if k % 2 else bx[3:]
    leaves = np.array([bx for n_ in range(lit.shape[0]) for bx, l in _slots(lit, n_) if l & 63], F)
    for k in range(60, n):  # aimed at leaf boxes: hits on sparse scenes too
        bx = leaves[rng.integers(0, leaves.shape[0])]
        tgt = bx[:3] + (bx[3:] - bx[:3]) * rng.random(3).astype(F)
        d[k] = (tgt - o[k]) / np.linalg.norm(tgt - o[k])
    return o, d


@pytest.mark.parametrize("name", MODEL_SCENES)
def test_bounded_model_walk_facts(name):
    """Facts 1-5 of include/minipath_hip.h and occluded == bounded hit, on the model walk (see the module docstring)."""
    host = _host(name)
    wide, wroot, _, _ = host.device_tree()
    lit, lroot, _, _ = host.device_tree(literal=True)
    info = host.info()
    bmin, bmax = np.array(list(info.bbox_min), F), np.array(list(info.bbox_max), F)
    tris_of = _tris(host, lit)
    unb = lambda l: F(np.inf) if l.size == 0 else l.min()  # noqa: E731

    def tris_min(link, o, d):  # test_device_tree_cpu._walk's interface: the leaf's smallest valid t
        return unb(tris_of(link, o, d))

    o, d = _model_rays(lit, bmin, bmax)
    n = o.shape[0]
    checked = {"hit": 0, "miss": 0, "band": 0}
    for k in range(n):
        seq_u, tu, _ = _walk(lit, lroot, tris_min, o[k], d[k])
        ts = None if tu == FMAX else F(tu)  # (the model's _walk keeps best = f32::MAX for a miss)
        mx = _max_entry(lit, lroot, o[k], d[k])
        for b in _bounds(ts, mx):
            sw, tw = _walk_bounded(wide, wroot, tris_of, o[k], d[k], b)
            sl, tl = _walk_bounded(lit, lroot, tris_of, o[k], d[k], b)
            # fact 5: same leaves, same result on both trees
            assert sw == sl and tw == tl, (k, b)
            # occluded == bounded hit, on both trees
            for nodes, root in ((wide, wroot), (lit, lroot)):
                _, ta = _walk_bounded(nodes, root, tris_of, o[k], d[k], b, any_hit=True)
                assert (ta is not None) == (tl is not None), (k, b)
            if b == FMAX:  # fact 1
                assert sl == seq_u and (tl if tl is not None else FMAX) == tu
            if ts is None or ts >= b:  # fact 2
                assert tl is None, (k, b, ts)
                checked["miss"] += 1
            if tl is not None:  # fact 3
                assert tl < b and ts is not None and ts <= tl, (k, b, ts, tl)
                checked["hit"] += 1
            if b >= mx:  # fact 4: exact
                assert tl == (ts if ts is not None and ts < b else None), (k, b)
                if ts is not None and ts < b:
                    assert sl == seq_u
                checked["band"] += 1
    assert checked["hit"] > 10 and checked["miss"] > 10 and checked["band"] > 10
