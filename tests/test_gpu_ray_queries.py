"""GPU tests of the bounded closest-hit and occlusion queries (mp_trace_rays_bounded / mp_occluded_rays; definitions and facts in
include/minipath_hip.h "Bounded and occlusion queries").  The oracle has no bounded walk: everything is derived from its unbounded
trace (t* = the unbounded closest-hit distance) through the facts, and from the GPU's own unbounded mp_trace_rays.
  1. tmax NULL / +inf / f32::MAX: the bits of mp_trace_rays in every field;
  2. t* >= b or an unbounded miss: a miss (and NaN / tmax <= 0: a miss);
  3. a bounded hit at t: t* <= t < b (the header's exception, a ray crossing two boxes whose floating-point entry lies past a
     triangle they hold, does not occur on these rays);
  4. b at or above the padded exit of the scene's box: exactly (t* < b ? the unbounded record : miss);
  occluded == (bounded prim != MP_NO_PRIM) for every ray and every bound."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib, scenes
from tests import meshes
from tests.conftest import TEAPOT

pytestmark = pytest.mark.gpu

F = np.float32
FMAX = np.finfo(F).max
NO = 0xFFFFFFFF
MESHES = ["soup_300", "soup_5000", "grid_40", "sphere_24", "flat_plane", "two_clusters", "sliver_fan"]
SCENES = ["teapot", "atrium"] + MESHES + ["sphere", "group", "instances"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return mp.Context(0)


def _quats(rng, n):
    q = rng.standard_normal((n, 4)).astype(F)
    q /= np.sqrt((q.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(F)
    q[0] = (0.0, 0.0, 0.0, 1.0)
    return q.astype(F)


def _camera_rays(oracle, n, seed):
    s = oracle.build_sampler(oracle.teapot_camera(), 256, 256)
    rng = np.random.default_rng(seed)
    o, d = np.zeros((n, 3), F), np.zeros((n, 3), F)
    for i in range(n):
        r = oracle.sample_ray(s, int(rng.integers(0, 256)), int(rng.integers(0, 256)), 77 + i)
        o[i], d[i] = list(r.o), list(r.d)
    return o, d


def _make(name, ctx, oracle):
    """(GPU scene object, oracle trace (o, d) -> t, prim, u, v, inst, rays o, d)"""
    if name == "teapot":
        gpu, orc = mp.TriangleBvh.with_obj(TEAPOT, ctx), oracle.Bvh.from_obj(TEAPOT)
        o1, d1 = meshes.random_rays(12000, 31, *orc.bbox())
        o2, d2 = _camera_rays(oracle, 4000, 5)
        o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
        return gpu, (lambda o, d: (*orc.trace(o, d), np.zeros(o.shape[0], np.uint32))), o, d
    if name == "atrium" or name in MESHES:
        pos, nrm, tex, tri = scenes.atrium(1, 0.05) if name == "atrium" else meshes.make(name)
        gpu, orc = mp.TriangleBvh.build(pos, nrm, tex, tri, ctx), oracle.Bvh.build(pos, nrm, tex, tri)
        bmin, bmax = orc.bbox()
        o, d = meshes.random_rays(16000, 41, bmin, np.maximum(bmax, bmin + 1e-3))
        # and rays aimed at triangle centroids: hits on sparse scenes too
        rng = np.random.default_rng(42)
        c = pos[tri[rng.integers(0, tri.shape[0], 4000)]].mean(axis=1).astype(F)
        d[-4000:] = (c - o[-4000:]).astype(F)
        return gpu, (lambda o, d: (*orc.trace(o, d), np.zeros(o.shape[0], np.uint32))), o, d
    if name == "sphere":
        c, r = (1.0, 2.0, 3.0), 1.5
        gpu = mp.Sphere(c, r, ctx)
        o, d = meshes.random_rays(3000, 43, np.array(c, F) - r, np.array(c, F) + r)

        def trace(o, d):
            n = o.shape[0]
            t, prim = np.full(n, FMAX, F), np.full(n, NO, np.uint32)
            for i in range(n):
                h = oracle.sphere_intersect(c, r, oracle.ray_new(o[i], d[i]))
                if h.hit:
                    t[i], prim[i] = h.t, 0
            return t, prim, np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.uint32)

        return gpu, trace, o, d
    if name == "group":
        rng = np.random.default_rng(19)
        pos, nrm, tex, tri = meshes.make("soup_300")
        teapot, soup, ball = mp.TriangleBvh.with_obj(TEAPOT, ctx), mp.TriangleBvh.build(pos, nrm, tex, tri, ctx), mp.Sphere((0.4, 0, 0), 1.0, ctx)
        o_teapot, o_soup = oracle.Bvh.from_obj(TEAPOT), oracle.Bvh.build(pos, nrm, tex, tri)
        tr = np.array([[0, 0, 0], [7.0, 0.5, -2.0], [-5.5, 2.0, 1.0], [0.0, 5.0, -1.0], [3.0, 4.5, 2.5]], F)
        q = _quats(rng, 5)
        gpu = mp.ObjectGroup([teapot, teapot, soup, ball, soup], tr, rotations=q)
        box = oracle.Bvh.from_obj(TEAPOT)
        box.set_group([box, o_teapot, o_soup, ((0.4, 0.0, 0.0), 1.0), o_soup], tr, rotations=q)
        gpu._keep = (teapot, soup, ball, box, o_teapot, o_soup)
        i = gpu.info()
        o, d = meshes.random_rays(16000, 23, np.array(list(i.bbox_min), F), np.array(list(i.bbox_max), F))
        return gpu, box.trace_inst, o, d
    if name == "instances":
        base = mp.TriangleBvh.with_obj(TEAPOT, ctx)
        tr = np.array([[0, 0, 0], [7.5, 0, -3], [-7.0, 0.5, -6], [0.25, 3.4, -1.0]], F)
        gpu = mp.Instances(base, tr)
        orc = oracle.Bvh.from_obj(TEAPOT)
        orc.set_instances(tr)
        gpu._keep = (orc,)
        i = gpu.info()
        o, d = meshes.random_rays(16000, 4, np.array(list(i.bbox_min), F), np.array(list(i.bbox_max), F))
        return gpu, orc.trace_inst, o, d
    raise KeyError(name)


def _cuda(*a):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def _host(out):
    import torch

    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _box_exit(scene, o, d):
    """slab exit of the scene's box in f64, padded (children are rounded outward by the quantiser): fact 4's level"""
    i = scene.info()
    lo, hi = np.array(list(i.bbox_min), np.float64), np.array(list(i.bbox_max), np.float64)
    dd = d.astype(np.float64)
    dd = dd / np.linalg.norm(dd, axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        a, c = (lo - o) / dd, (hi - o) / dd
    far = np.where(np.isnan(np.maximum(a, c)), np.inf, np.maximum(a, c)).min(axis=1)
    far = np.where(np.isfinite(far), far, 0.0)
    return (np.maximum(far, 0.0) * (1 + 1e-3) + 1e-2 * (1 + np.abs(hi - lo).max())).astype(F)


FULL = ("t", "prim", "u", "v", "point", "normal", "tex", "material", "instance")


@pytest.mark.parametrize("name", SCENES)
def test_unbounded_bound_gives_the_same_bits(ctx, oracle, name):
    """Fact 1: tmax None / +inf / f32::MAX (tensor and Python float) and a NULL d_tmax give mp_trace_rays' bits in every field."""
    import torch

    scene, _, o, d = _make(name, ctx, oracle)
    to, td = _cuda(o, d)
    ref = _host(scene.intersect(to, td, full=True))
    n = o.shape[0]
    for tm in (float("inf"), float(FMAX), torch.full((n,), float("inf"), device="cuda"), torch.full((n,), float(FMAX), device="cuda")):
        got = _host(scene.intersect(to, td, full=True, tmax=tm))
        for k in FULL:
            assert np.array_equal(bits(got[k]), bits(ref[k])), (k, tm if isinstance(tm, float) else "tensor")
        occ = scene.occluded(to, td, tmax=tm).cpu().numpy()
        assert np.array_equal(occ, ref["prim"].view(np.uint32) != NO)
    # d_tmax == NULL through the C ABI
    out = {k: torch.empty_like(torch.from_numpy(ref[k])).cuda() for k in FULL}
    hits = _lib.HitsSoA(*[out[k].data_ptr() for k in FULL])
    oc, dc = to.t().contiguous(), td.t().contiguous()
    _lib.check(_lib.lib().mp_trace_rays_bounded(ctx.handle, scene.handle, *[x.data_ptr() for x in (oc[0], oc[1], oc[2], dc[0], dc[1], dc[2])],
                                                None, n, C.byref(hits), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    got = _host(out)
    for k in FULL:
        assert np.array_equal(bits(got[k]), bits(ref[k])), k
    assert np.array_equal(scene.occluded(to, td).cpu().numpy(), ref["prim"].view(np.uint32) != NO)


def _tmax_rounds(ts, hit, exit_, rng):
    """per-ray bounds: around t* for hits ({t*(1-2^-8), t*, nextafter(t*), t*(1+2^-8), 2 t*}), finite values for misses, then 0 /
    -1 / NaN / positive denormals mixed in, then the fact-4 level"""
    n = ts.shape[0]
    tsf = np.where(hit, ts, F(1)).astype(F)
    around = [tsf * F(1 - 2**-8), tsf, np.nextafter(tsf, F(np.inf)), tsf * F(1 + 2**-8), tsf * F(2)]
    miss_vals = np.exp(rng.uniform(-3, 9, n)).astype(F)
    rounds = [np.where(hit, a, miss_vals).astype(F) for a in around]
    mixed = np.where(hit, np.stack(around)[rng.integers(0, 5, n), np.arange(n)], miss_vals).astype(F)
    special = np.array([0.0, -1.0, np.nan, np.float32(1e-45), np.float32(3e-39), -0.0, -np.inf], F)
    pick = rng.random(n) < 0.3
    mixed[pick] = special[rng.integers(0, special.shape[0], int(pick.sum()))]
    rounds.append(mixed)
    rounds.append(exit_)
    rounds.append(exit_ * F(4))
    return rounds


@pytest.mark.parametrize("name", SCENES)
def test_bounded_and_occluded_against_the_oracle(ctx, oracle, name):
    """Facts 2, 3 and 4 against the oracle's unbounded trace, and occluded == bounded hit, on every bound."""
    scene, trace, o, d = _make(name, ctx, oracle)
    ts, prim, u, v, inst = trace(o, d)
    hit = prim != NO
    assert hit.mean() > 0.02 or name == "flat_plane"
    to, td = _cuda(o, d)
    unb = _host(scene.intersect(to, td, full=True))
    assert np.array_equal(unb["prim"].view(np.uint32), prim) and np.array_equal(bits(unb["t"]), bits(ts))  # the oracle's t*
    exit_ = _box_exit(scene, o, d)
    rng = np.random.default_rng(3)
    n4 = nb = 0
    for tm in _tmax_rounds(ts, hit, exit_, rng):
        (tt,) = _cuda(tm)
        got = _host(scene.intersect(to, td, full=True, tmax=tt))
        occ = scene.occluded(to, td, tmax=tt).cpu().numpy()
        gp = got["prim"].view(np.uint32)
        ghit = gp != NO
        b = np.where(tm > 0, np.minimum(tm, FMAX), F(0))  # NaN compares false: b = 0
        # occluded == bounded hit, exactly
        assert np.array_equal(occ, ghit), f"{int((occ != ghit).sum())} rays"
        # fact 2 and the effective bound: a miss where t* >= b, the unbounded walk misses, or tmax is NaN / <= 0
        must_miss = ~hit | ~(ts < b)
        assert not ghit[must_miss].any(), f"{int(ghit[must_miss].sum())} hits beyond the bound"
        miss = ~ghit
        assert np.all(got["t"][miss] == FMAX) and not got["u"][miss].any() and not got["v"][miss].any()
        assert not got["instance"][miss].any() and not got["point"][miss].any()
        # fact 3
        assert np.all(got["t"][ghit] < b[ghit]) and np.all(ts[ghit] <= got["t"][ghit])
        nb += int(ghit.sum())
        # fact 4: bounds at or above the padded box exit
        f4 = (tm >= exit_) & (b > 0)
        keep = f4 & hit & (ts < b)
        for k in FULL:
            assert np.array_equal(bits(got[k][keep]), bits(unb[k][keep])), k
        assert not ghit[f4 & ~keep].any()
        n4 += int(keep.sum())
    assert nb > 0 and (n4 > 100 or name == "flat_plane")


@pytest.mark.parametrize("n", [0, 1, 63, 65, 1000, 4099])
def test_edge_sizes(ctx, oracle, n):
    """n = 0 is a no-op; n = 1, 65 and sizes that are not a multiple of 64 give the rows of a large call."""
    import torch

    scene, _, o, d = _make("teapot", ctx, oracle)
    o, d = o[:4099], d[:4099]
    tm = np.linspace(0.5, 30.0, o.shape[0]).astype(F)
    to, td, tt = _cuda(o, d, tm)
    big = _host(scene.intersect(to, td, full=True, tmax=tt))
    bocc = scene.occluded(to, td, tmax=tt).cpu().numpy()
    got = _host(scene.intersect(to[:n].contiguous(), td[:n].contiguous(), full=True, tmax=tt[:n].contiguous()))
    occ = scene.occluded(to[:n].contiguous(), td[:n].contiguous(), tmax=tt[:n].contiguous()).cpu().numpy()
    assert occ.dtype == np.bool_ and occ.shape == (n,)
    for k in FULL:
        assert got[k].shape[0] == n and np.array_equal(bits(got[k]), bits(big[k][:n])), k
    assert np.array_equal(occ, bocc[:n])
    torch.cuda.synchronize()


def test_errors(ctx):
    """The checks of mp_trace_rays: a scene of another context, NULL ray / output arrays, a host-only BVH."""
    import torch

    other = mp.Context(0)
    scene = mp.TriangleBvh.with_obj(TEAPOT, other)
    o = torch.zeros((4, 3), device="cuda")
    d = torch.ones((4, 3), device="cuda")
    L = _lib.lib()
    hits = _lib.HitsSoA()
    x = o.data_ptr()
    assert L.mp_trace_rays_bounded(ctx.handle, scene.handle, *([x] * 6), None, 4, C.byref(hits), None) == 1
    assert L.mp_occluded_rays(ctx.handle, scene.handle, *([x] * 6), None, 4, x, None) == 1
    assert b"another context" in L.mp_last_error()
    own = mp.TriangleBvh.with_obj(TEAPOT, ctx)
    assert L.mp_trace_rays_bounded(ctx.handle, own.handle, x, None, x, x, x, x, None, 4, C.byref(hits), None) == 1
    assert L.mp_occluded_rays(ctx.handle, own.handle, x, x, x, x, x, None, None, 4, x, None) == 1
    assert L.mp_occluded_rays(ctx.handle, own.handle, *([x] * 6), None, 4, None, None) == 1
    assert L.mp_trace_rays_bounded(ctx.handle, own.handle, *([x] * 6), None, 4, None, None) == 1
    host = mp.TriangleBvh.with_obj(TEAPOT)
    with pytest.raises(_lib.MinipathError):
        host.occluded(o, d, tmax=1.0)
    with pytest.raises(_lib.MinipathError):
        host.intersect(o, d, tmax=1.0)
    assert L.mp_occluded_rays(ctx.handle, host.handle, *([x] * 6), None, 4, x, None) == 1  # no device arrays
    # the scene of the other context works with that context
    assert not own.occluded(o, d, tmax=0.0).cpu().numpy().any()
    assert scene.occluded(o, d).shape == (4,)
    torch.cuda.synchronize()
