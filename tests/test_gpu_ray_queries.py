"""GPU tests of the bounded closest-hit and occlusion queries (mp_trace_rays_bounded / mp_occluded_rays; definitions and facts in
include/minipath_hip.h "Bounded and occlusion queries").  The kernels are compared bit for bit, in every mp_hits_soa field, with the
oracle's W(b) (mpo_trace_rays_bounded) and with its early-exit walk (mpo_occluded_rays), which tests/test_ray_queries_oracle_cpu.py
pins on the CPU -- on random and camera rays, on the band rays of the wall scene, on secondary rays started on surfaces, and on
launches whose grid-stride loop takes more than two steps.  Beside that the facts stay asserted as they were, from the oracle's
unbounded trace (t* = the unbounded closest-hit distance) and the GPU's own unbounded mp_trace_rays:
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
from minipath_amd import _lib
from tests import dispatch_cases as dc
from tests import plan_probe as pp
from tests import ray_query_scenes as rq
from tests.conftest import TEAPOT
from tests.ray_query_scenes import FMAX, FULL, NO, F, bits

pytestmark = pytest.mark.gpu

MESHES, SCENES = rq.MESHES, rq.SCENES


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return mp.Context(0)


def _make(name, ctx, oracle):
    """(GPU scene object, oracle trace (o, d) -> t, prim, u, v, inst, rays o, d); the scenes are tests/ray_query_scenes.py's"""
    gpu, orc, o, d = rq.make(name, ctx, oracle)
    gpu._oracle = orc
    return gpu, orc.trace, o, d


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
    -1 / NaN / positive denormals mixed in, then the fact-4 level, then t* + 2 and + 4 ulp"""
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
    for ulps in (2, 4):
        rounds.append(np.where(hit, _ulps_up(tsf, ulps), miss_vals).astype(F))
    return rounds


def _ulps_up(x, k):
    for _ in range(k):
        x = np.nextafter(x, F(np.inf))
    return x


def _obj(scene):
    """the OBJ template argument of the scene's ray kernels"""
    return "true" if isinstance(scene, (mp.ObjectGroup, mp.Instances)) else "false"


def _assert_exact(ctx, scene, orc, o, d, tm, to=None, td=None):
    """Both queries against the oracle's walks, bit for bit in every field, and the kernels that ran.  Returns (records, occluded)."""
    if to is None:
        to, td = _cuda(o, d)
    (tt,) = _cuda(tm)
    want, wocc = orc.trace_bounded(o, d, tm), orc.occluded(o, d, tm)
    got = _host(scene.intersect(to, td, full=True, tmax=tt))
    assert ctx.last_kernels() == [f"query_rays_kernel<{_obj(scene)}, kBounded>"]
    occ = scene.occluded(to, td, tmax=tt).cpu().numpy()
    assert ctx.last_kernels() == [f"query_rays_kernel<{_obj(scene)}, kAnyHit>"]
    for k in FULL:
        bad = (bits(got[k]) != bits(want[k])).reshape(o.shape[0], -1).any(axis=1)
        assert not bad.any(), f"{k}: {int(bad.sum())} rays, first {int(np.flatnonzero(bad)[0])}"
    assert np.array_equal(occ, wocc), f"{int((occ != wocc).sum())} rays"
    return got, occ


@pytest.mark.parametrize("name", SCENES)
def test_bounded_and_occluded_against_the_oracle(ctx, oracle, name):
    """Every field of the bounded query and the occlusion query against the oracle's W(b) and early-exit walk, bit for bit, on
    every bound; beside them facts 2, 3 and 4 against the oracle's unbounded trace, and occluded == bounded hit."""
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
        got, occ = _assert_exact(ctx, scene, scene._oracle, o, d, tm, to, td)
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


def _mixed_bounds(ts, hit, rng):
    """one bound per ray: around t* for hits ({t*(1-2^-8), t*, t* + 1, 2 and 4 ulp, t*(1+2^-8), 2 t*}), finite values for misses,
    and the values that are not walked (0, -0, -1, NaN, -inf) and positive denormals on three rays in ten"""
    n = ts.shape[0]
    tsf = np.where(hit, ts, F(1)).astype(F)
    around = [tsf * F(1 - 2**-8), tsf, _ulps_up(tsf, 1), _ulps_up(tsf, 2), _ulps_up(tsf, 4), tsf * F(1 + 2**-8), tsf * F(2)]
    tm = np.where(hit, np.stack(around)[rng.integers(0, len(around), n), np.arange(n)], np.exp(rng.uniform(-3, 9, n))).astype(F)
    special = np.array([0.0, -1.0, np.nan, np.float32(1e-45), np.float32(3e-39), -0.0, -np.inf], F)
    pick = rng.random(n) < 0.3
    tm[pick] = special[rng.integers(0, special.shape[0], int(pick.sum()))]
    return tm


@pytest.mark.parametrize("name", ["walls", "wall_group"])
def test_band_rays(ctx, oracle, name):
    """The band fixture (tests/ray_query_scenes.py; 79 band rays, tests/test_ray_queries_oracle_cpu.py::test_band_fixture): rays
    on which W(nextafter(t*)) is not what the facts derive from the unbounded trace, among 4 000 ordinary rays of the wall scene,
    through both queries -- the scene on its own and as a member of a two-member rotated group.  Bit-equal to the oracle at
    t* + 0, 1, 2 and 4 ulp, t*(1 +- 2^-8), 2 t* and a mixed round with the special values."""
    scene, _, o, d = _make(name, ctx, oracle)
    orc = scene._oracle
    band, unb, _ = rq.band_mask(orc, o, d)
    assert band.sum() >= 32, int(band.sum())
    hit = unb["prim"] != NO
    ts = np.where(hit, unb["t"], F(1)).astype(F)
    to, td = _cuda(o, d)
    got, occ = _assert_exact(ctx, scene, orc, o, d, _ulps_up(ts, 1), to, td)
    # what makes them band rays, seen on the GPU: not the unbounded record although t* < b
    differs = np.zeros(o.shape[0], bool)
    for k in FULL:
        differs |= (bits(got[k]) != bits(unb[k])).reshape(o.shape[0], -1).any(axis=1)
    assert np.array_equal(differs & hit, band)
    rounds = [ts, _ulps_up(ts, 2), _ulps_up(ts, 4), ts * F(1 - 2**-8), ts * F(1 + 2**-8), ts * F(2), np.full(o.shape[0], FMAX, F),
              _mixed_bounds(unb["t"], hit, np.random.default_rng(8))]
    for tm in rounds:
        _assert_exact(ctx, scene, orc, o, d, tm.astype(F), to, td)


@pytest.mark.parametrize("name", list(rq.SECONDARY))
def test_secondary_rays(ctx, oracle, name):
    """Rays that start ON a surface, as the documented callers send them: from the hit points of about 8 000 primary rays (the
    oracle's records), offset 1e-4 along the normal towards the incoming ray -- inside many nested boxes with slab entry 0.
    Shadow rays to a point light (un-normalised, tmax = dist (1 - 1e-4)) and random bounce rays (tmax = 2 and 0.05): records and
    occlusion bit-equal to the oracle; between 5 % and 95 % of every set is occluded, so none is vacuous.
    Occluded shares (shadow, tmax 2, tmax 0.05): teapot 46 / 53 / 51 %, grid_40 50 / 57 / 51 %, atrium 21 / 57 / 51 %, walls
    80 / 64 / 50 %, group 67 / 53 / 49 %."""
    scene, _, o, d = _make(name, ctx, oracle)
    orc = scene._oracle
    for key, (so, sd, tm) in rq.secondary_rays(orc, *rq.primary_rays(name, orc, o, d), rq.SECONDARY[name], 5).items():
        assert so.shape[0] > 1000
        _, occ = _assert_exact(ctx, scene, orc, so, sd, tm)
        print(f"{name} {key}: {so.shape[0]} rays, {occ.mean():.3f} occluded")
        assert 0.05 < occ.mean() < 0.95, (key, occ.mean())


BASE = 4099  # shares no factor with 64: every chunk of the tiled set sees another alignment of the base rays


@pytest.mark.parametrize("api", ["trace", "bounded", "occluded"])
@pytest.mark.parametrize("name", ["teapot", "instances"])
def test_more_than_two_sweeps(ctx, oracle, name, api):
    """The grid-stride loop of trace_rays_kernel and query_rays_kernel<OBJ, MODE> (OBJ = false: teapot, true: instances) beyond
    its first step: plan_ray_query caps the grid at cu_count * 8 blocks of 4 waves of 64 rays, and n = 2 * grid * 256 + 4099 + 37
    rays (1 052 712 with grid 2048 at 256 CUs) make every wave take a second chunk and some a third -- a fresh kernarg view, and
    the LDS queue and stack of the chunk before.  The rays are 4 099 base rays with oracle records and mixed bounds, tiled on
    the device: row i of every output is the record of base ray i % 4099."""
    import torch

    scene, _, o, d = _make(name, ctx, oracle)
    orc = scene._oracle
    o, d = np.ascontiguousarray(o[-BASE:]), np.ascontiguousarray(d[-BASE:])
    unb = orc.trace_bounded(o, d)
    hit = unb["prim"] != NO
    assert 0.1 < hit.mean() < 0.9
    tm = _mixed_bounds(unb["t"], hit, np.random.default_rng(12))
    want = unb if api == "trace" else orc.trace_bounded(o, d, tm)
    wocc = orc.occluded(o, d, tm)
    assert 0.05 < wocc.mean() < 0.95 and np.isnan(tm).any() and (tm == 0).any()
    # the launch: the grid the plan gives for n rays, and n more than two sweeps of it
    facts = {**dc.scene_facts("teapot"), "stack_bound": scene.info().stack_bound, "members": 4 if name == "instances" else 0}
    kind = {"trace": pp.TRACE, "bounded": pp.BOUNDED, "occluded": pp.OCCLUDED}[api]
    cap = pp.plan(kind, pp.launch(facts, 0, 0, 0, cus=ctx.cu_count), n_rays=1 << 40)
    n = 2 * cap.grid * 256 + BASE + 37
    plan = pp.plan(kind, pp.launch(facts, 0, 0, 0, cus=ctx.cu_count), n_rays=n)
    assert plan.rc == 0 and plan.grid == cap.grid == ctx.cu_count * 8
    assert n > 2 * plan.grid * 256
    print(f"{name} {api}: n = {n}, grid = {plan.grid}")
    idx = torch.arange(n, device="cuda") % BASE
    to, td, tt = (x[idx].contiguous() for x in _cuda(o, d, tm))
    if api == "occluded":
        got = {"occluded": scene.occluded(to, td, tmax=tt).view(torch.uint8)}
        exp = {"occluded": wocc.astype(np.uint8)}
    else:
        got = scene.intersect(to, td, full=True, tmax=None if api == "trace" else tt)
        exp = {k: want[k].view(np.int32) if want[k].dtype == np.uint32 else want[k] for k in FULL}
    assert ctx.last_kernels() == [pp.name(plan)]
    tail = np.arange(n - 8192, n) % BASE
    for k, e in exp.items():
        g = got[k]
        assert g.shape[0] == n
        a = g.view(torch.int32) if g.dtype == torch.float32 else g
        (te,) = _cuda(e.view(np.int32) if e.dtype == F else e)
        bad = (a != te[idx]).reshape(n, -1).any(dim=1)
        assert not bool(bad.any()), f"{k}: {int(bad.sum())} rows, first {int(torch.nonzero(bad)[0])}"
        assert np.array_equal(a[-8192:].cpu().numpy(), (e.view(np.int32) if e.dtype == F else e)[tail]), k


@pytest.mark.parametrize("name", ["teapot", "group"])
def test_nullable_outputs(ctx, oracle, name):
    """mp_trace_rays_bounded through the C ABI with only d_prim, only d_normal and only d_instance non-NULL: that array as the
    full call writes it, and a guard region behind it untouched."""
    import torch

    scene, _, o, d = _make(name, ctx, oracle)
    o, d = o[:BASE], d[:BASE]
    unb = scene._oracle.trace_bounded(o, d)
    tm = _mixed_bounds(unb["t"], unb["prim"] != NO, np.random.default_rng(14))
    to, td, tt = _cuda(o, d, tm)
    full = scene.intersect(to, td, full=True, tmax=tt)
    assert name != "group" or int(full["instance"].max()) > 0
    oc, dc_ = to.t().contiguous(), td.t().contiguous()
    guard = 1024
    for field in ("prim", "normal", "instance"):
        ref = full[field]
        buf = torch.full((ref.numel() + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        hits = _lib.HitsSoA()
        setattr(hits, "d_" + field, buf.data_ptr())
        _lib.check(_lib.lib().mp_trace_rays_bounded(ctx.handle, scene.handle, *[x.data_ptr() for x in (oc[0], oc[1], oc[2], dc_[0], dc_[1], dc_[2])],
                                                    tt.data_ptr(), BASE, C.byref(hits), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        assert torch.equal(buf[:ref.numel()], ref.reshape(-1).view(torch.int32)), field
        assert bool((buf[ref.numel():] == 0x5A5A5A5A).all()), field


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
