"""GPU tests of adaptive sampling (include/minipath_adaptive.h, minipath_amd.adaptive.AdaptiveSampler).  Every comparison is on
f32 / u32 bit patterns with zero differences allowed: the three device operations against the numpy model
(tests/adaptive_model.py) on synthetic planes inside guard regions, mpa_finish_tiles against mp_untile_preview, and the driver
against the model over the oracle, against the plain render (threshold -1) and against the plain render's preview (threshold
+inf)."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import adaptive as ad
from tests import adaptive_model as m
from tests.adaptive_model import CASE, FLOAT_PLANES, PLANES, F, bits
from tests.conftest import TEAPOT
from tests.test_gpu_aov import _options, _scene

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
PAD = 4096
ALL = {k: True for k in PLANES}
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "gpu tests need a GPU"
    return t


@pytest.fixture(scope="module")
def ctx(torch):
    c = mp.Context(0)
    yield c
    _options(c)


class Guarded:
    """a host array (any 4-byte dtype) on the device in the middle of a larger tensor of sentinels"""

    def __init__(self, torch, a):
        self.torch, self.shape, self.dtype = torch, a.shape, a.dtype
        raw = np.ascontiguousarray(a).reshape(-1).view(np.int32)
        self.n = raw.size
        self.whole = torch.full((PAD + self.n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.whole[PAD:PAD + self.n].copy_(torch.from_numpy(raw.copy()))

    @property
    def ptr(self):
        return self.whole.data_ptr() + 4 * PAD

    def host(self):
        return self.whole[PAD:PAD + self.n].cpu().numpy().view(self.dtype).reshape(self.shape)

    def guards_intact(self):
        raw = self.whole.cpu().numpy()
        return bool(np.all(raw[:PAD] == SENTINEL) and np.all(raw[-PAD:] == SENTINEL))


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _extents(n, ts):
    """1 x 1, a single row, a single column, full, and odd ones in between"""
    kinds = [(ts, ts), (1, 1), (ts, 1), (1, ts), (ts // 2 + 1, ts - 1), (ts - 1, ts // 2 + 1), (ts, ts // 2), (2, 3)]
    return np.array([kinds[i % len(kinds)] for i in range(n)], np.uint32)


def _poison_tails(a, wh, seed):
    """what a slot does not own: NaN in one slot, the sentinel in the next (a is [n, ts, ts, 4] float32, changed in place)"""
    ts = a.shape[1]
    own = np.zeros(a.shape[:3], bool)
    for i, (w, h) in enumerate(wh):
        own[i, :h, :w] = True
    raw = a.view(np.uint32)
    for i in range(a.shape[0]):
        raw[i][~own[i]] = 0x7FC00000 if (i + seed) % 2 == 0 else SENTINEL
    return own


def _state_planes(n, ts, k, seed):
    """synthetic {sum, sum, sum, hits} planes after k samples, with NaN, inf, negative and zero moments among the owned pixels"""
    rng = np.random.default_rng(seed)
    wh = _extents(n, ts)
    hits = rng.integers(0, 5, (n, ts, ts)) / 4.0                  # fraction of samples that hit
    mean = rng.random((n, ts, ts))
    spread = rng.random((n, ts, ts)) * rng.choice([0.0, 0.02, 0.3], (n, ts, ts))
    s = (mean * hits * k).astype(F)
    q = ((mean * mean + spread) * hits * k).astype(F)
    special = [(NAN, 1.0), (INF, 1.0), (-3.0, 2.0), (0.0, 0.0), (0.5, NAN), (0.5, INF), (-0.0, 0.0), (1.0, -1.0)]
    for i, (w, h) in enumerate(wh):
        w, h = int(w), int(h)
        for j, (vs, vq) in enumerate(special):
            if w * h == 1 and j != i % len(special):
                continue
            if i % 3 == 1 or (i % 3 == 2 and (vs != vs or vq == INF)):
                continue  # every third slot holds none, so that its max_err is an ordinary number; every third none that gives +inf
            p = (i * 7 + j * 3) % (w * h)
            s[i, p // w, p % w], q[i, p // w, p % w] = vs, vq
    shade, sq = np.zeros((n, ts, ts, 4), F), np.zeros((n, ts, ts, 4), F)
    shade[..., :3], sq[..., :3] = s[..., None], q[..., None]
    shade[..., 3] = sq[..., 3] = (hits * k).astype(F)
    _poison_tails(shade, wh, 0)
    _poison_tails(sq, wh, 1)
    return shade, sq, wh


# 1. mpa_tile_error against the model
@pytest.mark.parametrize("n", [1, 5, 300])
@pytest.mark.parametrize("ts", [5, 16, 64])
def test_tile_error_matches_the_model(torch, ts, n):
    L = ad.lib()
    mid = 0.1
    for k in (1, 16, (1 << 24) + 1):
        shade, sq, wh = _state_planes(n, ts, k, seed=ts * 1000 + n)
        g = {"shade": Guarded(torch, shade), "shade_sq": Guarded(torch, sq), "wh": Guarded(torch, wh),
             "open": Guarded(torch, np.full(n, SENTINEL, np.uint32)), "max_err": Guarded(torch, np.full(n, SENTINEL, np.uint32).view(F))}
        for threshold in (0.0, mid, -1.0):
            ad.check(L.mpa_tile_error(0, ts, n, k, threshold, 0.05, g["shade"].ptr, g["shade_sq"].ptr, g["wh"].ptr, g["open"].ptr,
                                      g["max_err"].ptr, _stream(torch)))
            assert ad.last_kernels() == ["tile_error_kernel"]
            torch.cuda.synchronize()
            want_open, want_err = m.tile_error(shade, sq, wh, k, threshold, 0.05)
            got_open, got_err = g["open"].host(), g["max_err"].host()
            print(ts, n, k, threshold, "open", int(got_open.sum()), "of", int((wh[:, 0] * wh[:, 1]).sum()), "max", float(np.max(got_err)))
            assert np.array_equal(got_open, want_open), (k, threshold)
            assert np.array_equal(bits(got_err), bits(want_err)), (k, threshold)
            owned = wh[:, 0].astype(np.int64) * wh[:, 1]
            if threshold < 0:
                assert np.array_equal(got_open, owned)  # every owned pixel, and nothing of the tails
            if threshold == mid and n >= 5 and k == 16:
                assert np.any(got_open == 0) or np.any(got_open < owned), "the mid threshold must close some pixels"
                assert np.any(got_open > 0)
        for name in g:
            assert g[name].guards_intact(), name
        assert np.array_equal(bits(g["shade"].host()), bits(shade)) and np.array_equal(bits(g["shade_sq"].host()), bits(sq))
        assert np.array_equal(g["wh"].host(), wh)


# 2. mpa_move_tiles: permutation, gather, scatter back, NULL arrays, skipped indices, an int32 plane
@pytest.mark.parametrize("dtype", [np.float32, np.int32], ids=["f32", "i32"])
@pytest.mark.parametrize("ts", [5, 16, 33, 64])
def test_move_tiles(torch, ts, dtype):
    L = ad.lib()
    rng = np.random.default_rng(ts)
    n_src, n_dst = 7, 9
    src = rng.integers(0, 1 << 32, (n_src, ts, ts, 4), dtype=np.uint64).astype(np.uint32).view(dtype)  # any bits: NaNs of every kind
    fill = np.full((n_dst, ts, ts, 4), SENTINEL, np.uint32).view(dtype)

    def idx(v):
        return None if v is None else Guarded(torch, np.asarray(v, np.uint32))

    def move(n, s, s_idx, d, d_idx):
        gs, gd = idx(s_idx), idx(d_idx)
        ad.check(L.mpa_move_tiles(0, ts, n, s.ptr, s.shape[0], gs.ptr if gs else None, d.ptr, d.shape[0], gd.ptr if gd else None,
                                  _stream(torch)))
        assert ad.last_kernels() == ["move_tiles_kernel"]
        torch.cuda.synchronize()
        assert all(x.guards_intact() for x in (s, d, gs, gd) if x is not None)
        want = m.move_tiles(s.host(), s_idx, d.host_before, d_idx, n)
        assert np.array_equal(bits(d.host()), bits(want))
        d.host_before = want

    def dev(a):
        g = Guarded(torch, a)
        g.host_before = a.copy()
        return g

    g_src = dev(src)
    # a permutation
    perm = [int(i) for i in rng.permutation(n_src)]
    d = dev(fill)
    move(n_src, g_src, perm, d, list(reversed(range(n_src))))
    assert np.all(bits(d.host()[n_src:]) == SENTINEL)
    # a gather of a subset into compact slots, and the scatter back into a fresh buffer: the source's slots, nothing else
    sub = [5, 1, 3]
    work = dev(fill)
    move(3, g_src, sub, work, None)
    assert np.array_equal(bits(work.host()[:3]), bits(src[sub])) and np.all(bits(work.host()[3:]) == SENTINEL)
    back = dev(fill)
    move(3, work, None, back, sub)
    assert np.array_equal(bits(back.host()[sub]), bits(src[sub]))
    rest = [i for i in range(n_dst) if i not in sub]
    assert np.all(bits(back.host()[rest]) == SENTINEL)
    # both arrays NULL: slots 0..n-1 as they are
    same = dev(fill)
    move(4, g_src, None, same, None)
    assert np.array_equal(bits(same.host()[:4]), bits(src[:4]))
    # indices out of range are skipped, their neighbours move
    skip = dev(fill)
    move(4, g_src, [0, n_src, 2, 0xFFFFFFFF], skip, [1, 2, n_dst, 4])
    assert np.array_equal(bits(skip.host()[1]), bits(src[0]))
    assert np.all(bits(skip.host()[[0, 2, 3, 4, 5, 6, 7, 8]]) == SENTINEL)
    assert np.array_equal(bits(g_src.host()), bits(src))


# 3. mpa_finish_tiles against the model, and against mp_untile_preview
@pytest.mark.parametrize("ts", [5, 16, 33, 64])
def test_finish_tiles_matches_the_model(torch, ts):
    L = ad.lib()
    n, spp = 11, 48
    rng = np.random.default_rng(ts + 1)
    wh = _extents(n, ts)
    plane = (rng.random((n, ts, ts, 4)) * 100 - 20).astype(F)
    plane[0, 0, 0] = (NAN, INF, -0.0, 1e-44)
    _poison_tails(plane, wh, 0)
    samples = np.array([0, 1, 7, spp, spp + 1, 3, 47, spp, 0xFFFFFFFF, 16, 5], np.uint32)
    g_plane, g_k, g_wh = Guarded(torch, plane), Guarded(torch, samples), Guarded(torch, wh)
    ad.check(L.mpa_finish_tiles(0, ts, n, spp, g_plane.ptr, g_k.ptr, g_wh.ptr, _stream(torch)))
    assert ad.last_kernels() == ["finish_tiles_kernel"]
    torch.cuda.synchronize()
    want = m.finish_tiles(plane, samples, wh, spp)
    assert np.array_equal(bits(g_plane.host()), bits(want))  # tails included: they come back as they were
    for i in (0, 3, 4, 7, 8):
        assert np.array_equal(bits(want[i]), bits(plane[i]))
    assert not np.array_equal(bits(want[2]), bits(plane[2]))
    assert all(g.guards_intact() for g in (g_plane, g_k, g_wh))
    assert np.array_equal(g_k.host(), samples) and np.array_equal(g_wh.host(), wh)


def _sampler(ctx, threshold, obj=None, cam=None, case=CASE, planes=PLANES, **kw):
    obj = mp.TriangleBvh.with_obj(TEAPOT, ctx) if obj is None else obj
    st = mp.RenderSettings(case["ts"], case["spp"], case["res"], seed=case["seed"])
    args = dict(floor=case["floor"], min_samples=case["min_samples"], round_samples=case["round_samples"], planes=planes)
    args.update(kw)
    return mp.AdaptiveSampler(mp.Scene(obj), mp.Camera.teapot_view() if cam is None else cam, st, threshold, **args)


def _host(torch, planes):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in planes.items()}


def _owned(tiles, ts):
    own = np.zeros((len(tiles), ts, ts), bool)
    for i, t in enumerate(tiles):
        own[i, : t.height(), : t.width()] = True
    return own


def _same_owned(got, want, own, what, slots=None, names=PLANES):
    for k in names:
        a, b = bits(got[k]), bits(want[k])
        sel = own if slots is None else own & np.isin(np.arange(own.shape[0]), slots)[:, None, None]
        diff = int(np.sum(a[sel] != b[sel]))
        assert diff == 0, (what, k, diff)


def test_finish_of_a_uniform_k_is_the_preview(torch, ctx):
    _options(ctx)
    ad_ = _sampler(ctx, -1.0)
    fr = ad_.fr
    state = fr.new_aov_planes(**ALL)
    fr.render_aov_pass(state, 0, 16)
    k = torch.full((len(fr.tiles),), 16, dtype=torch.int32, device="cuda")
    for name in FLOAT_PLANES:
        fin = state[name].clone()
        ad.check(ad.lib().mpa_finish_tiles(0, CASE["ts"], len(fr.tiles), CASE["spp"], fin.data_ptr(), k.data_ptr(), ad_._d_wh.data_ptr(),
                                           _stream(torch)))
        got, want = fr.untile_plane(fin), fr.untile_plane(state[name], preview_samples=16)
        torch.cuda.synchronize()
        assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy())), name
        if name != "normal":  # (whose .w is the depth)
            assert float(want[..., 3].max().item()) == 1.0, "a preview: hit counts / k"


# 4. end to end against the model over the oracle
def test_end_to_end_equals_the_model(torch, ctx):
    _options(ctx)
    frame, exp, tiles = m.teapot_case()
    ad_ = _sampler(ctx, CASE["threshold"])
    assert ad_.fr.tiles == tiles
    own = _owned(tiles, CASE["ts"])
    spp, n = CASE["spp"], len(tiles)
    final = exp.planes
    prev = None
    for b in exp.bounds[1:]:
        was_active = list(ad_.active)
        assert ad_.step() is True
        got = _host(torch, ad_.planes)
        want_k = np.minimum(exp.samples, b)
        assert np.array_equal(ad_.samples, want_k), (b, ad_.samples.tolist())
        # tiles of this round hold the state after b samples (the means, at the budget); the others are frozen
        if b < spp:
            _same_owned(got, exp.states[b], own, ("state", b), slots=was_active)
            chk = [c for c in exp.checks if c[0] == b][0]
            assert chk[1] == was_active
            assert np.array_equal(ad_.open[was_active], chk[2]) and np.array_equal(bits(ad_.max_err[was_active]), bits(chk[3]))
            assert ad_.active == [i for i, o in zip(chk[1], chk[2]) if o != 0]
        else:
            _same_owned(got, final, own, ("budget tiles", b), slots=was_active)
            assert ad_.active == []
        if prev is not None:
            frozen = [i for i in range(n) if i not in was_active]
            _same_owned(got, prev, own, ("frozen", b), slots=frozen)
            for i in frozen:
                assert np.array_equal(bits(got["shade"][i]), bits(prev["shade"][i]))  # the whole slot
        prev = got
    assert ad_.step() is False and ad_.round == len(exp.bounds) - 1
    ad_.finish()
    ad_.finish()  # once
    got = _host(torch, ad_.planes)
    assert sorted(got) == sorted(PLANES)
    _same_owned(got, final, own, "finished frame")
    assert np.array_equal(ad_.samples, exp.samples)
    stops = {int(k) for k in ad_.samples}
    assert CASE["min_samples"] in stops and spp in stops and any(CASE["min_samples"] < k < spp for k in stops)
    assert ad_.samples_drawn == exp.samples_drawn
    assert np.array_equal(ad_.sample_map(), exp.sample_map(*CASE["res"])) and ad_.sample_map().dtype == np.int32
    # the image: untile_plane applies as to a plain render's planes
    img = ad_.untile_plane("shade")
    torch.cuda.synchronize()
    want = np.zeros((CASE["res"][1], CASE["res"][0], 4), F)
    for i, t in enumerate(tiles):
        want[t.min_y:t.max_y, t.min_x:t.max_x] = final["shade"][i, : t.height(), : t.width()]
    assert np.array_equal(bits(img.cpu().numpy()), bits(want))


def test_render_is_step_to_the_end_and_finish(torch, ctx):
    _options(ctx)
    _, exp, tiles = m.teapot_case()
    ad_ = _sampler(ctx, CASE["threshold"], planes=("shade",))  # shade_sq comes along by itself
    out = ad_.render()
    assert out is ad_.planes and sorted(out) == ["shade", "shade_sq"] and ad_.finished
    _same_owned(_host(torch, out), exp.planes, _owned(tiles, CASE["ts"]), "render()", names=("shade", "shade_sq"))
    assert np.array_equal(ad_.samples, exp.samples)
    with pytest.raises(RuntimeError):
        ad_.active = [0]
        ad_.step()


# 5. threshold -1: nothing stops, the frame is the plain render's
@pytest.mark.parametrize("name", ["teapot", "group"])
def test_negative_threshold_is_the_plain_render(torch, ctx, oracle, name):
    _options(ctx)
    obj, cam, _, _ = _scene(name, ctx, oracle)
    case = dict(CASE, spp=40)  # rounds 16, 16 and a ragged 8
    ad_ = _sampler(ctx, -1.0, obj, cam, case)
    ad_.render()
    assert ad_.bounds == [0, 16, 32, 40] and np.all(ad_.samples == 40) and ad_.round == 3
    assert np.array_equal(ad_.open, ad_._area), "every pixel was open at every check"
    plain = ad_.fr.new_aov_planes(**ALL)
    ad_.fr.render_aov_pass(plain)
    got, want = _host(torch, ad_.planes), _host(torch, plain)
    hit = want["ids"].view(np.uint32)[..., 3]
    assert 0 < hit.sum() < CASE["res"][0] * CASE["res"][1], "the view must hold hits and misses"
    for k in PLANES:
        assert np.array_equal(bits(got[k]), bits(want[k])), (name, k)
    assert ad_.samples_drawn == 40 * CASE["res"][0] * CASE["res"][1]


# 6. threshold +inf: every tile stops at min_samples, the frame is the plain render's preview after min_samples
def test_infinite_threshold_is_the_preview_after_min_samples(torch, ctx):
    _options(ctx)
    ad_ = _sampler(ctx, INF, min_samples=7)
    ad_.render()
    assert np.all(ad_.samples == 7) and ad_.round == 1 and np.all(ad_.open == 0)
    fr = ad_.fr
    state = fr.new_aov_planes(**ALL)
    fr.render_aov_pass(state, 0, 7)
    for k in FLOAT_PLANES:
        got, want = ad_.untile_plane(k), fr.untile_plane(state[k], preview_samples=7)
        torch.cuda.synchronize()
        assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy())), k
    got, want = ad_.untile_plane("ids"), fr.untile_plane(state["ids"])
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    assert ad_.samples_drawn == 7 * CASE["res"][0] * CASE["res"][1]
