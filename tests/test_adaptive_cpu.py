"""CPU tests of adaptive sampling: properties of the numpy model (tests/adaptive_model.py, the restatement of
include/minipath_adaptive.h that the GPU tests compare bits against), the round schedule, what libminipath_adaptive.so decides
before its first HIP call -- every refusal, through the built library without touching a GPU -- and the non-vacuity of the
end-to-end case of tests/test_gpu_adaptive.py, from the oracle alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import adaptive as ad
from tests import adaptive_model as m
from tests.adaptive_model import F, bits
from tests.conftest import ROOT

MP_ERR_INVALID = 1
SENTINEL = 0x5A5A5A5A
NAN, INF = float("nan"), float("inf")


# ---- the model -----------------------------------------------------------------------------------------------------------------
def test_error_against_f64():
    rng = np.random.default_rng(11)
    n, floor = 4000, 0.05
    for k in (1, 16, 48, 4096):
        hits = rng.integers(0, k + 1, n)
        mean = rng.random(n)                     # of the hit samples
        spread = rng.random(n) * 0.2
        spread[rng.random(n) < 0.2] = 0          # q / k == m * m up to rounding: the clamp at 0
        s = (mean * hits).astype(F)
        q = ((mean * mean + spread) * hits).astype(F)
        got = m.pixel_error(s, q, k, floor)
        assert got.dtype == F and np.all(got >= 0)
        s64, q64 = s.astype(np.float64), q.astype(np.float64)
        m64, m264 = s64 / k, q64 / k
        d64 = m264 - m64 * m64
        want = np.sqrt(np.maximum(d64, 0) / k) / (m64 + floor)
        # u = 2^-24.  r carries one rounding, m and m2 two, m*m five, the difference one more: d is off by at most
        # (3 m2 + 6 m*m) u plus second-order terms, within 7 u (m2 + m*m) absolutely, and so is max(d, 0) against max(d64, 0): dv
        # below, once divided by k.  On top of that come relative errors: v = max(d, 0) * r two roundings, which the square root
        # halves before adding its own (2 u), the denominator (m: 2 u, the sum of two positive numbers one more: 3 u), the
        # quotient (u): 6 u, taken as 8 u.
        u = 2.0 ** -24
        dv = 7 * u * (m264 + m64 * m64) / k
        v64 = np.maximum(d64, 0) / k
        bound = (np.sqrt(v64 + dv) - np.sqrt(v64)) / (m64 + floor) * (1 + 8 * u) + 8 * u * want + 1e-45
        assert np.all(np.abs(got.astype(np.float64) - want) <= bound), float(np.max(np.abs(got - want) - bound))


def test_all_miss_pixel_is_exactly_plus_zero():
    for k in (1, 16, (1 << 24) + 1):
        e = m.pixel_error(np.zeros(3, F), np.zeros(3, F), k, 0.05)
        assert np.all(bits(e) == 0)
    shade = np.zeros((2, 4, 4, 4), F)
    opened, err = m.tile_error(shade, shade, [[4, 4], [1, 3]], 16, 0.0, 0.05)
    assert list(opened) == [0, 0] and np.all(bits(err) == 0)  # converged even at threshold 0
    opened, _ = m.tile_error(shade, shade, [[4, 4], [1, 3]], 16, -1.0, 0.05)
    assert list(opened) == [16, 3]  # a negative threshold leaves every pixel open


def test_nan_moment_is_open_and_infinite():
    shade = np.zeros((1, 4, 4, 4), F)
    sq = np.zeros((1, 4, 4, 4), F)
    shade[0, 1, 2, 0] = NAN
    opened, err = m.tile_error(shade, sq, [[4, 4]], 8, 1e30, 0.05)
    assert list(opened) == [1] and err[0] == np.inf
    opened, err = m.tile_error(shade, sq, [[2, 4]], 8, 1e30, 0.05)  # not owned: not counted
    assert list(opened) == [0] and bits(err)[0] == 0
    shade[0, 1, 2, 0] = INF  # m = inf, m * m = inf, d = -inf or NaN -> v = 0, e = 0 / inf = +0
    opened, err = m.tile_error(shade, sq, [[4, 4]], 8, 0.0, 0.05)
    assert list(opened) == [0] and bits(err)[0] == 0
    # what follows from the header's max: a NaN SECOND moment alone is clamped away with the negative differences (d = NaN ->
    # v = 0); the render cannot produce one without a NaN first moment, which is the case above
    sq[0, 0, 0, 0] = NAN
    opened, err = m.tile_error(np.zeros_like(shade), sq, [[4, 4]], 8, INF, 0.05)
    assert list(opened) == [0] and bits(err)[0] == 0
    sq[0, 0, 0, 0] = INF  # v = inf, e = inf: closed only at threshold +inf
    opened, err = m.tile_error(np.zeros_like(shade), sq, [[4, 4]], 8, 1e30, 0.05)
    assert list(opened) == [1] and err[0] == np.inf
    opened, err = m.tile_error(np.zeros_like(shade), sq, [[4, 4]], 8, INF, 0.05)
    assert list(opened) == [0] and err[0] == np.inf
    # the order of max_err: -0 < +0, and a slot that owns nothing gives +0
    neg = np.zeros((2, 2, 2, 4), F)
    neg[0, :, :, 0] = -1.0  # m + floor < 0, v = 0: e = -0
    opened, err = m.tile_error(neg, np.zeros_like(neg), [[2, 2], [0, 2]], 1, 0.5, 0.05)
    assert bits(err)[0] == 0x80000000 and bits(err)[1] == 0 and list(opened) == [0, 0]


@pytest.mark.parametrize("args, want", [
    ((64, 16, 16), [0, 16, 32, 48, 64]),
    ((16, 16, 16), [0, 16]),          # min_samples == sample_count: one round, no check
    ((8, 16, 4), [0, 8]),             # min_samples > sample_count
    ((70, 16, 16), [0, 16, 32, 48, 64, 70]),  # ragged last round
    ((21, 16, 16), [0, 16, 21]),
    ((5, 2, 1), [0, 2, 3, 4, 5]),     # round_samples = 1
    ((1, 1, 1), [0, 1]),
    ((65536, 64, 4096), [0, 64] + list(range(4160, 65536, 4096)) + [65536]),
])
def test_round_bounds(args, want):
    got = ad.round_bounds(*args)
    assert got == want == m.round_bounds(*args)
    assert got[0] == 0 and got[-1] == args[0] and all(a < b for a, b in zip(got, got[1:]))


def test_round_bounds_refuses():
    for args in ((0, 1, 1), (8, 0, 1), (8, 1, 0), (8, -3, 2)):
        with pytest.raises(ValueError):
            ad.round_bounds(*args)


def test_move_and_finish_models():
    rng = np.random.default_rng(5)
    src = rng.random((4, 3, 3, 4)).astype(F)
    dst = np.zeros((3, 3, 3, 4), F)
    m.move_tiles(src, [3, 9, 0], dst, [1, 0, 7], 3)  # j = 1: the source is out of range; j = 2: the destination
    assert np.array_equal(dst[1], src[3]) and np.all(dst[0] == 0) and np.all(dst[2] == 0)
    fin = m.finish_tiles(src, [0, 5, 8, 9], [[3, 3], [2, 1], [3, 3], [3, 3]], 8)
    assert np.array_equal(fin[0], src[0]) and np.array_equal(fin[2], src[2]) and np.array_equal(fin[3], src[3])
    assert np.array_equal(bits(fin[1, :1, :2]), bits((src[1, :1, :2] * (F(1) / F(5))).astype(F)))
    keep = np.ones((3, 3), bool)
    keep[:1, :2] = False
    assert np.array_equal(fin[1][keep], src[1][keep])


# ---- the library, before its first HIP call --------------------------------------------------------------------------------------
def test_every_declared_symbol_has_a_signature():
    text = open(os.path.join(ROOT, "include", "minipath_adaptive.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mpa_\w+)\s*\(", text))
    assert declared == set(ad.SIGNATURES) and len(declared) == 5
    L = ad.lib()
    for name in declared:
        assert getattr(L, name).argtypes == ad.SIGNATURES[name][1]
    assert mp.AdaptiveSampler is ad.AdaptiveSampler


NO_DEVICE = 1 << 20  # no such GPU: were a call accepted by mistake, the runtime would refuse the device and nothing would be launched
TS, N = 4, 3
ERR_ARGS = ("shade", "shade_sq", "wh", "open", "max_err")


def _refused(call, bufs):
    before = ad.last_kernels()
    rc = call()
    assert rc == MP_ERR_INVALID and ad.lib().mpa_last_error()
    assert ad.last_kernels() == before  # nothing was launched
    for k, v in bufs.items():
        assert np.all(v == SENTINEL), k  # nothing was written (host memory here: a launch would not even get this far)


def _ids(d):
    return ",".join(f"{k}={v}" for k, v in d.items())


@pytest.mark.parametrize("bad", [dict(shade=None), dict(shade_sq=None), dict(wh=None), dict(open=None), dict(max_err=None), dict(n=0),
                                 dict(ts=0), dict(k=0), dict(threshold=NAN), dict(floor=0.0), dict(floor=-1.0), dict(floor=NAN),
                                 dict(floor=INF), dict(device=-1), dict(open="shade"), dict(open="shade_sq"), dict(open="wh"),
                                 dict(max_err="shade"), dict(max_err="shade_sq"), dict(max_err="wh"), dict(max_err="open")], ids=_ids)
def test_tile_error_refuses(bad):
    bufs = {k: np.full(N * TS * TS * 4, SENTINEL, np.uint32) for k in ERR_ARGS}
    ptr = {k: v.ctypes.data for k, v in bufs.items()}
    for k in ERR_ARGS:
        if k in bad:
            ptr[k] = None if bad[k] is None else ptr[bad[k]]
    _refused(lambda: ad.lib().mpa_tile_error(bad.get("device", NO_DEVICE), bad.get("ts", TS), bad.get("n", N), bad.get("k", 16),
                                             bad.get("threshold", 0.1), bad.get("floor", 0.05), *[ptr[k] for k in ERR_ARGS], None), bufs)


@pytest.mark.parametrize("bad", [dict(src=None), dict(dst=None), dict(dst="src"), dict(ts=0), dict(src_slots=0), dict(dst_slots=0),
                                 dict(device=-1)], ids=_ids)
def test_move_tiles_refuses(bad):
    names = ("src", "src_slot", "dst", "dst_slot")
    bufs = {k: np.full(N * TS * TS * 4, SENTINEL, np.uint32) for k in names}
    ptr = {k: v.ctypes.data for k, v in bufs.items()}
    for k in names:
        if k in bad:
            ptr[k] = None if bad[k] is None else ptr[bad[k]]
    _refused(lambda: ad.lib().mpa_move_tiles(bad.get("device", NO_DEVICE), bad.get("ts", TS), N, ptr["src"], bad.get("src_slots", N),
                                             ptr["src_slot"], ptr["dst"], bad.get("dst_slots", N), ptr["dst_slot"], None), bufs)


def test_move_tiles_of_nothing_is_a_no_op():
    bufs = {k: np.full(N * TS * TS * 4, SENTINEL, np.uint32) for k in ("src", "dst")}
    before = ad.last_kernels()
    assert ad.lib().mpa_move_tiles(NO_DEVICE, TS, 0, bufs["src"].ctypes.data, N, None, bufs["dst"].ctypes.data, N, None, None) == 0
    assert ad.last_kernels() == before and all(np.all(v == SENTINEL) for v in bufs.values())


@pytest.mark.parametrize("bad", [dict(plane=None), dict(samples=None), dict(wh=None), dict(n=0), dict(ts=0), dict(spp=0), dict(device=-1),
                                 dict(samples="plane"), dict(wh="plane")], ids=_ids)
def test_finish_tiles_refuses(bad):
    names = ("plane", "samples", "wh")
    bufs = {k: np.full(N * TS * TS * 4, SENTINEL, np.uint32) for k in names}
    ptr = {k: v.ctypes.data for k, v in bufs.items()}
    for k in names:
        if k in bad:
            ptr[k] = None if bad[k] is None else ptr[bad[k]]
    _refused(lambda: ad.lib().mpa_finish_tiles(bad.get("device", NO_DEVICE), bad.get("ts", TS), bad.get("n", N), bad.get("spp", 64),
                                               ptr["plane"], ptr["samples"], ptr["wh"], None), bufs)


def test_oversized_arguments_are_unsupported_not_launched():
    bufs = {k: np.full(16, SENTINEL, np.uint32) for k in ERR_ARGS}
    p = [bufs[k].ctypes.data for k in ERR_ARGS]
    L = ad.lib()
    before = ad.last_kernels()
    assert L.mpa_tile_error(NO_DEVICE, 65536, 1, 4, 0.1, 0.05, *p, None) == 5
    assert L.mpa_move_tiles(NO_DEVICE, 65535, 1 << 20, p[0], 1, None, p[1], 1, None, None) == 5  # 2^20 * 2^22 blocks
    assert L.mpa_finish_tiles(NO_DEVICE, 65536, 1, 4, p[0], p[1], p[2], None) == 5
    assert ad.last_kernels() == before and all(np.all(v == SENTINEL) for v in bufs.values())


def test_last_kernels_buffer_protocol():
    L = ad.lib()
    need = C.c_size_t(99)
    assert L.mpa_last_kernels(None, 0, C.byref(need)) == 0 and need.value == len("\n".join(ad.last_kernels()))
    assert L.mpa_last_kernels(None, 4, None) == MP_ERR_INVALID


def test_sampler_refuses_in_python():
    """decided from the arguments alone, before a scene, a Context or the library is touched"""
    cam = mp.Camera.teapot_view()
    for kw in (dict(chunked_sum=True), dict(traversal="groups"), dict(max_depth=2, wavefront=True)):
        with pytest.raises(ValueError, match="MP_FLAG"):
            mp.AdaptiveSampler(None, cam, mp.RenderSettings(16, 64, (32, 32), **kw), 0.1)
    st = mp.RenderSettings(16, 64, (32, 32))
    for kw in (dict(min_samples=0), dict(round_samples=0), dict(round_samples=-4), dict(planes=("shade", "beauty")), dict(floor=0.0),
               dict(floor=INF)):
        with pytest.raises(ValueError):
            mp.AdaptiveSampler(None, cam, st, 0.1, **kw)
    with pytest.raises(ValueError):
        mp.AdaptiveSampler(None, cam, st, NAN)


# ---- the end-to-end case is not vacuous --------------------------------------------------------------------------------------------
def test_the_end_to_end_case_holds_every_stop_class():
    """the teapot of adaptive_model.CASE under the model: tiles stop at the first check, at later checks, and run to the budget,
    with clipped tiles (the right column is 8 wide, the bottom row 8 high) among the stopped and among the unstopped"""
    frame, exp, tiles = m.teapot_case()
    c = m.CASE
    assert exp.bounds == [0, 16, 32, 48, 64] and len(tiles) == 15
    first = exp.bounds[1]
    at_first = [i for i in range(len(tiles)) if exp.samples[i] == first]
    later = [i for i in range(len(tiles)) if first < exp.samples[i] < c["spp"]]
    budget = [i for i in range(len(tiles)) if exp.samples[i] == c["spp"]]
    print("stop at", first, at_first, "later", later, "budget", budget, "samples", exp.samples.tolist())
    assert at_first and later and budget and len(at_first) + len(later) + len(budget) == len(tiles)
    clipped = {i for i in range(len(tiles)) if exp.area[i] < c["ts"] ** 2}
    assert clipped & set(at_first + later) and clipped & set(budget)
    assert any(w < c["ts"] for w, _ in exp.wh) and any(h < c["ts"] for _, h in exp.wh)
    # stopped tiles hold previews, budget tiles the plain frame's bits
    plain = {k: m.tile_major(v, tiles, c["ts"]) for k, v in frame.planes().items()}
    for i in budget:
        assert all(np.array_equal(bits(exp.planes[k][i]), bits(plain[k][i])) for k in m.PLANES)
    assert any(not np.array_equal(bits(exp.planes["shade"][i]), bits(plain["shade"][i])) for i in at_first + later)
    assert np.array_equal(bits(exp.planes["ids"]), bits(plain["ids"]))
    assert exp.samples_drawn == int(exp.sample_map(*c["res"]).sum()) < c["spp"] * c["res"][0] * c["res"][1]
