"""CPU tests of the sky lighting: the numpy model (tests/sky_model.py, the restatement of include/minipath_sky.h that the GPU tests
compare bits against) against a float64 evaluation and against what the map stands for, the conditions on the inputs of the GPU cases
(tests/sky_cases.py), and what libminipath_sky.so decides before its first HIP call -- every refusal, the struct size, the symbols --
through the built library without touching a GPU."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import sky
from tests import secondary_model as sm, sky_cases as tc, sky_model as m, stream_cases
from tests.conftest import ROOT, TEAPOT
from tests.sky_model import F, bits

MP_ERR_INVALID, MP_ERR_HIP = 1, 4
SENTINEL = 0x5A5A5A5A
INF, NAN = float("inf"), float("nan")
U = 2.0 ** -24  # the unit roundoff of binary32: the relative error of one correctly rounded operation


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the model -----------------------------------------------------------------------------------------------------------------
# The error of the lookup in binary32 against the same formulas without rounding, to first order in U.
#   The position in the map.  l1 is two additions of non-negative terms: relative error 2 U.  px = m.x / l1: 3 U relative, and
#   |px| <= 1, so 3 U absolute.  The fold 1 - |py| keeps the 3 U and adds one rounding of a value of at most 1: 4 U.  u = px * 0.5
#   (exact) + 0.5 halves that and adds one rounding of a value of at most 1: 3 U.  u * Nf: 3 U N and one rounding of a value of at most
#   N: 4 U N;  - 0.5: one more: 5 U N.  The clamps, floor and wx = fx - x0 are exact.  So |fx - fx*| <= 5 U N, and the same for fy;
#   POSITION_ROUNDINGS = 6 leaves one for the second-order terms.
#   The interpolation.  The exact interpolant is continuous and piecewise bilinear in (fx, fy), with slope at most D along either
#   axis, D = the largest difference between two neighbouring texels: moving the position costs at most (|dfx| + |dfy|) D, also
#   across a texel boundary, where the binary32 and the exact evaluation take different taps.  Each of top and bot is 1 - wx (one
#   rounding), two products and a sum: 3 U relative for texels of one sign, and L the same again over them: 6 U relative, at most
#   6 U Tmax; INTERPOLATION_ROUNDINGS = 7 likewise leaves one.
#   |L - L*| <= 2 * 6 U N D + 7 U Tmax.   For a map of one colour D = 0: |L - c| <= 7 U |c|.
POSITION_ROUNDINGS, INTERPOLATION_ROUNDINGS = 6, 7


def lookup_bound(n, env):
    T = env[..., :3].astype(np.float64)
    D = max(np.abs(np.diff(T, axis=0)).max(initial=0.0), np.abs(np.diff(T, axis=1)).max(initial=0.0))
    return 2 * POSITION_ROUNDINGS * U * n * D + INTERPOLATION_ROUNDINGS * U * np.abs(T).max()


def lookup64(env, d, pole):
    """the header's lookup in float64 on the same float32 inputs"""
    T = np.asarray(env, np.float64)[..., :3]
    n = T.shape[0]
    mm = m.to_map(d, pole).astype(np.float64)
    l1 = np.abs(mm).sum(-1)
    px, py = mm[:, 0] / l1, mm[:, 1] / l1
    lower = mm[:, 2] < 0
    px, py = np.where(lower, np.copysign(1 - np.abs(py), px), px), np.where(lower, np.copysign(1 - np.abs(px), py), py)
    L = 0
    taps = []
    for p in (px, py):
        f = np.clip((p * 0.5 + 0.5) * n - 0.5, 0, n - 1)
        i0 = np.floor(f).astype(np.int64)
        taps.append((i0, np.minimum(i0 + 1, n - 1), f - i0))
    (x0, x1, wx), (y0, y1, wy) = taps
    top = T[y0, x0] * (1 - wx)[:, None] + T[y0, x1] * wx[:, None]
    bot = T[y1, x0] * (1 - wx)[:, None] + T[y1, x1] * wx[:, None]
    L = top * (1 - wy)[:, None] + bot * wy[:, None]
    return L, lower


def _directions(count, seed):
    """seeded directions of every orientation, each scaled by a power of two between 2^-20 and 2^20"""
    rng = np.random.default_rng(seed)
    d = rng.normal(0, 1, (count, 3))
    return (d * 2.0 ** rng.integers(-20, 21, (count, 1))).astype(F)


@pytest.mark.parametrize("pole", tc.POLES)
@pytest.mark.parametrize("n", tc.MAPS)
def test_the_lookup_against_float64(n, pole):
    """10 000 directions in a map of random texels: within the bound derived above"""
    env = tc.texel_map(n)
    d = _directions(10000, 77 + n)
    L, info = m.lookup(env, d, pole, want_info=True)
    L64, lower = lookup64(env, d, pole)
    assert info["ok"].all() and np.array_equal(info["folded"], lower) and 0.4 < lower.mean() < 0.6
    bound = lookup_bound(n, env)
    err = np.abs(L.astype(np.float64) - L64).max()
    print(n, pole, "max error", err, "bound", bound)
    assert err <= bound
    if n > 1:
        assert err > 0 and len(set(zip(info["x0"].tolist(), info["y0"].tolist()))) >= min(n * n, 1000) // 2  # and it is no empty statement


@pytest.mark.parametrize("pole", tc.POLES)
@pytest.mark.parametrize("n", tc.MAPS)
def test_texel_centres_come_back_as_their_texel(n, pole):
    """decode to encode: the direction mpe_fill_gradient gives the centre of every texel, looked up in a map that holds the texel's own
    index, returns exactly that texel: x0 = i, y0 = j, wx = wy = 0, and the fold is taken for exactly the texels below the horizon"""
    centres, lower = m.texel_directions(n)
    d = m.from_map(centres.reshape(-1, 3), pole)
    env = tc.index_map(n)
    L, info = m.lookup(env, d, pole, want_info=True)
    jj, ii = np.divmod(np.arange(n * n), n)
    assert info["ok"].all() and np.array_equal(info["x0"], ii) and np.array_equal(info["y0"], jj)
    assert not info["wx"].any() and not info["wy"].any() and np.array_equal(info["folded"], lower.reshape(-1))
    assert _same(L, env.reshape(-1, 4)[:, :3])
    if n > 2:  # (one texel is the zenith, z = 1 at its centre; the four centres of N = 2 lie on the horizon, z = 0)
        assert lower.any() and (~lower).any()


@pytest.mark.parametrize("n", tc.MAPS)
def test_a_map_of_one_colour_returns_it(n):
    """10 000 seeded directions, every pole: the colour within 7 U of itself (the bound above with D = 0), negative components too"""
    colour = np.array([0.7, -3.3, 1e-3], F)
    env = np.zeros((n, n, 4), F)
    env[..., :3] = colour
    env[..., 3] = np.nan
    assert lookup_bound(n, env) == INTERPOLATION_ROUNDINGS * U * np.abs(colour.astype(np.float64)).max()
    for pole in tc.POLES:
        L = m.lookup(env, _directions(10000, 5 + pole), pole)
        assert np.all(np.abs(L.astype(np.float64) - colour.astype(np.float64)) <= INTERPOLATION_ROUNDINGS * U * np.abs(colour.astype(np.float64)))


@pytest.mark.parametrize("pole", tc.POLES)
def test_a_horizontal_plane_sees_the_sky_or_the_ground(oracle, pole):
    """white zenith and horizon, black ground, nothing in the way: a plane whose normal is the pole has a mean of 1, one that faces
    away a mean of 0 -- up to the map's resolution.  A tap can touch a texel of the other half only where the direction's octahedral
    height |m.z| / l1 is below two texels' worth, 2 * (2 / N) in each of px and py: 4 / N; and |m.z| / l1 >= h / sqrt(3) for the sine h
    of the elevation, so only for h < 4 sqrt(3) / N.  Cosine-distributed rays have h < x with probability x^2: the expected share of
    such samples is 48 / N^2.  Every other sample is 1 (or 0) to within the 7 U of the bound above, and every sample lies between 0 and
    1 + 7 U: the mean differs from 1 (or 0) by at most the share f of such samples that the seed drew, plus 7 U, plus the rounding of
    the sum and the divide (S - 1 additions of partial sums of at most S, over S, and one divide: S U); and f is within three times its
    expectation."""
    n, w, h, samples = 64, 8, 8, 64
    env = m.fill_gradient(n, (1, 1, 1), (1, 1, 1), (0, 0, 0))
    axis = m.from_map(np.array([0, 0, 1], F), pole)
    rng = np.random.default_rng(3 + pole)
    points = rng.uniform(-1, 1, (h, w, 3)).astype(F)
    position = np.concatenate([points, np.ones((h, w, 1), F)], -1)
    free = lambda o, d, t: np.zeros(len(t), np.uint8)  # noqa: E731
    eps = 7 * U
    for sign in (1, -1):
        normal = np.concatenate([np.broadcast_to(sign * axis, (h, w, 3)), np.ones((h, w, 1), F)], -1).astype(F)
        eye = 100 * sign * axis  # on the normal's side: the normal is kept
        out, sums, rays = m.run(oracle, free, position, normal, env, 11, samples, 16, eye, pole=pole, want_rays=True)
        d = rays["d"].astype(np.float64)
        hgt = sign * m.to_map(d, pole)[..., 2] / np.linalg.norm(d, axis=-1)
        assert np.all(sums[..., 3] == samples) and np.all(hgt >= 0)
        L = m.lookup(env, rays["d"].reshape(-1, 3), pole).reshape(samples, h, w, 3)
        clear = hgt >= 4 * np.sqrt(3) / n
        f = 1 - clear.mean(0)  # per pixel
        want = 1.0 if sign > 0 else 0.0
        assert np.all(np.abs(L[clear] - want) <= eps) and L.min() >= 0 and L.max() <= 1 + eps
        assert np.all(np.abs(out[..., :3] - want) <= f[..., None] + eps + samples * U) and np.all(out[..., 3] == 1)
        print(pole, sign, "mean", out[..., :3].mean(), "share near the horizon", f.mean())
        assert abs(out[..., :3].mean(dtype=np.float64) - want) <= f.mean() + eps + samples * U and f.mean() <= 3 * 48 / n ** 2


def test_batches_do_not_change_the_result(oracle):
    """8 samples in one batch equal 3 + 3 + 2, sums, out and the visibility, bit for bit, on a synthetic plane set with an occluder that
    is a function of the ray alone"""
    from tests import secondary_cases

    c = secondary_cases.synthetic(37, 23)
    env = tc.texel_map(5)

    def occluder(o, d, tmax):
        return ((bits(d[:, 0]) ^ bits(o[:, 1])) >> 3) & 1

    kw = dict(pole=2, radius=0.75, visibility=True)
    a = m.run(oracle, occluder, c["position"], c["normal"], env, 5, 8, 8, secondary_cases.EYE, **kw)
    b = m.run(oracle, occluder, c["position"], c["normal"], env, 5, 8, 3, secondary_cases.EYE, **kw)
    assert all(_same(x, y) for x, y in zip(a, b))
    free = m.run(oracle, lambda o, d, t: np.zeros(len(t), np.uint8), c["position"], c["normal"], env, 5, 8, 8, secondary_cases.EYE, **kw)
    assert 0 < a[1][..., :3].sum() < free[1][..., :3].sum()
    # and the visibility is SecondaryVisibility's model for the same seed
    ao, counts = sm.run(oracle, occluder, c["position"], c["normal"], sm.MODE_AO, 5, 8, 3, np.array(secondary_cases.EYE, F), radius=0.75)
    assert _same(a[2], ao) and _same(a[3], counts)
    assert np.array_equal(a[1][..., 3], counts[..., 1])  # the same samples are counted


def test_resolve_sums_by_the_codes():
    """one pixel, one texel, every tmax code with both answers: a sample is counted for tmax > 0 or -1, looked up only when it was traced
    and not occluded; a looked-up direction without a finite positive l1 adds +0 and stays counted"""
    env = np.array([[[2.0, 0.5, 8.0, NAN]]], F)
    tmax = np.array([0.5, 0.5, -1.0, 0.0, NAN, INF, -2.0, -0.0, 3.0, 1.0], F)
    occ = np.array([0, 1, 0, 0, 0, 0, 0, 0, 7, 0], np.uint8)
    d = np.array([[0, 1, 0]] * 9 + [[0, 0, 0]], F)
    sums, out = m.resolve(env, d[:, 0], d[:, 1], d[:, 2], tmax, occ, (1, 1), 10, 1)
    # counted: 0, 1, 2, 5, 8, 9; looked up: 0, 5 and 9, the last with a zero direction
    assert sums[0, 0].tolist() == [4.0, 1.0, 16.0, 6.0]
    assert _same(out[0, 0], np.array([F(4) / F(6), F(1) / F(6), F(16) / F(6), 1], F))
    more, _ = m.resolve(env, d[:, 0], d[:, 1], d[:, 2], tmax, occ, (1, 1), 10, 1, sums=np.array([[[1.0, -0.0, 1.0, 5.0]]], F))
    assert more[0, 0].tolist() == [5.0, 1.0, 17.0, 11.0]
    # -0 in the sums: a looked-up sample of a zero direction makes it +0 (E + L with L = +0), a sample that is not looked up leaves it
    z = np.array([[[-0.0, -0.0, -0.0, 0.0]]], F)
    looked, _ = m.resolve(env, d[9:, 0], d[9:, 1], d[9:, 2], tmax[9:], occ[9:], (1, 1), 1, 1, sums=z)
    skipped, out0 = m.resolve(env, d[1:2, 0], d[1:2, 1], d[1:2, 2], np.array([0.0], F), occ[1:2], (1, 1), 1, 1, sums=z)
    assert not np.signbit(looked[0, 0, :3]).any() and np.signbit(skipped[0, 0, :3]).all()
    assert out0[0, 0].tolist() == [0, 0, 0, 0]  # nothing counted: alpha 0, black
    assert m.resolve(env, d[:, 0], d[:, 1], d[:, 2], tmax, occ, (1, 1), 10, 1, want_out=False)[1] is None


def test_the_gradient_map():
    """mpe_fill_gradient's model: the zenith's colour at the zenith's texels, the ground's below the horizon, a blend above it that
    follows the elevation's sine, 1 in every .w; the texel in which the horizon's own colour appears exactly is the one at h = 0"""
    z, hz, g = tc.E2E["zenith"], tc.E2E["horizon"], tc.E2E["ground"]
    for n in tc.MAPS + [16]:
        env = m.fill_gradient(n, z, hz, g)
        centres, lower = m.texel_directions(n)
        assert env.shape == (n, n, 4) and np.all(env[..., 3] == 1) and np.all(env[lower][:, :3] == np.array(g, F))
        hgt = centres[..., 2].astype(np.float64) / np.linalg.norm(centres.astype(np.float64), axis=-1)
        want = np.array(hz) + (np.array(z) - np.array(hz)) * hgt[..., None]
        assert np.all(np.abs(env[~lower][:, :3] - want[~lower]) <= 8 * U * 2)  # five roundings of values of at most 1.5
    assert _same(m.fill_gradient(1, z, hz, g)[0, 0, :3], np.array(z, F))  # one texel: the zenith itself (h = 1)
    assert np.all(m.texel_directions(2)[0][..., 2] == 0) and _same(m.fill_gradient(2, z, hz, g)[..., :3], np.broadcast_to(np.array(hz, F), (2, 2, 3)))


# ---- the inputs of the GPU cases -------------------------------------------------------------------------------------------------
def test_the_synthetic_cases_reach_every_rule():
    """in the largest case of every map size, at least tc.MIN_PER_RULE looked-up rays each: every planted kind of direction, folded and
    unfolded lookups, a lookup without a finite positive l1, taps on one texel (wx = wy = 0), on a texel edge (a weight of exactly
    0.5) and clamped at the border; and every tmax code with both answers over the whole matrix"""
    w, h = tc.SIZES[-1]
    for n in tc.MAPS:
        r = tc.resolve_inputs(w, h, tc.BATCHES[-1], n)
        looked = (r["tmax"] > 0) & (r["occluded"] == 0)
        _, info = m.lookup(tc.texel_map(n), r["m"], 2, want_info=True)
        seen = collections.Counter(np.array(tc.KINDS)[r["kind"][looked]].tolist())
        ok = looked & info["ok"]
        seen["folded"], seen["unfolded"], seen["no l1"] = int((ok & info["folded"]).sum()), int((ok & ~info["folded"]).sum()), int((looked & ~info["ok"]).sum())
        seen["on a texel"] = int((ok & (info["wx"] == 0) & (info["wy"] == 0)).sum())
        raw = [(info[k] * F(n) - F(0.5)).astype(F) for k in ("u", "v")]  # fx and fy before the clamps
        clamped = (raw[0] < 0) | (raw[0] > n - 1) | (raw[1] < 0) | (raw[1] > n - 1)
        seen["clamped"] = int((ok & clamped).sum())
        if n > 1:
            seen["on an edge"] = int((ok & ~clamped & ((info["wx"] == 0.5) | (info["wy"] == 0.5))).sum())
        print(n, dict(seen))
        assert set(tc.KINDS) <= set(seen) and all(v >= tc.MIN_PER_RULE for v in seen.values()), (n, seen)
        # what each kind was planted for
        kind = lambda name: r["kind"] == tc.KINDS.index(name)  # noqa: E731
        assert not info["ok"][kind("zero") | kind("nan") | kind("inf") | kind("l1 overflows")].any()
        assert info["ok"][kind("subnormal") | kind("scaled 2^100") | kind("horizon -0")].all() and not info["folded"][kind("horizon -0")].any()
        corners = {(int(x), int(y)) for x, y in zip(info["x0"][kind("corner")], info["y0"][kind("corner")])}
        assert corners == {(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1)} or n == 1
        assert clamped[kind("border")].all() and clamped[kind("corner")].all()
        assert not info["wx"][kind("texel centre")].any() and not info["wy"][kind("texel centre")].any()
        assert np.all(np.isfinite(m.resolve(tc.texel_map(n), *m.from_map(r["m"], 1).T, r["tmax"], r["occluded"], (h, w), 8, 1, sums=r["sums"])[0]))
        assert np.signbit(r["sums"][..., 1]).sum() >= tc.MIN_PER_RULE
    codes = collections.Counter()
    for (w, h) in tc.SIZES:
        for batch in tc.BATCHES:
            r = tc.resolve_inputs(w, h, batch, 5)
            for v in tc.TMAX_CODES:
                hit = np.isnan(r["tmax"]) if v != v else bits(r["tmax"]) == bits(F(v))
                codes[str(v), "open"] += int((hit & (r["occluded"] == 0)).sum())
                codes[str(v), "occluded"] += int((hit & (r["occluded"] != 0)).sum())
    assert len(codes) == 2 * len(tc.TMAX_CODES) and all(v >= tc.MIN_PER_RULE for v in codes.values()), codes
    assert tc.SIZES == [(1, 1), (3, 2), (64, 16)] and tc.BATCHES == [1, 3, 8] and tc.MAPS == [1, 2, 5, 64] and tc.POLES == [0, 1, 2]
    for n in tc.MAPS:
        assert np.unique(tc.texel_map(n)[..., :3]).size == 3 * n * n and np.isnan(tc.texel_map(n)[..., 3]).all()


def test_the_end_to_end_case_holds_every_class(oracle):
    """on the oracle alone, at the case's own settings: at least 5 pixels without a counted sample, with every sample open and with open
    and occluded samples; at least 20 open rays in the upper and in the folded half of the map; nine different colour components"""
    e, c = tc.e2e(oracle, TEAPOT), tc.E2E
    got = {k: int(v.sum()) for k, v in tc.classes(e["sums"], e["rays"]).items()}
    halves = tc.open_rays_per_half(e["rays"], c["pole"])
    print(got, halves)
    assert set(got) == set(tc.E2E_CLASSES) and all(n >= tc.E2E_MIN_PER_CLASS for n in got.values()), got
    assert tc.E2E_MIN_PER_CLASS == 5 and tc.E2E_MIN_RAYS_PER_HALF == 20 and min(halves) >= tc.E2E_MIN_RAYS_PER_HALF, halves
    assert c["res"] == (24, 16) and c["samples"] == 8 and c["batch"] == 3 and c["map_size"] == 16
    assert len(set(c["zenith"] + c["horizon"] + c["ground"])) == 9
    hit = e["planes"]["position"][..., 3] > 0
    assert np.array_equal(e["sums"][..., 3] == c["samples"], hit) and np.all(e["sums"][..., 3][~hit] == 0)
    assert np.all(e["out"][..., 3] == hit) and np.all(np.isfinite(e["out"])) and np.all(e["out"][~hit] == 0)
    cls = tc.classes(e["sums"], e["rays"])
    assert e["out"][..., :3][cls["open"]].min() > 0 and e["rays"]["tmax"].shape == (c["samples"],) + hit.shape
    # the visibility of the same trace: the open share of the counted samples
    assert np.all(e["ao"][..., 0][cls["open"]] == 1) and np.all((e["ao"][..., 0][cls["mixed"]] > 0) & (e["ao"][..., 0][cls["mixed"]] < 1))
    assert np.array_equal(e["counts"][..., 1], e["sums"][..., 3])


@pytest.mark.parametrize("name", ["stage", "control"])
def test_the_stream_cases_poison_gives_another_result(oracle, name):
    """as tests/test_stream_cases_cpu.py: the model of the poison differs from the model of the true inputs in at least MIN_DIFFERENT
    words of every output, and so do the inputs"""
    case = tc.stream_stage(oracle, TEAPOT) if name == "stage" else tc.stream_control()
    true, poison = case.want("model", "true"), case.want("model", "poison")
    assert sorted(true) == sorted(poison) == ["out", "sums"]
    for k in true:
        assert stream_cases.differing(poison[k], true[k]) >= stream_cases.MIN_DIFFERENT, (name, k)
    for k in case.true:
        assert stream_cases.differing(case.poison[k], case.true[k]) >= stream_cases.MIN_DIFFERENT, (name, k)


# ---- the library, before its first HIP call --------------------------------------------------------------------------------------
LW, LH, LB, LN = 6, 5, 3, 4
NO_DEVICE = 1 << 20  # no such GPU: were a call accepted by mistake, the runtime would refuse the device and nothing would be launched
RES_ARGS = ("env", "dx", "dy", "dz", "tmax", "occluded", "sums", "out")
PLANE_BYTES, RAY_BYTES, MAP_BYTES = LH * LW * 16, LH * LW * LB * 4, LN * LN * 16
STRIDE = 2 * PLANE_BYTES  # buffer k of a call lies at byte offset k * STRIDE of one allocation (the largest buffer is a plane)


def _settings(**kw):
    v = dict(struct_size=C.sizeof(sky.SkySettings), width=LW, height=LH, flags=0, sample_count=8, sample_begin=2, batch=LB, map_size=LN, pole=1)
    v.update(kw)
    return sky.SkySettings(**v)


def test_struct_size_and_symbols():
    L = sky.lib()
    S = sky.SkySettings
    assert L.mpe_settings_size() == C.sizeof(S) == 36
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32]
    header = open(os.path.join(ROOT, "include", "minipath_sky.h")).read()
    body = header.split("#ifndef MINIPATH_SKY_H")[1]
    declared = set(re.findall(r"\b(mpe_[a-z_]+)\s*\(", body))
    assert declared == set(sky.SIGNATURES) and all(hasattr(L, n) for n in declared)
    assert "#define MPE_MAX_MAP 8192u" in body and sky.MPE_MAX_MAP == 8192 and "#define MPE_FLAG_ACCUMULATE 1u" in body
    assert mp.SkyLight is sky.SkyLight and mp.gradient_sky is sky.gradient_sky and {"SkyLight", "gradient_sky"} <= set(mp.__all__)
    assert L.mpe_check_settings(C.byref(_settings())) == 0
    assert L.mpe_check_settings(C.byref(_settings(flags=1, sample_count=65536, sample_begin=65281, width=1 << 20, height=1, batch=255,
                                                  map_size=8192, pole=0))) == 0
    assert L.mpe_check_settings(C.byref(_settings(width=1 << 15, height=1 << 15, batch=1, map_size=1, pole=2))) == 0  # 2^30 rays
    assert L.mpe_check_settings(C.byref(_settings(struct_size=1000))) == 0  # a later, larger struct: what is beyond is not read


def _buffers(names):
    # one allocation, so that "overlapping" can be asked for
    whole = np.full(len(names) * STRIDE // 4, SENTINEL, np.uint32)
    return whole, {k: whole.ctypes.data + i * STRIDE for i, k in enumerate(names)}


def _resolve(st, device=NO_DEVICE, **replace):
    whole, ptr = _buffers(RES_ARGS)
    for k, v in replace.items():
        ptr[k] = None if v is None else (ptr[v[0]] + v[1] if isinstance(v, tuple) else ptr[v])
    before = sky.last_kernels()
    rc = sky.lib().mpe_resolve(device, None if st is None else C.byref(st), *[ptr[k] for k in RES_ARGS], None)
    assert sky.last_kernels() == before  # nothing was launched
    assert np.all(whole == SENTINEL)     # nothing was written (host memory here: a launch would not even get this far)
    return rc


def _f3(c):
    return None if c is None else (C.c_float * 3)(*c)


def _gradient(n=LN, zenith=(1, 2, 3), horizon=(4, 5, 6), ground=(7, 8, 9), device=NO_DEVICE, env=0):
    whole = np.full(8192 * 4 // 4 + LN * LN * 4, SENTINEL, np.uint32)
    before = sky.last_kernels()
    rc = sky.lib().mpe_fill_gradient(device, n, _f3(zenith), _f3(horizon), _f3(ground), None if env is None else whole.ctypes.data + env, None)
    assert sky.last_kernels() == before and np.all(whole == SENTINEL)
    return rc


BAD_SETTINGS = [dict(width=0), dict(height=0), dict(width=0, height=0), dict(width=(1 << 20) + 1), dict(height=(1 << 20) + 1), dict(batch=0),
                dict(width=1 << 16, height=1 << 15, batch=1), dict(width=1 << 20, height=1 << 20, batch=1),
                dict(width=1 << 10, height=1 << 10, batch=2048, sample_count=65536, sample_begin=0), dict(batch=0xFFFFFFFF), dict(sample_begin=6),
                dict(sample_begin=0xFFFFFFFF), dict(sample_begin=0xFFFFFFFE, batch=3), dict(sample_count=0, sample_begin=0), dict(sample_count=65537),
                dict(sample_count=2), dict(map_size=0), dict(map_size=8193), dict(map_size=0xFFFFFFFF), dict(pole=3), dict(pole=0xFFFFFFFF),
                dict(flags=2), dict(flags=0x80000001), dict(struct_size=0), dict(struct_size=32), dict(struct_size=35)]
BAD_RESOLVE = ([{k: None} for k in RES_ARGS if k != "out"] + [dict(device=-1), dict(settings=None)]
               + [{o: i} for o in ("sums", "out") for i in ("env", "dx", "dy", "dz", "tmax", "occluded")] + [dict(out="sums")]   # an output equal to another buffer
               + [dict(sums=("tmax", RAY_BYTES - 16)), dict(out=("occluded", 16 * ((RAY_BYTES // 4 - 1) // 16))), dict(occluded=("sums", PLANE_BYTES - 1)),
                  dict(out=("sums", 16)), dict(tmax=("out", -RAY_BYTES + 4)), dict(dz=("sums", -RAY_BYTES + 4)), dict(env=("sums", -MAP_BYTES + 16)),
                  dict(sums=("env", MAP_BYTES - 16))]                                                                            # partial overlaps
               + [{k: (k, by)} for k in ("env", "sums", "out") for by in (4, 8, 12)]                                             # misaligned planes
               + [{k: (k, by)} for k in ("dx", "dy", "dz", "tmax") for by in (1, 2, 3)])                                         # misaligned ray arrays
BAD_GRADIENT = [dict(n=0), dict(n=8193), dict(n=0xFFFFFFFF), dict(device=-1), dict(zenith=None), dict(horizon=None), dict(ground=None), dict(env=None),
                dict(env=4), dict(env=8), dict(env=12)] + [{which: tuple(v if i == c else 1.0 for i in range(3))} for which in ("zenith", "horizon", "ground")
                                                           for c in range(3) for v in (NAN, INF, -INF)]


def _id(d):
    return ",".join(f"{k}={v}" for k, v in d.items())


@pytest.mark.parametrize("bad", BAD_SETTINGS, ids=_id)
def test_settings_are_refused(bad):
    assert _resolve(_settings(**bad)) == MP_ERR_INVALID
    assert sky.lib().mpe_last_error()
    assert sky.lib().mpe_check_settings(C.byref(_settings(**bad))) == MP_ERR_INVALID


@pytest.mark.parametrize("bad", BAD_RESOLVE, ids=_id)
def test_resolve_refuses_arguments(bad):
    bad = dict(bad)
    st = None if "settings" in bad and bad.pop("settings") is None else _settings()
    assert _resolve(st, **bad) == MP_ERR_INVALID
    assert sky.lib().mpe_last_error()


@pytest.mark.parametrize("bad", BAD_GRADIENT, ids=_id)
def test_fill_gradient_refuses_arguments(bad):
    assert _gradient(**bad) == MP_ERR_INVALID
    assert sky.lib().mpe_last_error()


def test_what_is_not_refused_gets_to_the_device():
    """the same calls with nothing wrong, and their legal variations, get as far as the device (which does not exist): MP_ERR_HIP"""
    assert sky.lib().mpe_check_settings(None) == MP_ERR_INVALID
    assert _resolve(_settings()) == MP_ERR_HIP
    assert _resolve(_settings(flags=1), out=None) == MP_ERR_HIP
    assert _resolve(_settings(pole=0, map_size=1)) == MP_ERR_HIP
    assert _resolve(_settings(), dy="dx", dz="dx") == MP_ERR_HIP                        # inputs may alias inputs
    assert _resolve(_settings(), occluded=("tmax", RAY_BYTES)) == MP_ERR_HIP            # adjacent is not overlapping
    assert _resolve(_settings(), out=("sums", PLANE_BYTES)) == MP_ERR_HIP
    assert _resolve(_settings(), occluded=("occluded", 3), tmax=("tmax", 4)) == MP_ERR_HIP  # bytes have no rule; an odd word is aligned
    assert _resolve(_settings(sample_begin=5)) == MP_ERR_HIP                            # the last samples of the pass
    assert _gradient() == MP_ERR_HIP
    assert _gradient(n=1, zenith=(-1, 0, 1e38), env=16) == MP_ERR_HIP


def test_last_kernels_buffer_protocol():
    L = sky.lib()
    need = C.c_size_t(99)
    assert L.mpe_last_kernels(None, 0, C.byref(need)) == 0 and need.value == len("\n".join(sky.last_kernels()))
    assert L.mpe_last_kernels(None, 4, None) == MP_ERR_INVALID and L.mpe_last_error() == b"NULL argument"
    buf = C.create_string_buffer(b"xxxx", 4)
    assert L.mpe_last_kernels(buf, 1, None) == 0 and buf.raw == b"\x00xxx"  # cap 1: the terminating 0 alone


def test_a_host_only_scene_raises():
    """a scene without a Context cannot be traced (as TriangleBvh.occluded says)"""
    host_scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT))
    with pytest.raises(mp.MinipathError):
        mp.SkyLight(host_scene, (8, 8))
    assert mp.SkyLight.eye_of(mp.Camera.teapot_view()) == [0.0, 2.0, 10.0]
    with pytest.raises(ValueError):
        mp.gradient_sky(4, (1, 1, 1), (1, 1, 1), (0, 0, 0), "cpu")
