"""CPU tests of the lights: the numpy model (tests/lights_model.py, the restatement of include/minipath_lights.h that the GPU tests
compare bits against) against a float64 restatement, against the geometry it stands for and against the oracle's RNG, the
conditions on the inputs of the GPU cases (tests/lights_cases.py), and what libminipath_lights.so decides before its first HIP call
-- every refusal, the struct sizes, the symbols -- through the built library without touching a GPU."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import lights as ll
from tests import lights_cases as tc, lights_model as m, secondary_model
from tests.conftest import ROOT, TEAPOT
from tests.lights_model import F, bits

MP_ERR_INVALID, MP_ERR_HIP = 1, 4
SENTINEL = 0x5A5A5A5A
INF, NAN = float("inf"), float("nan")
U = 2.0 ** -24  # the unit roundoff of binary32


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the model -----------------------------------------------------------------------------------------------------------------
LIGHTS64 = [((1.5, 2.0, -1.0), 0.0, (1.0, 2.0, 3.0)), ((-2.0, 0.5, 1.5), 0.4, (4.0, 0.0, 1.0)), ((0.25, 3.0, 0.5), 0.75, (1.0, 1.0, 1.0))]
SCALE = 4.0  # no coordinate of a point, a light or a disc sample's target exceeds it in magnitude


def _facing_planes(n_pixels, seed):
    """a row of hit pixels with random points, unit normals and alphas"""
    rng = np.random.default_rng(seed)
    alpha = rng.choice([1.0, 0.5, 0.375], n_pixels)
    pts = rng.uniform(-1, 1, (n_pixels, 3))
    nrm = rng.normal(0, 1, (n_pixels, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    position = np.concatenate([pts * alpha[:, None], alpha[:, None]], -1).astype(F)[None]
    normal = np.concatenate([nrm * alpha[:, None], alpha[:, None]], -1).astype(F)[None]
    return position, normal, pts, nrm


def _basis64(mv):
    sg = np.copysign(1.0, mv[..., 2])
    a = -1.0 / (sg + mv[..., 2])
    bb = mv[..., 0] * mv[..., 1] * a
    return (np.stack([1.0 + sg * mv[..., 0] * mv[..., 0] * a, sg * bb, -sg * mv[..., 0]], -1),
            np.stack([bb, sg + mv[..., 1] * mv[..., 1] * a, -mv[..., 1]], -1))


def test_the_model_against_float64(oracle):
    """1 500 pixels x 2 samples x 3 lights against the same formulas in float64 on the same float32 planes and the same disc samples.
    The bound counts roundings (U = 2^-24 each, relative to the magnitude of the operation's result, which no coordinate lets exceed
    SCALE = 4): the origin o = P + n * bias takes 3 roundings on top of n's 8 (l2: 5, sqrt, divide, and n * bias scaled by bias), at
    most 4 U SCALE per component; the target g of a sphere adds w = c - o (1), q2 and its root (6), m (1), the basis (at most 6 per
    component, on values of at most 2), u R and v R (1 each) and the three operations of the combination: below 24 roundings on
    values of at most SCALE, and d = g - o one more: |d - d64| <= 32 U SCALE per component.  len and tmax follow with 7 more roundings
    relative to len: |tmax - tmax64| <= 32 U SCALE + 8 U len.  n.d carries d's error (|n| = 1: 3 components) and 5 roundings of its
    own, so |nd - nd64| <= 3 * 32 U SCALE + 8 U len, and the weight nd / (dd len), whose divisor has 8 roundings and whose quotient
    one, differs by at most (96 U SCALE + 8 U len) / (dd len) + 16 U |weight|."""
    npx, B, eye, bias, margin = 1500, 2, np.array([0.5, 7.0, -3.0]), 1e-3, 0.125
    position, normal, _, _ = _facing_planes(npx, 15)
    g, info = m.generate(oracle, position, normal, LIGHTS64, 4321, B, 0, B, eye, bias=bias, margin=margin, want_info=True)
    assert np.all(info["pixel"] == m.P_LIVE) and 0.3 < info["flipped"].mean() < 0.7
    p64, n64 = position.astype(np.float64)[0], normal.astype(np.float64)[0]
    P = p64[:, :3] / p64[:, 3:]
    n = n64[:, :3] / np.linalg.norm(n64[:, :3], axis=-1, keepdims=True)
    n = np.where((np.einsum("ij,ij->i", P - eye.astype(F).astype(np.float64), n) > 0)[:, None], -n, n)
    o = P + n * np.float64(F(bias))
    table = m.table(LIGHTS64).astype(np.float64)
    got = {k: g[k].reshape(B, 3, npx) for k in m.RAY_ARRAYS}
    checked = 0
    for b in range(B):
        for l in range(3):
            c, R = table[l, :3], table[l, 3]
            w = c - o
            q = np.linalg.norm(w, axis=-1)
            target = np.broadcast_to(c, w.shape)
            if R > 0:
                t, bt = _basis64(w / q[:, None])
                uv = info["uv"][b, l, 0].astype(np.float64)
                target = c + (t * (uv[:, :1] * R) + bt * (uv[:, 1:] * R))
            d = target - o
            dd = np.einsum("ij,ij->i", d, d)
            ln = np.sqrt(dd)
            nd = np.einsum("ij,ij->i", n, d)
            lit = info["lit"][b, l, 0]
            # the two decide alike wherever float64 is not within the bound of a threshold
            clear = (np.abs(nd) > 200 * U * SCALE) & (np.abs(q - R) > 64 * U * SCALE) & (np.abs(ln - margin) > 64 * U * SCALE)
            lit64 = (q > R) & (nd > 0) & (ln - margin > 0)
            assert np.array_equal(lit[clear], lit64[clear]) and clear.mean() > 0.99
            k = lit & lit64
            checked += int(k.sum())
            for i, name in enumerate(("ox", "oy", "oz")):
                assert np.max(np.abs(got[name][b, l][k] - o[k, i])) <= 4 * U * SCALE
            for i, name in enumerate(("dx", "dy", "dz")):
                assert np.max(np.abs(got[name][b, l][k] - d[k, i])) <= 32 * U * SCALE
            assert np.all(np.abs(got["tmax"][b, l][k] - (ln[k] - margin)) <= 32 * U * SCALE + 8 * U * ln[k])
            w64 = nd[k] / (dd[k] * ln[k])
            assert np.all(np.abs(got["weight"][b, l][k] - w64) <= (96 * U * SCALE + 8 * U * ln[k]) / (dd[k] * ln[k]) + 16 * U * np.abs(w64))
            for name in m.RAY_ARRAYS:  # unlit rays: the code and zeros
                assert np.all(got[name][b, l][~lit] == (-1 if name == "tmax" else 0))
    assert checked > 0.3 * B * 3 * npx


def test_weight_is_the_cosine_over_the_squared_distance(oracle):
    """the geometry in float64, from the points and normals the planes were made of: a point light's ray ends at the light, its tmax
    is the distance less the margin and its weight cos(theta) / dist^2 with theta between the facing normal and the ray; a sphere
    light's target lies on the disc of radius R about its centre across the line to the surface, at R |(u, v)| from the centre"""
    npx, B, eye, bias, margin = 600, 2, np.array([0.5, 7.0, -3.0]), 1e-3, 0.125
    position, normal, pts, nrm = _facing_planes(npx, 16)
    g, info = m.generate(oracle, position, normal, LIGHTS64, 99, B, 0, B, eye, bias=bias, margin=margin, want_info=True)
    facing = np.where((np.einsum("ij,ij->i", pts - eye, nrm) > 0)[:, None], -nrm, nrm)
    o = pts + facing * bias
    got = {k: g[k].reshape(B, 3, npx).astype(np.float64) for k in m.RAY_ARRAYS}
    for b in range(B):
        for l, (c, R, _) in enumerate(LIGHTS64):
            lit = info["lit"][b, l, 0]
            assert lit.sum() > npx // 5
            d = np.stack([got["dx"][b, l], got["dy"][b, l], got["dz"][b, l]], -1)[lit]
            dist = np.linalg.norm(d, axis=-1)
            cos = np.einsum("ij,ij->i", facing[lit], d) / dist
            assert np.all(cos > 0) and np.max(np.abs(got["weight"][b, l][lit] - cos / dist ** 2) * dist ** 2) <= 1e-5
            assert np.max(np.abs(got["tmax"][b, l][lit] - (dist - margin))) <= 1e-5
            off = o[lit] + d - np.array(c)  # the target less the centre
            if R == 0:
                assert np.max(np.abs(off)) <= 1e-5
            else:
                axis = (np.array(c) - o[lit]) / np.linalg.norm(np.array(c) - o[lit], axis=-1, keepdims=True)
                uv = info["uv"][b, l, 0].astype(np.float64)[lit]
                assert np.max(np.abs(np.einsum("ij,ij->i", off, axis))) <= 1e-5
                assert np.max(np.abs(np.linalg.norm(off, axis=-1) - R * np.linalg.norm(uv, axis=-1))) <= 1e-5


def test_draws_are_made_for_sphere_lights_alone(oracle):
    """in the mixed table the only sphere is the middle light: its disc sample is the FIRST draw of the stream of the key (what
    mps_generate draws for the same seed), the point lights draw nothing, and moving a point light leaves the sample and the rays of
    the other lights as they were; among eight spheres the second light has the second draw"""
    w, h = 5, 3
    position, normal, _, _ = _facing_planes(w * h, 17)
    position, normal = position.reshape(h, w, 4), normal.reshape(h, w, 4)
    kw = dict(seed=0xDEADBEEFCAFE, sample_count=8, sample_begin=5, batch=3, eye=(0, 0, 50), bias=tc.BIAS, margin=0.0)
    mixed = tc.TABLES["mixed"]
    g, info = m.generate(oracle, position, normal, mixed, want_info=True, **kw)
    moved = [((0.5, 0.5, 1.5), 0.0, mixed[0][2])] + mixed[1:]
    g2, info2 = m.generate(oracle, position, normal, moved, want_info=True, **kw)
    _, info8 = m.generate(oracle, position, normal, tc.TABLES["spheres"], want_info=True, **kw)
    assert _same(info["uv"], info2["uv"]) and not info["uv"][:, 0].any() and not info["uv"][:, 2].any()
    n = w * h
    for k in m.RAY_ARRAYS:
        a, a2 = g[k].reshape(3, 3, n), g2[k].reshape(3, 3, n)
        assert _same(a[:, 1:], a2[:, 1:]), k
    assert not _same(g["dx"].reshape(3, 3, n)[:, 0], g2["dx"].reshape(3, 3, n)[:, 0])
    for b in range(3):
        for y in range(h):
            for x in range(w):
                _, first = secondary_model.disc_sample(oracle, kw["seed"], w, 8, x, y, 5 + b)
                two = m.disc_samples(oracle, kw["seed"], w, 8, x, y, 5 + b, 2)
                assert _same(info["uv"][b, 1, y, x], first) and _same(two[0], first)
                assert _same(info8["uv"][b, 0, y, x], first) and _same(info8["uv"][b, 1, y, x], two[1]) and not _same(two[0], two[1])


def test_batches_do_not_change_the_result(oracle):
    """8 samples in one batch equal 3 + 3 + 2, rays and sums, bit for bit, on a synthetic plane set with a random occluder"""
    c = tc.synthetic(37, 23)
    lights = tc.TABLES["mixed"]
    kw = dict(bias=tc.BIAS, margin=tc.MARGIN)
    pixels, L = 37 * 23, len(lights)
    whole = m.generate(oracle, c["position"], c["normal"], lights, 5, 8, 0, 8, tc.EYE, **kw)
    parts = [m.generate(oracle, c["position"], c["normal"], lights, 5, 8, b0, n, tc.EYE, **kw) for b0, n in ((0, 3), (3, 3), (6, 2))]
    for k in m.RAY_ARRAYS:
        assert _same(whole[k], np.concatenate([p[k] for p in parts])), k
    assert whole["tmax"].size == 8 * L * pixels

    def occluder(o, d, tmax):  # a function of the ray alone
        return ((bits(d[:, 0]) ^ bits(o[:, 1])) >> 3) & 1

    a = m.run(oracle, occluder, c["position"], c["normal"], lights, 5, 8, 8, tc.EYE, **kw)
    b = m.run(oracle, occluder, c["position"], c["normal"], lights, 5, 8, 3, tc.EYE, **kw)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    free = m.run(oracle, lambda o, d, t: np.zeros(len(t), np.uint8), c["position"], c["normal"], lights, 5, 8, 8, tc.EYE, **kw)
    assert 0 < a[1][..., :3].sum() < free[1][..., :3].sum()


def test_resolve_sums_by_the_codes():
    """one pixel, two lights, every tmax code with both answers: a sample is counted by its first ray alone (tmax > 0 or -1), a ray
    adds intensity * weight only when it was traced and not occluded"""
    lights = [((0, 0, 0), 0.0, (1.0, 2.0, 4.0)), ((1, 0, 0), 0.0, (8.0, 0.0, 0.5))]
    #        sample 0     1            2           3          4           5
    tmax = np.array([0.5, 0.5,  -1.0, 2.0,   0.0, 0.5,   NAN, 0.5,   INF, -1.0,   -2.0, -0.0], F)
    wt = np.array([0.25, 1.0,   9.0, 0.5,    9.0, 2.0,   9.0, 4.0,   1.0, 9.0,    9.0, 9.0], F)
    occ = np.array([0, 1,       0, 0,        0, 0,       0, 7,       0, 0,        0, 0], np.uint8)
    sums, out = m.resolve(tmax, wt, occ, lights, (1, 1), 6)
    # counted: samples 0, 1, 4.  light 0 seen in 0 (0.25) and 4 (1.0); light 1 seen in 1 (0.5) and 2 (2.0: the sample is not counted,
    # the ray is: only a caller's own buffers can say so, mpl_generate makes a pixel's first rays none together)
    assert sums[0, 0].tolist() == [1.25 + 8 * 2.5, 2.5, 5.0 + 0.5 * 2.5, 3.0]
    assert _same(out[0, 0], np.array([F(21.25) / F(3), F(2.5) / F(3), F(6.25) / F(3), 1], F))
    more, _ = m.resolve(tmax, wt, occ, lights, (1, 1), 6, sums=np.array([[[1.0, 1.0, 1.0, 5.0]]], F))
    assert more[0, 0].tolist() == [22.25, 3.5, 7.25, 8.0]
    none, out3 = m.resolve(tmax[4:6], wt[4:6], occ[4:6], lights, (1, 1), 1)
    assert none[0, 0].tolist() == [16.0, 0.0, 1.0, 0.0] and out3[0, 0].tolist() == [0, 0, 0, 0]  # nothing counted: alpha 0, black
    assert m.resolve(tmax, wt, occ, lights, (1, 1), 6, want_out=False)[1] is None


# ---- the inputs of the GPU cases -------------------------------------------------------------------------------------------------
def test_the_synthetic_cases_reach_every_rule(oracle):
    """over the sizes and the tables of the GPU test, at least tc.MIN_PER_RULE pixels each: a miss, a NaN and a negative alpha, a zero
    and a NaN normal, normals that flip and that do not, a light behind the surface, a point inside a sphere light, a point at the
    light (dd == 0), a ray no longer than the margin, a light grazing at a subnormal cosine term; and every table has lit rays"""
    seen = collections.Counter()
    for w, h in tc.SIZES:
        c = tc.synthetic(w, h)
        A, N = c["position"][..., 3], c["normal"][..., :3]
        seen["miss"] += int((A == 0).sum())
        seen["nan alpha"] += int(np.isnan(A).sum())
        seen["negative alpha"] += int((A < 0).sum())
        seen["zero normal"] += int(((A > 0) & ~N.any(-1)).sum())
        seen["nan normal"] += int(((A > 0) & np.isnan(N).any(-1)).sum())
        for name in tc.TABLES:
            g, info = tc.generated(oracle, w, h, name, 1, 0)
            live = info["pixel"] == m.P_LIVE
            assert np.array_equal(info["pixel"] == m.P_NONE_ALPHA, ~(A > 0)) and np.array_equal(info["pixel"] == m.P_NONE_NORMAL, (A > 0) & ~(m.dot(N, N) > 0))
            if name == "point":
                seen["flipped"] += int((live & info["flipped"]).sum())
                seen["kept"] += int((live & ~info["flipped"]).sum())
            any_light = lambda k: info[k][0].any(0)  # noqa: E731  (pixels where the rule holds for some light)
            seen[name + ": behind"] += int((info["behind"][0] & ~info["at"][0]).any(0).sum())
            seen[name + ": lit"] += int(any_light("lit").sum())
            seen["inside a sphere"] += int(any_light("inside").sum())
            seen["at the light"] += int(any_light("at").sum())
            seen["within the margin"] += int(any_light("short").sum())
            seen["grazing, subnormal"] += int(any_light("grazing").sum())
            tm = g["tmax"].reshape(-1, h, w)
            assert np.all((tm[:, ~live] == 0)) and np.all(tm[:, live] != 0)
    print(dict(seen))
    assert len(seen) == 17 and all(n >= tc.MIN_PER_RULE for n in seen.values()), seen
    assert tc.synthetic(1, 1)["kind"][0, 0] == 0 and tc.generated(oracle, 1, 1, "point", 1, 0)[1]["pixel"][0, 0] == m.P_LIVE
    radii = {k: [lt[1] for lt in v] for k, v in tc.TABLES.items()}
    assert radii["point"] == [0.0] and [r > 0 for r in radii["mixed"]] == [False, True, False] and all(r > 0 for r in radii["spheres"])
    assert len(radii["spheres"]) == ll.MPL_MAX_LIGHTS
    # the planted pixels do what they were planted for, with the light they were planted for
    _, info = tc.generated(oracle, 64, 16, "mixed", 1, 0)
    kind = tc.synthetic(64, 16)["kind"]
    assert np.all(info["at"][0, 0][kind == 6]) and np.all(info["inside"][0, 1][kind == 7]) and np.all(info["short"][0, 0][kind == 8])
    assert np.all((info["grazing"] | info["short"])[0, 0][kind == 9]) and info["grazing"][0, 0][kind == 9].mean() > 0.75  # (some lie within the margin)
    r = tc.resolve_inputs(37, 23, 3, "mixed")
    assert all((bits(r["tmax"]) == bits(F(v))).sum() >= tc.MIN_PER_RULE for v in tc.TMAX_CODES if v == v) and np.isnan(r["tmax"]).sum() >= tc.MIN_PER_RULE
    assert np.all(np.isfinite(r["weight"])) and (r["weight"] == 0).sum() >= 16 and ((r["weight"] > 0) & (r["weight"] < 2.0 ** -126)).sum() >= 16


def test_the_end_to_end_case_holds_every_class(oracle):
    """on the oracle alone, at the case's own settings, at least 8 pixels each: a miss; lit and fully visible; lit and fully
    shadowed; partly shadowed by the sphere light; facing away from both lights"""
    e = tc.e2e(oracle, TEAPOT)
    got = {k: int(v.sum()) for k, v in tc.classes(e["sums"], e["rays"]).items()}
    print(got)
    assert set(got) == set(tc.E2E_CLASSES) and all(n >= tc.E2E_MIN_PER_CLASS for n in got.values()), got
    radii = [lt[1] for lt in tc.E2E["lights"]]
    assert radii[0] == 0 and radii[1] > 0
    hit = e["planes"]["position"][..., 3] > 0
    assert np.array_equal(e["sums"][..., 3] == tc.E2E["samples"], hit) and np.all(e["sums"][..., 3][~hit] == 0)
    assert np.all(e["out"][..., 3] == hit) and np.all(np.isfinite(e["out"])) and np.all(e["out"][~hit] == 0)
    away = tc.classes(e["sums"], e["rays"])["away"]
    assert not e["sums"][..., :3][away].any() and e["out"][..., :3][tc.classes(e["sums"], e["rays"])["visible"]].min() > 0
    assert e["rays"]["tmax"].shape == (tc.E2E["samples"], 2) + hit.shape


# ---- the library, before its first HIP call --------------------------------------------------------------------------------------
LW, LH, LB, LL = 6, 5, 3, 2
NO_DEVICE = 1 << 20  # no such GPU: were a call accepted by mistake, the runtime would refuse the device and nothing would be launched
GEN_ARGS = ("position", "normal") + m.RAY_ARRAYS
RES_ARGS = ("tmax", "weight", "occluded", "sums", "out")
PLANE_BYTES, RAY_BYTES = LH * LW * 16, LH * LW * LB * LL * 4
STRIDE = 2 * RAY_BYTES  # buffer k of a call lies at byte offset k * STRIDE of one allocation (a plane is smaller than a ray array)
GOOD_LIGHTS = [((0.0, 1.0, 2.0), 0.0, (1.0, 1.0, 1.0)), ((3.0, -1.0, 0.5), 0.25, (0.0, 2.0, 0.0))]


def _settings(**kw):
    v = dict(struct_size=C.sizeof(ll.LightsSettings), width=LW, height=LH, flags=0, sample_count=8, sample_begin=2, batch=LB, light_count=LL,
             seed=1, bias=1e-4, margin=0.0)
    eye = kw.pop("eye", (0.0, 0.0, 5.0))
    v.update(kw)
    st = ll.LightsSettings(**v)
    st.eye[:] = eye
    return st


def _lights(change=None, count=LL):
    """the good table, extended with copies of its last light to `count`, with the fields of `change` ({(light, field): value}) set"""
    t = (ll.Light * max(count, 1))()
    for i in range(max(count, 1)):
        p, r, it = GOOD_LIGHTS[min(i, len(GOOD_LIGHTS) - 1)]
        t[i].position[:], t[i].radius, t[i].intensity[:] = p, r, it
    for (i, field), value in (change or {}).items():
        if field in ("radius", "reserved"):
            setattr(t[i], field, value)
        else:
            getattr(t[i], field[0])[field[1]] = value
    return t


def test_struct_sizes_and_symbols():
    L = ll.lib()
    S, T = ll.LightsSettings, ll.Light
    assert L.mpl_settings_size() == C.sizeof(S) == 64 and C.sizeof(T) == 32
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 52, 56]
    assert [getattr(T, f).offset for f, _ in T._fields_] == [0, 12, 16, 28]
    header = open(os.path.join(ROOT, "include", "minipath_lights.h")).read()
    body = header.split("#ifndef MINIPATH_LIGHTS_H")[1]
    declared = set(re.findall(r"\b(mpl_[a-z_]+)\s*\(", body))
    assert declared == set(ll.SIGNATURES) and all(hasattr(L, n) for n in declared)
    assert "#define MPL_MAX_LIGHTS 8u" in body and ll.MPL_MAX_LIGHTS == 8 and "#define MPL_FLAG_ACCUMULATE 1u" in body
    assert mp.LocalLights is ll.LocalLights and "LocalLights" in mp.__all__
    assert L.mpl_check_settings(C.byref(_settings()), _lights()) == 0
    assert L.mpl_check_settings(C.byref(_settings(struct_size=60, flags=1, bias=0.0, margin=3.0, sample_count=65536, sample_begin=65281,
                                                  width=1 << 20, height=1, batch=255, light_count=8)), _lights(count=8)) == 0
    assert L.mpl_check_settings(C.byref(_settings(width=1 << 15, height=1 << 14, batch=1, light_count=3)), _lights(count=3)) == 0  # 1.5 * 2^30 rays
    # lights beyond light_count are not read
    assert L.mpl_check_settings(C.byref(_settings(light_count=1)), _lights({(1, "radius"): NAN})) == 0


def test_the_wrappers_light_table():
    t = ll.light_table(GOOD_LIGHTS)
    assert len(t) == 2 and list(t[1].position) == [3.0, -1.0, 0.5] and t[1].radius == 0.25 and list(t[1].intensity) == [0.0, 2.0, 0.0] and t[1].reserved == 0
    t8 = ll.light_table(np.arange(24, dtype=np.float32).reshape(3, 8))
    assert len(t8) == 3 and list(t8[2].position) == [16, 17, 18] and t8[2].radius == 19 and list(t8[2].intensity) == [20, 21, 22] and t8[2].reserved == 23
    assert np.array_equal(m.table(GOOD_LIGHTS), np.frombuffer(t, np.float32).reshape(2, 8))
    for bad in ([], [GOOD_LIGHTS[0]] * 9, [(1, 2, 3, 4)], [((0, 0), 0.0, (1, 1, 1))]):
        with pytest.raises(ValueError):
            ll.light_table(bad)


def _buffers(names):
    # one allocation, so that "overlapping" can be asked for
    whole = np.full(len(names) * STRIDE // 4, SENTINEL, np.uint32)
    return whole, {k: whole.ctypes.data + i * STRIDE for i, k in enumerate(names)}


def _call(fn_name, names, st, device=NO_DEVICE, lights="good", **replace):
    whole, ptr = _buffers(names)
    for k, v in replace.items():
        ptr[k] = None if v is None else (ptr[v[0]] + v[1] if isinstance(v, tuple) else ptr[v])
    table = _lights(count=st.light_count if st is not None and 0 < st.light_count <= 8 else LL) if isinstance(lights, str) else lights
    before = ll.last_kernels()
    rc = getattr(ll.lib(), fn_name)(device, None if st is None else C.byref(st), table, *[ptr[k] for k in names], None)
    assert ll.last_kernels() == before  # nothing was launched
    assert np.all(whole == SENTINEL)    # nothing was written (host memory here: a launch would not even get this far)
    return rc


def _generate(st, **kw):
    return _call("mpl_generate", GEN_ARGS, st, **kw)


def _resolve(st, **kw):
    return _call("mpl_resolve", RES_ARGS, st, **kw)


BAD_SETTINGS = [dict(width=0), dict(height=0), dict(width=0, height=0), dict(width=(1 << 20) + 1), dict(height=(1 << 20) + 1), dict(batch=0),
                dict(width=1 << 16, height=1 << 15, batch=1, light_count=1), dict(width=1 << 20, height=1 << 20, batch=1),
                dict(width=1 << 10, height=1 << 10, batch=2048, sample_count=65536, light_count=1),
                dict(width=1 << 10, height=1 << 10, batch=256, sample_count=65536, light_count=8),   # only the lights take it to 2^31
                dict(width=1 << 15, height=1 << 14, batch=1, light_count=4), dict(batch=0xFFFFFFFF), dict(sample_begin=6),
                dict(sample_begin=0xFFFFFFFF), dict(sample_begin=0xFFFFFFFE, batch=3), dict(sample_count=0, sample_begin=0), dict(sample_count=65537),
                dict(sample_count=2), dict(light_count=0), dict(light_count=9), dict(light_count=0xFFFFFFFF), dict(flags=2), dict(flags=0x80000001),
                dict(bias=-1e-4), dict(bias=NAN), dict(bias=INF), dict(margin=-0.1), dict(margin=NAN), dict(margin=INF), dict(eye=(NAN, 0, 0)),
                dict(eye=(0, INF, 0)), dict(eye=(0, 0, -INF)), dict(struct_size=0), dict(struct_size=56), dict(struct_size=59)]
BAD_LIGHTS = ([{(i, ("position", c)): v} for i in (0, 1) for c in range(3) for v in (NAN, INF, -INF)]
              + [{(i, ("intensity", c)): v} for i in (0, 1) for c in range(3) for v in (NAN, INF, -1.0)]
              + [{(i, "radius"): v} for i in (0, 1) for v in (NAN, INF, -0.5)] + [{(i, "reserved"): v} for i in (0, 1) for v in (NAN, 1.0, -1e-30)])
BAD_GENERATE = ([{k: None} for k in GEN_ARGS] + [dict(device=-1), dict(settings=None), dict(lights=None)]
                + [{o: i} for o in m.RAY_ARRAYS for i in ("position", "normal")]               # a ray array equal to a plane
                + [dict(oy="ox"), dict(tmax="dz"), dict(dx="oz"), dict(weight="tmax"), dict(weight="ox")]   # two ray arrays the same
                + [dict(ox=("position", PLANE_BYTES - 4)), dict(position=("ox", RAY_BYTES - 4)), dict(oy=("ox", 4)), dict(tmax=("normal", -RAY_BYTES + 4)),
                   dict(normal=("dz", -PLANE_BYTES + 16)), dict(weight=("tmax", RAY_BYTES - 4))])  # partial overlaps
BAD_RESOLVE = ([{k: None} for k in RES_ARGS if k != "out"] + [dict(device=-1), dict(settings=None), dict(lights=None)]
               + [dict(sums="tmax"), dict(sums="weight"), dict(sums="occluded"), dict(out="tmax"), dict(out="weight"), dict(out="occluded"), dict(out="sums"),
                  dict(sums=("tmax", RAY_BYTES - 4)), dict(out=("occluded", RAY_BYTES // 4 - 1)), dict(occluded=("sums", PLANE_BYTES - 1)),
                  dict(out=("sums", 16)), dict(tmax=("out", -RAY_BYTES + 4)), dict(weight=("sums", -RAY_BYTES + 4))])


def _id(d):
    return ",".join(f"{k}={v}" for k, v in d.items())


@pytest.mark.parametrize("bad", BAD_SETTINGS, ids=_id)
def test_settings_are_refused(bad):
    st = _settings(**bad)
    for call in (_generate, _resolve):
        assert call(_settings(**bad)) == MP_ERR_INVALID
        assert ll.lib().mpl_last_error()
    assert ll.lib().mpl_check_settings(C.byref(st), _lights(count=8)) == MP_ERR_INVALID


@pytest.mark.parametrize("bad", BAD_LIGHTS, ids=_id)
def test_lights_are_refused(bad):
    for call in (_generate, _resolve):
        assert call(_settings(), lights=_lights(bad)) == MP_ERR_INVALID
        assert ll.lib().mpl_last_error().startswith(b"a light's")
    assert ll.lib().mpl_check_settings(C.byref(_settings()), _lights(bad)) == MP_ERR_INVALID


@pytest.mark.parametrize("bad", BAD_GENERATE, ids=_id)
def test_generate_refuses_arguments(bad):
    bad = dict(bad)
    st = None if "settings" in bad and bad.pop("settings") is None else _settings()
    assert _generate(st, **bad) == MP_ERR_INVALID
    assert ll.lib().mpl_last_error()


@pytest.mark.parametrize("bad", BAD_RESOLVE, ids=_id)
def test_resolve_refuses_arguments(bad):
    bad = dict(bad)
    st = None if "settings" in bad and bad.pop("settings") is None else _settings()
    assert _resolve(st, **bad) == MP_ERR_INVALID
    assert ll.lib().mpl_last_error()


def test_what_is_not_refused_gets_to_the_device():
    """the same calls with nothing wrong, and their legal variations, get as far as the device (which does not exist): MP_ERR_HIP"""
    assert ll.lib().mpl_check_settings(None, _lights()) == MP_ERR_INVALID
    assert ll.lib().mpl_check_settings(C.byref(_settings()), None) == MP_ERR_INVALID
    assert _generate(_settings()) == MP_ERR_HIP
    assert _generate(_settings(), lights=_lights({(1, "radius"): 0.0})) == MP_ERR_HIP                # point lights alone
    assert _generate(_settings(margin=2.5, bias=0.0)) == MP_ERR_HIP
    assert _generate(_settings(), lights=_lights({(0, ("intensity", 1)): 0.0, (0, "reserved"): -0.0})) == MP_ERR_HIP
    assert _generate(_settings(), normal="position") == MP_ERR_HIP                                # inputs may alias inputs
    assert _generate(_settings(), ox=("position", PLANE_BYTES)) == MP_ERR_HIP                     # adjacent is not overlapping
    assert _generate(_settings(), weight=("tmax", RAY_BYTES)) == MP_ERR_HIP
    assert _generate(_settings(sample_begin=5)) == MP_ERR_HIP                                     # the last samples of the pass
    assert _resolve(_settings()) == MP_ERR_HIP
    assert _resolve(_settings(flags=1), out=None) == MP_ERR_HIP
    assert _resolve(_settings(), occluded=("tmax", RAY_BYTES)) == MP_ERR_HIP
    assert _resolve(_settings(), weight="tmax") == MP_ERR_HIP


def test_last_kernels_buffer_protocol():
    L = ll.lib()
    need = C.c_size_t(99)
    assert L.mpl_last_kernels(None, 0, C.byref(need)) == 0 and need.value == len("\n".join(ll.last_kernels()))
    assert L.mpl_last_kernels(None, 4, None) == MP_ERR_INVALID and L.mpl_last_error() == b"NULL argument"
    buf = C.create_string_buffer(b"xxxx", 4)
    assert L.mpl_last_kernels(buf, 1, None) == 0 and buf.raw == b"\x00xxx"  # cap 1: the terminating 0 alone


def test_a_host_only_scene_raises():
    """a scene without a Context cannot be traced (as TriangleBvh.occluded says)"""
    host_scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT))
    with pytest.raises(mp.MinipathError):
        mp.LocalLights(host_scene, (8, 8))
    assert mp.LocalLights.eye_of(mp.Camera.teapot_view()) == [0.0, 2.0, 10.0]
