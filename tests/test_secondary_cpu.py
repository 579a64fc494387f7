"""CPU tests of the secondary rays: the numpy model (tests/secondary_model.py, the restatement of include/minipath_secondary.h that
the GPU tests compare bits against) against a float64 restatement and against the oracle's RNG, the conditions on the inputs of the
GPU cases (tests/secondary_cases.py), and what libminipath_secondary.so decides before its first HIP call -- every refusal, the
struct size, the symbols -- through the built library without touching a GPU."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import secondary as sv
from tests import secondary_cases as tc, secondary_model as m
from tests.conftest import ROOT, TEAPOT
from tests.secondary_model import F, bits

MP_ERR_INVALID, MP_ERR_HIP = 1, 4
SENTINEL = 0x5A5A5A5A
INF, NAN = float("inf"), float("nan")


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _facing_planes(n_pixels, seed):
    """a row of hit pixels with random points, unit normals and alphas, seen from a far eye"""
    rng = np.random.default_rng(seed)
    alpha = rng.choice([1.0, 0.5, 0.375], n_pixels)
    pts = rng.uniform(-1, 1, (n_pixels, 3))
    nrm = rng.normal(0, 1, (n_pixels, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    position = np.concatenate([pts * alpha[:, None], alpha[:, None]], -1).astype(F)[None]
    normal = np.concatenate([nrm * alpha[:, None], alpha[:, None]], -1).astype(F)[None]
    return position, normal, pts, nrm


def test_ao_directions_are_a_cosine_law_about_the_facing_normal(oracle):
    """20 000 rays (2 500 pixels x 8 samples) against float64: the direction is a unit vector within 1e-6, lies in the hemisphere of
    the normal turned towards the eye, is the float64 basis' combination of the same disc sample, and its cosine to the normal
    averages 2/3 (sd of one cosine: sqrt(1/2 - 4/9) = 0.2357, so 5 sigma of the mean of 20 000 is 0.0083); the origin is the point
    moved by bias along that normal"""
    npx, B, eye, bias = 2500, 8, np.array([0.5, 7.0, -3.0]), 1e-3
    position, normal, pts, nrm = _facing_planes(npx, 5)
    g, info = m.generate(oracle, position, normal, m.MODE_AO, 1234, B, 0, B, eye, radius=2.0, bias=bias, want_info=True)
    assert np.all(info["pixel"] == m.P_LIVE)
    o, d, tmax = (a.astype(np.float64) for a in m.rays_of(g))
    facing = np.where((np.einsum("ij,ij->i", pts - eye, nrm) > 0)[:, None], -nrm, nrm)
    assert 0.3 < info["flipped"].mean() < 0.7 and np.array_equal(info["flipped"][0], np.einsum("ij,ij->i", pts - eye, nrm) > 0)
    fn = np.tile(facing, (B, 1))
    assert np.max(np.abs(np.linalg.norm(d, axis=-1) - 1)) <= 1e-6
    cos = np.einsum("ij,ij->i", d, fn)
    assert np.all(cos > -1e-6) and abs(cos.mean() - 2 / 3) <= 0.0083, cos.mean()
    assert np.max(np.abs(o - np.tile(pts + facing * bias, (B, 1)))) <= 1e-6 and np.all(tmax == 2.0)
    # the tangent part is the disc sample in an orthonormal basis: |d - n cos|^2 = u^2 + v^2, in float64 from the model's own (u, v)
    uv = info["uv"].reshape(-1, 2).astype(np.float64)
    assert np.max(np.abs(np.sum((d - fn * cos[:, None]) ** 2, -1) - np.sum(uv ** 2, -1))) <= 1e-5
    assert np.max(np.abs(cos - np.sqrt(np.maximum(1 - np.sum(uv ** 2, -1), 0)))) <= 2e-3  # sqrt near 0 amplifies the rounding of u, v


def test_sun_directions_against_float64(oracle):
    """lit pixels: d - L lies in the plane across L, with length spread * |(u, v)|; unlit pixels carry the code -1 and zeros"""
    npx, B, eye = 400, 4, np.array([0.0, 0.0, 9.0])
    position, normal, pts, nrm = _facing_planes(npx, 6)
    L = np.array([0.48, 0.6, -0.64])
    g, info = m.generate(oracle, position, normal, m.MODE_SUN, 99, B, 0, B, eye, light=L, spread=0.1, radius=INF, bias=0.0, want_info=True)
    o, d, tmax = (a.astype(np.float64) for a in m.rays_of(g))
    facing = np.where((np.einsum("ij,ij->i", pts - eye, nrm) > 0)[:, None], -nrm, nrm)
    lit = np.tile(facing @ L > 0, B)
    assert 0.2 < lit.mean() < 0.8 and np.array_equal(np.tile(info["pixel"][0] == m.P_LIVE, B), lit)
    assert np.all(tmax[lit] == INF) and np.all(tmax[~lit] == -1) and not o[~lit].any() and not d[~lit].any()
    off = d[lit] - L
    uv = info["uv"].reshape(-1, 2).astype(np.float64)[lit]
    assert np.max(np.abs(off @ L)) <= 1e-6 and np.max(np.abs(np.linalg.norm(off, axis=-1) - 0.1 * np.linalg.norm(uv, axis=-1))) <= 1e-6
    assert np.max(np.abs(o[lit] - np.tile(pts, (B, 1))[lit])) <= 1e-6


def test_the_disc_sample_is_the_oracles_draw_for_the_key(oracle):
    """(u, v) of sample s of pixel (x, y) is the first UnitDisc draw of the stream seeded with mix(seed) + ((y W + x) spp + s), and
    that is where the path extension's first bounce would draw it were the camera ray not drawn before"""
    L = oracle.lib()
    w, spp, seed = 5, 8, 0xDEADBEEFCAFE
    position, normal, _, _ = _facing_planes(w * 2, 7)
    position, normal = position.reshape(2, w, 4), normal.reshape(2, w, 4)
    _, info = m.generate(oracle, position, normal, m.MODE_AO, seed, spp, 5, 3, (0, 0, 50), want_info=True)
    for b in range(3):
        for y in range(2):
            for x in range(w):
                key = (L.mpo_seed_mix(C.c_uint64(seed)) + ((y * w + x) * spp + 5 + b)) & 0xFFFFFFFFFFFFFFFF
                assert key == L.mpo_sample_key(C.c_uint64(seed), w, spp, x, y, 5 + b)
                rng = oracle.Rng()
                L.mpo_rng_seed(C.byref(rng), C.c_uint64(key))
                want = np.zeros(2, F)
                L.mpo_rng_unit_disc(C.byref(rng), oracle._f32p(want))
                assert _same(info["uv"][b, y, x], want) and want[0] * want[0] + want[1] * want[1] <= 1


def test_batches_do_not_change_the_result(oracle):
    """8 samples in one batch equal 3 + 3 + 2, rays and counts, on a synthetic plane set with a random occluder"""
    c = tc.synthetic(37, 23)
    kw = dict(tc.MODES["ao"])
    mode = kw.pop("mode")
    whole = m.generate(oracle, c["position"], c["normal"], mode, 5, 8, 0, 8, tc.EYE, **kw)
    parts = [m.generate(oracle, c["position"], c["normal"], mode, 5, 8, b0, n, tc.EYE, **kw) for b0, n in ((0, 3), (3, 3), (6, 2))]
    for k in m.RAY_ARRAYS:
        assert _same(whole[k], np.concatenate([p[k] for p in parts])), k

    def occluder(o, d, tmax):  # a function of the ray alone
        return ((bits(d[:, 0]) ^ bits(o[:, 1])) >> 3) & 1

    a = m.run(oracle, occluder, c["position"], c["normal"], mode, 5, 8, 8, tc.EYE, **kw)
    b = m.run(oracle, occluder, c["position"], c["normal"], mode, 5, 8, 3, tc.EYE, **kw)
    assert _same(a[0], b[0]) and _same(a[1], b[1]) and 0 < a[1][..., 0].sum() < a[1][..., 1].sum()


def test_resolve_counts_by_the_codes():
    """one pixel, every tmax code with both answers: only tmax > 0 and -1 are counted, only unoccluded traced rays are visible"""
    tmax = np.array([0.0, 0.0, -1.0, -1.0, -0.0, 0.5, 0.5, INF, INF, NAN, NAN, -2.0], F)
    occ = np.array([0, 1, 0, 1, 0, 0, 1, 0, 7, 0, 1, 0], np.uint8)
    counts, out = m.resolve(tmax, occ, (1, 1), tmax.size)
    assert counts[0, 0].tolist() == [2, 6, 0, 0] and _same(out[0, 0], np.array([F(2) / F(6)] * 3 + [1], F))
    more, out2 = m.resolve(tmax, occ, (1, 1), tmax.size, counts=np.array([[[3, 4, NAN, NAN]]], F))
    assert more[0, 0].tolist() == [5, 10, 0, 0] and out2[0, 0].tolist() == [0.5, 0.5, 0.5, 1]
    none, out3 = m.resolve(tmax[:2], occ[:2], (1, 1), 2)
    assert none[0, 0].tolist() == [0, 0, 0, 0] and out3[0, 0].tolist() == [1, 1, 1, 0]  # a miss: visible, alpha 0
    assert m.resolve(tmax, occ, (1, 1), tmax.size, want_out=False)[1] is None


# ---- the inputs of the GPU cases -------------------------------------------------------------------------------------------------
def test_the_synthetic_cases_reach_every_rule(oracle):
    """over the sizes of the GPU test, at least tc.MIN_PER_RULE pixels each: a miss, a NaN and a negative alpha, a zero and a NaN
    normal, normals that flip and that do not, n.z of the turned normal equal to +0, -0, 1 and -1, a sun behind, exactly grazing and
    in front; spread == 0 and radius = +inf are settings of the hard sun"""
    seen = collections.Counter()
    for w, h in tc.SIZES:
        c = tc.synthetic(w, h)
        A, N = c["position"][..., 3], c["normal"][..., :3]
        seen["miss"] += int((A == 0).sum())
        seen["nan alpha"] += int(np.isnan(A).sum())
        seen["negative alpha"] += int((A < 0).sum())
        seen["zero normal"] += int(((A > 0) & ~N.any(-1)).sum())
        seen["nan normal"] += int(((A > 0) & np.isnan(N).any(-1)).sum())
        _, ao = tc.generated(oracle, w, h, "ao", 1, 0)
        live = ao["pixel"] == m.P_LIVE
        assert np.array_equal(ao["pixel"] == m.P_NONE_ALPHA, ~(A > 0)) and np.array_equal(ao["pixel"] == m.P_NONE_NORMAL, (A > 0) & ~(m.dot(N, N) > 0))
        seen["flipped"] += int((live & ao["flipped"]).sum())
        seen["kept"] += int((live & ~ao["flipped"]).sum())
        nz = ao["n"][..., 2]
        for name, pattern in (("n.z = +0", F(0.0)), ("n.z = -0", F(-0.0)), ("n.z = 1", F(1)), ("n.z = -1", F(-1))):
            seen[name] += int((live & (bits(nz) == bits(pattern))).sum())
        _, hard = tc.generated(oracle, w, h, "sun_hard", 1, 0)
        cosl = m.dot(hard["n"], np.broadcast_to(np.array(tc.MODES["sun_hard"]["light"], F), hard["n"].shape))
        hit = hard["pixel"] >= m.P_UNLIT
        seen["sun behind"] += int((hit & (cosl < 0)).sum())
        seen["sun grazing"] += int((hit & (cosl == 0)).sum())
        seen["sun in front"] += int((hit & (cosl > 0)).sum())
        assert np.array_equal(hard["pixel"] == m.P_UNLIT, hit & ~(cosl > 0))
        _, soft = tc.generated(oracle, w, h, "sun_soft", 1, 0)
        seen["soft sun lit"] += int((soft["pixel"] == m.P_LIVE).sum())
        seen["soft sun unlit"] += int((soft["pixel"] == m.P_UNLIT).sum())
    print(dict(seen))
    assert len(seen) == 16 and all(n >= tc.MIN_PER_RULE for n in seen.values()), seen
    hard, soft = tc.MODES["sun_hard"], tc.MODES["sun_soft"]
    assert hard["spread"] == 0 and hard["radius"] == INF and soft["spread"] > 0 and soft["light"][2] < 0 and soft["bias"] == 0
    assert tc.synthetic(1, 1)["kind"][0, 0] == 0 and tc.generated(oracle, 1, 1, "ao", 1, 0)[1]["pixel"][0, 0] == m.P_LIVE
    r = tc.resolve_inputs(37, 23, 3)
    assert all((bits(r["tmax"]) == bits(F(v))).sum() >= tc.MIN_PER_RULE for v in tc.TMAX_CODES if v == v) and np.isnan(r["tmax"]).sum() >= tc.MIN_PER_RULE


def test_the_end_to_end_cases_hold_every_class(oracle):
    """on the oracle alone, at the cases' own settings, at least 32 pixels each: AO partly occluded (0 < V < C), free (V == C), dark
    (V == 0 or V <= C / 4) and with a flipped normal; SUN unlit and lit but shadowed, for both spreads, and soft shadows' penumbra"""
    e = tc.e2e_ao(oracle, TEAPOT)
    ao = {k: int(v.sum()) for k, v in tc.classes(e["counts"], e["info"]).items()}
    print("ao", ao)
    assert all(ao[k] >= tc.E2E_MIN_PER_CLASS for k in ("partly", "free", "dark", "flipped")), ao
    assert np.all(e["counts"][..., 1][e["info"]["pixel"] == m.P_LIVE] == tc.E2E_AO["samples"]) and (e["counts"][..., 1] == 0).sum() >= 32  # and misses
    s = tc.e2e_sun(oracle, TEAPOT)
    for spread in tc.E2E_SUN["spreads"]:
        out, counts, info = s[spread]
        sun = {k: int(v.sum()) for k, v in tc.classes(counts, info).items()}
        print("sun", spread, sun)
        assert all(sun[k] >= tc.E2E_MIN_PER_CLASS for k in ("unlit", "shadowed", "flipped", "free")), sun
        assert np.all(counts[..., 0][info["pixel"] == m.P_UNLIT] == 0) and np.all(counts[..., 1][info["pixel"] == m.P_UNLIT] == tc.E2E_SUN["samples"])
    assert tc.classes(s[0.0][1])["partly"].sum() == 0 and tc.classes(s[0.05][1])["partly"].sum() >= 8  # a hard shadow has no penumbra
    assert abs(np.linalg.norm(tc.e2e_light()) - 1) < 1e-6


# ---- the library, before its first HIP call --------------------------------------------------------------------------------------
LW, LH, LB = 6, 5, 3
NO_DEVICE = 1 << 20  # no such GPU: were a call accepted by mistake, the runtime would refuse the device and nothing would be launched
GEN_ARGS = ("position", "normal") + m.RAY_ARRAYS
RES_ARGS = ("tmax", "occluded", "counts", "out")
PLANE_BYTES, RAY_BYTES = LH * LW * 16, LH * LW * LB * 4


def _settings(**kw):
    v = dict(struct_size=C.sizeof(sv.SecondarySettings), width=LW, height=LH, mode=0, flags=0, sample_count=8, sample_begin=2, batch=LB,
             seed=1, radius=1.0, bias=1e-4, spread=0.0)
    eye, light = kw.pop("eye", (0.0, 0.0, 5.0)), kw.pop("light", (0.0, 0.6, 0.8))
    v.update(kw)
    st = sv.SecondarySettings(**v)
    st.eye[:], st.light[:] = eye, light
    return st


def test_struct_sizes_and_symbols():
    L = sv.lib()
    assert L.mps_settings_size() == C.sizeof(sv.SecondarySettings) == 80 and sv.SecondarySettings.spread.offset == 72
    header = open(os.path.join(ROOT, "include", "minipath_secondary.h")).read()
    declared = set(re.findall(r"\b(mps_[a-z_]+)\s*\(", header.split("#ifndef MINIPATH_SECONDARY_H")[1]))
    assert declared == set(sv.SIGNATURES) and all(hasattr(L, n) for n in declared)
    assert mp.SecondaryVisibility is sv.SecondaryVisibility and "SecondaryVisibility" in mp.__all__
    assert L.mps_check_settings(C.byref(_settings())) == 0
    assert L.mps_check_settings(C.byref(_settings(struct_size=76, mode=1, flags=1, radius=INF, bias=0.0, spread=3.0, sample_count=65536,
                                                  sample_begin=63489, width=1 << 20, height=1, batch=2047))) == 0
    assert L.mps_check_settings(C.byref(_settings(width=1 << 15, height=1 << 15, batch=1))) == 0  # 2^30 rays


def _buffers(names):
    # one allocation, so that "overlapping" can be asked for: buffer k at byte offset k * 2 * PLANE_BYTES (a ray array is smaller)
    whole = np.full(len(names) * 2 * PLANE_BYTES // 4, SENTINEL, np.uint32)
    return whole, {k: whole.ctypes.data + i * 2 * PLANE_BYTES for i, k in enumerate(names)}


def _call(fn_name, names, st, device=NO_DEVICE, **replace):
    whole, ptr = _buffers(names)
    for k, v in replace.items():
        ptr[k] = None if v is None else (ptr[v[0]] + v[1] if isinstance(v, tuple) else ptr[v])
    before = sv.last_kernels()
    rc = getattr(sv.lib(), fn_name)(device, None if st is None else C.byref(st), *[ptr[k] for k in names], None)
    assert sv.last_kernels() == before  # nothing was launched
    assert np.all(whole == SENTINEL)    # nothing was written (host memory here: a launch would not even get this far)
    return rc


def _generate(st, **kw):
    return _call("mps_generate", GEN_ARGS, st, **kw)


def _resolve(st, **kw):
    return _call("mps_resolve", RES_ARGS, st, **kw)


BAD_SETTINGS = [dict(width=0), dict(height=0), dict(width=0, height=0), dict(width=(1 << 20) + 1), dict(height=(1 << 20) + 1), dict(batch=0),
                dict(width=1 << 16, height=1 << 15, batch=1), dict(width=1 << 20, height=1 << 20, batch=1), dict(width=1 << 10, height=1 << 10, batch=2048, sample_count=65536),
                dict(width=1 << 20, height=1, batch=2048, sample_count=65536), dict(batch=0xFFFFFFFF), dict(sample_begin=6), dict(sample_begin=0xFFFFFFFF),
                dict(sample_begin=0xFFFFFFFE, batch=3), dict(sample_count=0, sample_begin=0), dict(sample_count=65537), dict(sample_count=2), dict(mode=2),
                dict(mode=0xFFFFFFFF), dict(flags=2), dict(flags=0x80000001), dict(radius=0.0), dict(radius=-1.0), dict(radius=NAN), dict(radius=-INF),
                dict(bias=-1e-4), dict(bias=NAN), dict(bias=INF), dict(spread=-0.1), dict(spread=NAN), dict(spread=INF), dict(eye=(NAN, 0, 0)),
                dict(eye=(0, INF, 0)), dict(eye=(0, 0, -INF)), dict(light=(NAN, 0, 1)), dict(light=(0, INF, 1)), dict(light=(0, 0, NAN)),
                dict(struct_size=0), dict(struct_size=72), dict(struct_size=75)]
BAD_GENERATE = ([{k: None} for k in GEN_ARGS] + [dict(device=-1), dict(settings=None)]
                + [{o: i} for o in m.RAY_ARRAYS for i in ("position", "normal")]               # a ray array equal to a plane
                + [dict(oy="ox"), dict(tmax="dz"), dict(dx="oz")]                            # two ray arrays the same
                + [dict(ox=("position", PLANE_BYTES - 4)), dict(position=("ox", RAY_BYTES - 4)), dict(oy=("ox", 4)), dict(tmax=("normal", -RAY_BYTES + 4)),
                   dict(normal=("dz", -PLANE_BYTES + 16))])                                   # partial overlaps
BAD_RESOLVE = ([{k: None} for k in RES_ARGS if k != "out"] + [dict(device=-1), dict(settings=None)]
               + [dict(counts="tmax"), dict(counts="occluded"), dict(out="tmax"), dict(out="occluded"), dict(out="counts"),
                  dict(counts=("tmax", RAY_BYTES - 4)), dict(out=("occluded", LH * LW * LB - 1)), dict(occluded=("counts", PLANE_BYTES - 1)),
                  dict(out=("counts", 16)), dict(tmax=("out", -RAY_BYTES + 4))])


def _id(d):
    return ",".join(f"{k}={v}" for k, v in d.items())


@pytest.mark.parametrize("bad", BAD_SETTINGS, ids=_id)
def test_settings_are_refused(bad):
    for call in (_generate, _resolve):
        assert call(_settings(**bad)) == MP_ERR_INVALID
        assert sv.lib().mps_last_error()
    assert sv.lib().mps_check_settings(C.byref(_settings(**bad))) == MP_ERR_INVALID


@pytest.mark.parametrize("bad", BAD_GENERATE, ids=_id)
def test_generate_refuses_arguments(bad):
    bad = dict(bad)
    st = None if "settings" in bad and bad.pop("settings") is None else _settings()
    assert _generate(st, **bad) == MP_ERR_INVALID
    assert sv.lib().mps_last_error()


@pytest.mark.parametrize("bad", BAD_RESOLVE, ids=_id)
def test_resolve_refuses_arguments(bad):
    bad = dict(bad)
    st = None if "settings" in bad and bad.pop("settings") is None else _settings()
    assert _resolve(st, **bad) == MP_ERR_INVALID
    assert sv.lib().mps_last_error()


def test_what_is_not_refused_gets_to_the_device():
    """the same calls with nothing wrong, and their legal variations, get as far as the device (which does not exist): MP_ERR_HIP"""
    assert sv.lib().mps_check_settings(None) == MP_ERR_INVALID
    for mode in (0, 1):
        assert _generate(_settings(mode=mode, radius=INF)) == MP_ERR_HIP
    assert _generate(_settings(), normal="position") == MP_ERR_HIP                                # inputs may alias inputs
    assert _generate(_settings(), ox=("position", PLANE_BYTES)) == MP_ERR_HIP                     # adjacent is not overlapping
    assert _generate(_settings(), oy=("ox", RAY_BYTES)) == MP_ERR_HIP
    assert _generate(_settings(sample_begin=5)) == MP_ERR_HIP                                     # the last samples of the pass
    assert _resolve(_settings()) == MP_ERR_HIP
    assert _resolve(_settings(flags=1), out=None) == MP_ERR_HIP
    assert _resolve(_settings(), occluded=("tmax", RAY_BYTES)) == MP_ERR_HIP
    assert _resolve(_settings(), occluded="tmax") == MP_ERR_HIP


def test_last_kernels_buffer_protocol():
    L = sv.lib()
    need = C.c_size_t(99)
    assert L.mps_last_kernels(None, 0, C.byref(need)) == 0 and need.value == len("\n".join(sv.last_kernels()))
    assert L.mps_last_kernels(None, 4, None) == MP_ERR_INVALID
    buf = C.create_string_buffer(b"xxxx", 4)
    assert L.mps_last_kernels(buf, 1, None) == 0 and buf.raw[0] == 0  # cap 1: the terminating 0 alone


def test_a_host_only_scene_raises():
    """a scene without a Context cannot be traced (as TriangleBvh.occluded says)"""
    host_scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT))
    with pytest.raises(mp.MinipathError):
        mp.SecondaryVisibility(host_scene, (8, 8))
    assert mp.SecondaryVisibility.eye_of(mp.Camera.teapot_view()) == [0.0, 2.0, 10.0]
