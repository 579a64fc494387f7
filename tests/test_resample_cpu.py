"""CPU tests of the guided resampling: the numpy model (tests/resample_model.py, the restatement of include/minipath_resample.h that the
GPU tests compare bits against) against a scalar restatement and a float64 evaluation, the conditions on the inputs of the GPU cases
(tests/resample_cases.py), the usefulness of the shipped default weights, and what libminipath_resample.so decides before its first
HIP call -- every refusal, the struct size, the symbols -- through the built library without touching a GPU."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import resample as rs
from tests import resample_cases as tc, resample_model as m
from tests.conftest import ROOT, TEAPOT
from tests.resample_model import F, bits

MP_ERR_INVALID, MP_ERR_HIP = 1, 4
SENTINEL = 0x5A5A5A5A
INF, NAN = float("inf"), float("nan")
U = 2.0 ** -24  # the unit roundoff of binary32


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _scalar_upsample(x, y, position, normal, position_lo, normal_lo, picks, color_lo, f, k, sigma_plane):
    """the header's mpr_upsample for one pixel, one np.float32 scalar operation per line of the text"""
    H, W = position.shape[:2]
    h, w = picks.shape
    zero = np.zeros(4, F)

    def dot(a, b):
        return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))

    with np.errstate(all="ignore"):
        A = position[y, x, 3]
        if not A > 0:
            return zero
        P = [F(position[y, x, c] / A) for c in range(3)]
        N = normal[y, x, :3]
        l2 = dot(N, N)
        if not l2 > 0:
            return zero
        ln = np.sqrt(l2)
        n = [F(N[c] / ln) for c in range(3)]
        sd = F(F(sigma_plane) * F(normal[y, x, 3] / A))
        sum_w, sum_c, near = F(0), [F(0)] * 3, None
        for dY in (-1, 0, 1):
            for dX in (-1, 0, 1):
                qx, qy = x // f + dX, y // f + dY
                if not (0 <= qx < w and 0 <= qy < h):
                    continue
                pk = int(picks[qy, qx])
                Nq = normal_lo[qy, qx, :3]
                if pk == m.PICK_NONE or pk >= W * H or color_lo[qy, qx, 3] == 0 or not position_lo[qy, qx, 3] > 0 or not dot(Nq, Nq) > 0:
                    continue
                ddx, ddy = F(x - pk % W), F(y - pk // W)
                d2 = F(F(ddx * ddx) + F(ddy * ddy))
                ws = F(F(1) / F(F(1) + F(d2 / F(f * f))))
                Pq = [F(position_lo[qy, qx, c] / position_lo[qy, qx, 3]) for c in range(3)]
                lq = np.sqrt(dot(Nq, Nq))
                nq = [F(Nq[c] / lq) for c in range(3)]
                d = dot(n, nq)
                wn = d if d > 0 else F(0)
                for _ in range(k):
                    wn = F(wn * wn)
                e = dot(n, [F(Pq[c] - P[c]) for c in range(3)])
                a = F(np.abs(e) / sd)
                wp = F(F(1) / F(F(1) + F(a * a)))
                wt = F(F(ws * wn) * wp)
                if np.isnan(wt):
                    wt = F(0)
                if near is None or d2 < near[0]:
                    near = (d2, color_lo[qy, qx, :3])
                if wt == 0:
                    continue
                sum_w = F(sum_w + wt)
                sum_c = [F(sum_c[c] + F(wt * color_lo[qy, qx, c])) for c in range(3)]
        if sum_w > 0:
            return np.array([F(sum_c[c] / sum_w) for c in range(3)] + [F(1)], F)
        if near is not None:
            return np.array(list(near[1]) + [F(1)], F)
        return zero


@pytest.mark.parametrize("f", tc.FACTORS)
def test_the_model_has_no_tiles(f):
    """the vectorised model equals the header evaluated pixel by pixel, alone, on the rows and columns on both sides of every edge
    of the kernel's 16 x 16 tiles and of the image (37 x 23: 3 x 2 tiles, ragged): a pixel's result is a function of its 3 x 3 low
    neighbours, wherever a tile begins -- which is what the bit comparison of the GPU test then holds the kernel to"""
    W, H = 37, 23
    c, u = tc.synthetic(W, H), tc.upsample_inputs(W, H, f)
    cols = [x for x in (0, 1, 14, 15, 16, 17, 30, 31, 32, 33, 35, 36)]
    rows = [y for y in (0, 1, 7, 8, 14, 15, 16, 17, 21, 22)]
    n = 0
    for y in range(H):
        for x in range(W):
            if x in cols or y in rows:
                want = _scalar_upsample(x, y, c["position"], c["normal"], u["position_lo"], u["normal_lo"], u["picks"], u["color_lo"], f, u["k"],
                                        u["sigma_plane"])
                assert _same(u["out"][y, x], want), (x, y, u["out"][y, x], want)
                n += 1
    assert n >= 500


def _f64_bound(k, sigma_plane, position, normal, position_lo, keep):
    """The error bound of the f32 evaluation against the f64 one, from the operation count (u = 2^-24), for pixels with sum_w >= 1/4
    and colours in [0, 1].  out is a weighted mean, so an absolute error dw_i in each of the 9 weights moves it by at most
    sum(dw_i) / sum_w <= 36 dw.  w = ws wn wp, each factor at most 1 (+ a few u), so dw <= d(ws) + d(wn) + d(wp) + 2u.
      ws: three roundings of quantities <= 1 (d2 is exact): 3u.
      wn: n.c and nq.c carry 4 roundings each (two products and two sums of l2 shared, sqrt, divide: <= 4u relative), so the dot of the
          two unit vectors is off by at most 3 (4u + 4u + u) + 2u = 29u absolutely; max(., 0) is 1-Lipschitz and k squarings multiply
          an error by at most 2^k (the derivative of d^(2^k) on [0, 1]) and add u each: 2^k 29u + k u.
      wp: P.c, Pq.c one rounding each, the difference one more: |d(Pq.c - P.c)| <= 2u (|P.c| + |Pq.c|); times n.c (|n.c| <= 1, 4u
          relative), three products and two sums: de <= 3 * 2u * S + 8u * S = 14u S with S = max(|P| + |Pq|) over the case (>= any
          |Pq - P|).  a = |e| / sd, sd two roundings: da <= de / sd + 3u a.  wp = 1 / (1 + a^2) has |wp'| <= 0.65 and a |wp'| <= 1/2:
          d(wp) <= 0.65 * 14u S / sd_min + 1.5u + 3u.
    The final divide and the sums of step 3 add (9 + 9 + 1)u relative to a value <= 1."""
    with np.errstate(all="ignore"):
        P = position[..., :3] / position[..., 3:4]
        Pq = position_lo[..., :3] / position_lo[..., 3:4]
        sd = sigma_plane * normal[..., 3] / position[..., 3]
    S = float(np.nanmax(np.linalg.norm(P[keep].astype(np.float64), axis=-1))) + float(
        np.nanmax(np.linalg.norm(Pq[np.isfinite(Pq).all(-1)].astype(np.float64), axis=-1)))
    sd_min = float(np.min(sd[keep]))
    dwp = 0.0 if np.isinf(sigma_plane) else 0.65 * 14 * U * S / sd_min + 4.5 * U
    dw = 3 * U + (2 ** k * 29 + k) * U + dwp + 2 * U
    return 36 * dw + 19 * U


def test_the_model_against_float64(oracle):
    """every synthetic upsample case of 37 x 23 and the end-to-end case with the shipped weights: where the float64 evaluation of the
    same text has sum_w >= 1/4 the float32 model agrees within the bound derived in _f64_bound (printed beside the measured error)"""
    cases = []
    for f in tc.FACTORS:
        c, u = tc.synthetic(37, 23), tc.upsample_inputs(37, 23, f)
        cases.append((f"synthetic f={f}", f, u["k"], u["sigma_plane"], c["position"], c["normal"], u["position_lo"], u["normal_lo"], u["picks"],
                      u["color_lo"], u["out"]))
    fr, lo = tc.e2e_frame(oracle, TEAPOT), tc.e2e_low(oracle, TEAPOT, tc.E2E["phase"])
    k, sp = rs.DEFAULT_SIGMA_NORMAL_POW2, rs.DEFAULT_SIGMA_PLANE
    cases.append(("teapot", 2, k, sp, fr["planes"]["position"], fr["planes"]["normal"], lo["position_lo"], lo["normal_lo"], lo["picks"], lo["ao_lo"],
                  tc.e2e_up(oracle, TEAPOT, tc.E2E["phase"], k, sp)[0]))
    for name, f, k, sp, position, normal, position_lo, normal_lo, picks, color_lo, out32 in cases:
        out64, info = m.upsample(position, normal, position_lo, normal_lo, picks, color_lo, f, k, sp, want_info=True, dtype=np.float64)
        with np.errstate(all="ignore"):
            keep = (info["how"] == 1) & (info["sum_w"] >= 0.25) & np.isfinite(out64).all(-1) & (normal[..., 3] / position[..., 3] > 0)
        assert keep.sum() >= 32, (name, int(keep.sum()))
        tol = _f64_bound(k, sp, position, normal, position_lo, keep)
        err = float(np.max(np.abs(out32[keep].astype(np.float64) - out64[keep])))
        print(f"{name}: {int(keep.sum())} pixels, max |f32 - f64| = {err:.3e}, bound {tol:.3e}")
        assert err <= tol, (name, err, tol)
        assert np.all(out32[keep][:, 3] == 1)


def test_a_picked_pixel_gets_its_own_colour_back(oracle):
    """out is a weighted mean of colours in [0, 1], so at a block's pick, whose own tap has the weight w_own, it is within
    1 - w_own / sum_w of the pick's low colour (+ 8u of rounding): the own-tap dominance.  With every other tap skipped the mean is
    (w c) / w: the colour to within two roundings, and the colour's very bits when w == 1 (an axis normal, k squarings of 1)"""
    n = 0
    for W, H in tc.SIZES:
        for f in tc.FACTORS:
            u = tc.upsample_inputs(W, H, f)
            info = u["info"]
            own = info["own"] & (info["how"] == 1) & (info["w_own"] > 0)
            ys, xs = np.nonzero(own)
            c_own = u["color_lo"][ys // f, xs // f, :3]
            slack = 1 - info["w_own"][own].astype(np.float64) / info["sum_w"][own] + 8 * U
            assert np.all(np.abs(u["out"][ys, xs, :3].astype(np.float64) - c_own) <= slack[:, None])
            n += len(ys)
    assert n >= 200, n
    # one valid block in a frame of misses: every other tap is skipped
    for normal_xyz, exact in (((0.0, 0.0, 0.5), True), ((0.3, -0.2, 0.4), False)):
        for f in tc.FACTORS:
            W, H = 3 * f, 3 * f
            position, normal = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
            y, x = f + 1, f  # in the middle block, not its first pixel
            position[y, x] = (0.25, -0.5, 1.5, 0.5)
            normal[y, x] = normal_xyz + (3.0,)
            picks, (plo, nlo) = m.downsample(position, normal, [position, normal], f, m.PICK_PHASE, 0)
            assert picks[1, 1] == y * W + x and (picks != m.PICK_NONE).sum() == 1
            color_lo = np.full((3, 3, 4), 0.7, F)
            color_lo[1, 1] = (0.1, 0.6234567, 0.9, 1.0)
            for k in (0, 1, 8):
                out, info = m.upsample(position, normal, plo, nlo, picks, color_lo, f, k, 0.01, want_info=True)
                assert info["used"][y, x] == 1 and (out[..., 3] != 0).sum() == 1
                if exact:
                    assert _same(out[y, x], color_lo[1, 1])
                else:
                    assert np.all(np.abs(out[y, x, :3].astype(np.float64) - color_lo[1, 1, :3]) <= 2 * U * color_lo[1, 1, :3]) and out[y, x, 3] == 1


def test_downsample_by_hand():
    """a 5 x 2 frame at f = 2 (the last block ragged): the phase candidate, the scan past an invalid candidate, the candidate outside
    a ragged block, and NEAREST's strict compare with equal and NaN depths"""
    position, normal = np.zeros((2, 5, 4), F), np.zeros((2, 5, 4), F)
    position[..., 3] = 1
    normal[..., 2] = 1
    normal[..., 3] = [[3, 2, 5, 5, 9], [2, 1, NAN, 4, 8]]
    position[0, 0, 3] = 0        # block 0: its first pixel is a miss
    normal[1, 1, :3] = 0         #          and its last has no normal
    ids = np.arange(40, dtype=np.int32).reshape(2, 5, 4)
    picks, (ids_lo,) = m.downsample(position, normal, [ids], 2, m.PICK_PHASE, 0)
    assert picks.tolist() == [[1, 2, 4]] and ids_lo[0, 0].tolist() == [4, 5, 6, 7]                # scan, candidate, candidate
    assert m.downsample(position, normal, [], 2, m.PICK_PHASE, 3)[0].tolist() == [[1, 8, 4]]       # scan, candidate, outside -> scan
    assert m.downsample(position, normal, [], 2, m.PICK_NEAREST, 0)[0].tolist() == [[1, 8, 9]]     # 2, and 2 == 2 keeps the first; 4 < 5 after 5 == 5 and NaN; 8 < 9
    normal[0, 2, 3] = NAN
    assert m.downsample(position, normal, [], 2, m.PICK_NEAREST, 0)[0].tolist() == [[1, 2, 9]]     # a NaN first is never replaced
    position[..., 3] = -1
    picks, (ids_lo,) = m.downsample(position, normal, [ids], 2, m.PICK_NEAREST, 0)
    assert np.all(picks == m.PICK_NONE) and not ids_lo.any()
    assert m.low_size(5, 2, 2) == (3, 1) and m.low_size(37, 23, 4) == (10, 6) and m.low_size(1, 1, 3) == (1, 1)


# ---- the inputs of the GPU cases -------------------------------------------------------------------------------------------------
def test_the_synthetic_cases_reach_every_rule():
    """over the sizes, factors, phases and pick modes of the GPU test, at least tc.MIN_PER_RULE pixels each (full pixels for the
    planted values and the outcomes of mpr_upsample, low pixels for the outcomes of mpr_downsample and the planted low values), and
    every factor reaches every block-level rule at least once"""
    seen, per_f = collections.Counter(), collections.defaultdict(collections.Counter)
    for W, H in tc.SIZES:
        c = tc.synthetic(W, H)
        A, N = c["position"][..., 3], c["normal"][..., :3]
        seen["miss"] += int((A == 0).sum())
        seen["nan alpha"] += int(np.isnan(A).sum())
        seen["negative alpha"] += int((A < 0).sum())
        seen["zero normal"] += int(((A > 0) & ~N.any(-1)).sum())
        seen["nan normal"] += int(((A > 0) & np.isnan(N).any(-1)).sum())
        seen["nan depth"] += int((m.valid(c["position"], c["normal"]) & np.isnan(c["normal"][..., 3])).sum())
    for (W, H), f, mode, phase in tc.down_cases():
        picks, planes, info = tc.downsampled(W, H, f, mode, phase)
        here = collections.Counter()
        here["no pick"] = int((info["how"] == 0).sum())
        assert np.array_equal(info["how"] == 0, picks == m.PICK_NONE) and not planes[0][picks == m.PICK_NONE].any()
        if mode == m.PICK_PHASE:
            here["phase candidate"] = int((info["how"] == 1).sum())
            here["scan fallback"] = int((info["how"] == 2).sum())
        else:
            here["nearest replaced"] = int((info["replaced"] > 0).sum())
            here["nearest kept the first"] = int(((info["how"] == 3) & (info["replaced"] == 0)).sum())
            here["equal depths"] = int((info["ties"] > 0).sum())
            here["nan depth first"] = int(info["nan_first"].sum())
        seen.update(here)
        per_f[f].update(here)
    for W, H in tc.SIZES:
        for f in tc.FACTORS:
            u = tc.upsample_inputs(W, H, f)
            info, here = u["info"], collections.Counter()
            h, w = u["picks"].shape
            here["low alpha 0"] = int((u["color_lo"][..., 3] == 0).sum())
            here["corrupted pick"] = int(((u["picks"] != m.PICK_NONE) & (u["picks"] >= W * H)).sum())
            here["nan low position"] = int(np.isnan(u["position_lo"][..., :3]).any(-1).sum())
            here["zero pixel"] = int((info["how"] == 0).sum())
            here["weighted mean"] = int((info["how"] == 1).sum())
            here["blended by >= 2 taps"] = int((info["used"] >= 2).sum())
            here["nearest-tap fallback"] = int((info["how"] == 2).sum())
            here["every live tap has wn == 0"] = int(((info["how"] == 2) & (info["live"] > 0) & (info["wn0"] == info["live"])).sum())
            here["hole"] = int((info["how"] == 3).sum())
            here["tap outside the low image"] = int(((np.mgrid[0:H, 0:W][1] // f == 0) | (np.mgrid[0:H, 0:W][0] // f == h - 1)).sum())
            seen.update(here)
            per_f[f].update(here)
    print(dict(seen))
    assert len(seen) == 23 and all(n >= tc.MIN_PER_RULE for n in seen.values()), seen
    for f in tc.FACTORS:
        assert all(per_f[f][k] >= 1 for k in per_f[2]), (f, per_f[f])
    assert tc.synthetic(1, 1)["kind"][0, 0] == 0 and tc.downsampled(1, 1, 2, m.PICK_PHASE, 3)[0][0, 0] == 0  # a plain hit, found by the scan
    assert [tc.phases(f) for f in tc.FACTORS] == [[0, 2, 3], [0, 4, 8], [0, 8, 15]]


def _e2e_classes(oracle, phase):
    out, info = tc.e2e_up(oracle, TEAPOT, phase, rs.DEFAULT_SIGMA_NORMAL_POW2, rs.DEFAULT_SIGMA_PLANE)
    fr = tc.e2e_frame(oracle, TEAPOT)
    miss = ~(fr["planes"]["position"][..., 3] > 0)
    near_miss = np.zeros_like(miss)
    near_miss[1:] |= miss[:-1]
    near_miss[:-1] |= miss[1:]
    near_miss[:, 1:] |= miss[:, :-1]
    near_miss[:, :-1] |= miss[:, 1:]
    return {"picked": info["own"], "blended by >= 2 taps": info["used"] >= 2, "a tap rejected by the normal weight": info["wn0"] > 0,
            "a tap with wp < 1/2": info["wp_half"] > 0, "bordering a miss": ~miss & near_miss}


def test_the_end_to_end_case_holds_every_class(oracle):
    """on the oracle alone, with the shipped weights, at least 32 pixels each, for both phases of the GPU test"""
    for phase in (tc.E2E["phase"], tc.E2E["second_phase"]):
        got = {k: int(v.sum()) for k, v in _e2e_classes(oracle, phase).items()}
        print(phase, got)
        assert len(got) == 5 and all(n >= tc.E2E_MIN_PER_CLASS for n in got.values()), (phase, got)
    a, b = tc.e2e_low(oracle, TEAPOT, tc.E2E["phase"]), tc.e2e_low(oracle, TEAPOT, tc.E2E["second_phase"])
    assert ((a["picks"] != b["picks"]) & (a["picks"] != m.PICK_NONE)).sum() >= 32  # the second phase gives other picks
    assert m.low_size(*tc.E2E["res"], tc.E2E["factor"]) == (24, 16)


def test_the_shipped_defaults_are_useful(oracle):
    """against the oracle's 64-sample ambient occlusion at full resolution, the model's upsampled 8 samples traced at 24 x 16 have a
    strictly smaller mean absolute error over the hit pixels than each block's pick replicated over the block"""
    fr, lo, ref = tc.e2e_frame(oracle, TEAPOT), tc.e2e_low(oracle, TEAPOT, tc.E2E["phase"]), tc.e2e_reference(oracle, TEAPOT)
    out, _ = tc.e2e_up(oracle, TEAPOT, tc.E2E["phase"], rs.DEFAULT_SIGMA_NORMAL_POW2, rs.DEFAULT_SIGMA_PLANE)
    hit = fr["planes"]["position"][..., 3] > 0
    rep = m.replicate(lo["picks"], lo["ao_lo"], fr["planes"]["position"], tc.E2E["factor"])
    err = {k: float(np.abs(v[..., 0][hit].astype(np.float64) - ref[..., 0][hit]).mean()) for k, v in (("guided", out), ("replicated", rep))}
    print(err)
    assert hit.sum() >= 500 and np.all(out[..., 3][hit & (rep[..., 3] > 0)] == 1)
    assert err["guided"] < err["replicated"], err


# ---- the library, before its first HIP call --------------------------------------------------------------------------------------
LW, LH, LF = 6, 5, 2
NO_DEVICE = 1 << 20  # no such GPU: were a call accepted by mistake, the runtime would refuse the device and nothing would be launched
PLANE_BYTES = LH * LW * 16
LOW_BYTES, PICK_BYTES = 3 * 3 * 16, 3 * 3 * 4
DOWN_ARGS = ("position", "normal", "src0", "src1", "dst0", "dst1", "picks")
UP_ARGS = ("position", "normal", "position_lo", "normal_lo", "picks", "color_lo", "out")


def _settings(**kw):
    v = dict(struct_size=C.sizeof(rs.ResampleSettings), width=LW, height=LH, factor=LF, pick_mode=0, phase=1, sigma_normal_pow2=2.0,
             sigma_plane=0.05)
    v.update(kw)
    return rs.ResampleSettings(**v)


def _buffers(names):
    # one allocation, so that "overlapping" can be asked for: buffer k at byte offset k * 2 * PLANE_BYTES
    whole = np.full(len(names) * 2 * PLANE_BYTES // 4, SENTINEL, np.uint32)
    return whole, {k: whole.ctypes.data + i * 2 * PLANE_BYTES for i, k in enumerate(names)}


def _resolve(ptr, replace):
    for k, v in replace.items():
        ptr[k] = None if v is None else (ptr[v[0]] + v[1] if isinstance(v, tuple) else ptr[v])


def _downsample(st, device=NO_DEVICE, n_planes=2, arrays=(True, True), **replace):
    whole, ptr = _buffers(DOWN_ARGS)
    _resolve(ptr, replace)
    before = rs.last_kernels()
    src = rs.pointer_array([ptr["src0"], ptr["src1"], ptr["src0"], ptr["src1"], ptr["src0"]]) if arrays[0] else None
    dst = rs.pointer_array([ptr["dst0"], ptr["dst1"], ptr["dst0"], ptr["dst1"], ptr["dst0"]]) if arrays[1] else None
    rc = rs.lib().mpr_downsample(device, None if st is None else C.byref(st), ptr["position"], ptr["normal"], n_planes, src, dst, ptr["picks"], None)
    assert rs.last_kernels() == before  # nothing was launched
    assert np.all(whole == SENTINEL)    # nothing was written (host memory here: a launch would not even get this far)
    return rc


def _upsample(st, device=NO_DEVICE, **replace):
    whole, ptr = _buffers(UP_ARGS)
    _resolve(ptr, replace)
    before = rs.last_kernels()
    rc = rs.lib().mpr_upsample(device, None if st is None else C.byref(st), *[ptr[k] for k in UP_ARGS], None)
    assert rs.last_kernels() == before
    assert np.all(whole == SENTINEL)
    return rc


def test_struct_sizes_and_symbols():
    L = rs.lib()
    assert L.mpr_settings_size() == C.sizeof(rs.ResampleSettings) == 32 and rs.ResampleSettings.sigma_plane.offset == 28
    header = open(os.path.join(ROOT, "include", "minipath_resample.h")).read()
    declared = set(re.findall(r"\b(mpr_[a-z_]+)\s*\(", header.split("#ifndef MINIPATH_RESAMPLE_H")[1]))
    assert declared == set(rs.SIGNATURES) and all(hasattr(L, n) for n in declared)
    assert mp.GuidedResampler is rs.GuidedResampler and "GuidedResampler" in mp.__all__
    assert L.mpr_check_settings(C.byref(_settings())) == 0
    assert L.mpr_check_settings(C.byref(_settings(factor=4, pick_mode=1, phase=15, sigma_normal_pow2=8.0, sigma_plane=INF, width=1 << 20, height=4095))) == 0
    assert L.mpr_check_settings(C.byref(_settings(struct_size=64, sigma_normal_pow2=0.0, width=1, height=1 << 20))) == 0
    for (W, H, f) in ((6, 5, 2), (37, 23, 3), (37, 23, 4), (1, 1, 4), (1 << 20, 4095, 3)):
        lw, lh = C.c_uint32(), C.c_uint32()
        assert L.mpr_low_size(C.byref(_settings(width=W, height=H, factor=f)), C.byref(lw), C.byref(lh)) == 0
        assert (lw.value, lh.value) == m.low_size(W, H, f)
    assert L.mpr_low_size(C.byref(_settings()), None, C.byref(lh)) == MP_ERR_INVALID and L.mpr_low_size(None, C.byref(lw), C.byref(lh)) == MP_ERR_INVALID
    assert (rs.MPR_PICK_PHASE, rs.MPR_PICK_NEAREST, rs.MPR_PICK_NONE, rs.MPR_MAX_PLANES) == (m.PICK_PHASE, m.PICK_NEAREST, m.PICK_NONE, m.MAX_PLANES)
    for name, value in (("MPR_PICK_PHASE", "0u"), ("MPR_PICK_NEAREST", "1u"), ("MPR_PICK_NONE", "0xFFFFFFFFu"), ("MPR_MAX_PLANES", "4u")):
        assert re.search(rf"#define {name} {value}\b", header), name


BAD_SETTINGS = [dict(width=0), dict(height=0), dict(width=0, height=0), dict(width=(1 << 20) + 1), dict(height=(1 << 20) + 1),
                dict(width=1 << 20, height=4096), dict(width=1 << 20, height=1 << 20), dict(factor=0), dict(factor=1), dict(factor=5),
                dict(factor=0xFFFFFFFF), dict(pick_mode=2), dict(pick_mode=0xFFFFFFFF), dict(phase=4), dict(phase=0xFFFFFFFF),
                dict(factor=3, phase=9), dict(factor=4, phase=16), dict(pick_mode=1, phase=4), dict(sigma_normal_pow2=-1.0),
                dict(sigma_normal_pow2=9.0), dict(sigma_normal_pow2=1.5), dict(sigma_normal_pow2=NAN), dict(sigma_normal_pow2=INF),
                dict(sigma_plane=0.0), dict(sigma_plane=-0.05), dict(sigma_plane=NAN), dict(sigma_plane=-INF), dict(struct_size=0),
                dict(struct_size=28), dict(struct_size=31)]
BAD_DOWN = ([{k: None} for k in ("position", "normal", "src0", "src1", "dst0", "dst1", "picks")]
            + [dict(device=-1), dict(settings=None), dict(n_planes=5), dict(n_planes=0xFFFFFFFF), dict(arrays=(False, True)), dict(arrays=(True, False))]
            + [dict(dst0="position"), dict(dst1="normal"), dict(dst0="src0"), dict(dst1="src0"), dict(dst1="dst0"), dict(picks="dst0"),
               dict(picks="position"), dict(picks="src1")]                                                    # an output equal to another buffer
            + [dict(dst0=("position", PLANE_BYTES - 16)), dict(position=("dst0", LOW_BYTES - 16)), dict(dst1=("dst0", 16)),
               dict(picks=("dst1", LOW_BYTES - 4)), dict(dst0=("picks", PICK_BYTES - 4)), dict(src1=("picks", -PLANE_BYTES + 4)),
               dict(picks=("normal", PLANE_BYTES - 4))])                                                      # partial overlaps
BAD_UP = ([{k: None} for k in UP_ARGS] + [dict(device=-1), dict(settings=None)]
          + [dict(out=k) for k in UP_ARGS[:-1]]
          + [dict(out=("position", PLANE_BYTES - 16)), dict(normal=("out", PLANE_BYTES - 16)), dict(out=("color_lo", LOW_BYTES - 16)),
             dict(picks=("out", PLANE_BYTES - 4)), dict(out=("picks", PICK_BYTES - 4)), dict(position_lo=("out", -LOW_BYTES + 16))])


def _id(d):
    return ",".join(f"{k}={v}" for k, v in d.items())


@pytest.mark.parametrize("bad", BAD_SETTINGS, ids=_id)
def test_settings_are_refused(bad):
    for call in (_downsample, _upsample):
        assert call(_settings(**bad)) == MP_ERR_INVALID
        assert rs.lib().mpr_last_error()
    assert rs.lib().mpr_check_settings(C.byref(_settings(**bad))) == MP_ERR_INVALID
    lw, lh = C.c_uint32(77), C.c_uint32(77)
    assert rs.lib().mpr_low_size(C.byref(_settings(**bad)), C.byref(lw), C.byref(lh)) == MP_ERR_INVALID and (lw.value, lh.value) == (77, 77)


@pytest.mark.parametrize("bad", BAD_DOWN, ids=_id)
def test_downsample_refuses_arguments(bad):
    bad = dict(bad)
    st = None if "settings" in bad and bad.pop("settings") is None else _settings()
    assert _downsample(st, **bad) == MP_ERR_INVALID
    assert rs.lib().mpr_last_error()


@pytest.mark.parametrize("bad", BAD_UP, ids=_id)
def test_upsample_refuses_arguments(bad):
    bad = dict(bad)
    st = None if "settings" in bad and bad.pop("settings") is None else _settings()
    assert _upsample(st, **bad) == MP_ERR_INVALID
    assert rs.lib().mpr_last_error()


def test_what_is_not_refused_gets_to_the_device():
    """the same calls with nothing wrong, and their legal variations, get as far as the device (which does not exist): MP_ERR_HIP"""
    assert rs.lib().mpr_check_settings(None) == MP_ERR_INVALID
    for mode in (0, 1):
        assert _downsample(_settings(pick_mode=mode, sigma_plane=INF)) == MP_ERR_HIP
    assert _downsample(_settings(), n_planes=0, arrays=(False, False)) == MP_ERR_HIP            # picks alone
    assert _downsample(_settings(), src0="position", src1="normal") == MP_ERR_HIP               # sources may be the guides
    assert _downsample(_settings(), src1="src0", normal="position") == MP_ERR_HIP               # inputs may alias inputs
    assert _downsample(_settings(), dst1=("dst0", LOW_BYTES)) == MP_ERR_HIP                     # adjacent is not overlapping
    assert _downsample(_settings(), picks=("dst0", LOW_BYTES)) == MP_ERR_HIP
    assert _upsample(_settings()) == MP_ERR_HIP
    assert _upsample(_settings(factor=4, phase=15, pick_mode=1)) == MP_ERR_HIP
    assert _upsample(_settings(), normal="position", normal_lo="position_lo") == MP_ERR_HIP
    assert _upsample(_settings(), out=("position", PLANE_BYTES)) == MP_ERR_HIP
    assert _upsample(_settings(), color_lo=("out", PLANE_BYTES)) == MP_ERR_HIP


def test_last_kernels_buffer_protocol():
    L = rs.lib()
    need = C.c_size_t(99)
    assert L.mpr_last_kernels(None, 0, C.byref(need)) == 0 and need.value == len("\n".join(rs.last_kernels()))
    assert L.mpr_last_kernels(None, 4, None) == MP_ERR_INVALID
    buf = C.create_string_buffer(b"xxxx", 4)
    assert L.mpr_last_kernels(buf, 1, None) == 0 and buf.raw[0] == 0  # cap 1: the terminating 0 alone
