"""CPU tests of the temporal reprojection: the numpy model (tests/temporal_model.py, the restatement of include/minipath_temporal.h
that the GPU tests compare bits against) against the renderer's own camera and on hand-built frames, the conditions on the inputs of
the GPU cases (tests/temporal_cases.py), the usefulness of the shipped defaults, and what libminipath_temporal.so decides before its
first HIP call -- every refusal, the struct size, the symbols -- through the built library without touching a GPU."""
import collections
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import temporal as tp
from tests import denoise_model, temporal_cases as tc, temporal_model as m
from tests.conftest import ROOT, TEAPOT
from tests.temporal_model import F, bits

MP_ERR_INVALID = 1
SENTINEL = 0x5A5A5A5A
INF, NAN = float("inf"), float("nan")


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the view against the renderer ---------------------------------------------------------------------------------------------
def test_view_of_is_the_models_arithmetic():
    """TemporalAccumulator.view_of and the model's view_of give the same 15 floats for the same camera, and the oracle's camera agrees"""
    from oracle import pyoracle as po

    res = (96, 64)
    for i in range(2):
        cam = tc.e2e_camera(mp, i)
        center, forward, up, right = cam.center_forward_up_right()
        want = m.view_of(center, forward, up, right, cam.focal_length, cam.build_sampler(res).as_array()[12], res).floats()
        got = np.frombuffer(bytes(mp.TemporalAccumulator.view_of(cam, res)), F)
        assert _same(got, want) and got.size == 15
        eye, at = tc.E2E["cameras"][i]
        assert _same(tc.oracle_view(po, tc.oracle_camera(po, eye, at), res)[0].floats(), want)
    assert want[12] == F(50e-3) / (F(24e-3) / F(64)) and want[13] == 47.5 and want[14] == 31.5


def test_projection_against_the_renderer():
    """the oracle's planes of the teapot through a pinhole at 96 x 64 x 8 spp: the mean hit point of every fully covered pixel (x, y),
    projected through the SAME camera, lands within the pixel's jitter of (x, y) -- the sign and offset conventions of mpt_view are
    those of sample_ray"""
    from oracle import pyoracle as po

    e = tc.e2e_model(po, TEAPOT)
    for planes, view in zip(e["planes"], e["views"]):
        pos = planes["position"]
        full = pos[..., 3] == 1
        assert full.sum() > 1000
        a, u, v = m.project(view, pos[..., :3])
        yy, xx = np.mgrid[0:pos.shape[0], 0:pos.shape[1]]
        assert np.all(a[full] > 0)
        du, dv = np.abs(u - xx)[full], np.abs(v - yy)[full]
        print("largest |u - x|, |v - y|:", du.max(), dv.max())
        assert du.max() <= 0.5 + 1e-3 and dv.max() <= 0.5 + 1e-3
        assert du.max() > 0.05 and dv.max() > 0.05  # jittered samples: the means are not the pixel centres


# ---- properties of the model ---------------------------------------------------------------------------------------------------
W, H = 7, 5
BASE = dict(sigma_position=0.5, normal_min=0.9, max_history=INF, alpha_color=0.0, alpha_moments=0.0, min_variance_history=0.0)


def _flat_frame(seed, shift=(0, 0)):
    """a frame of points (x + shift, y + shift, 1) facing the camera of tc.exact_view, all hits, with a random colour"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    pos = np.stack([xx - F(W - 1) * F(0.5) + shift[0], yy - F(H - 1) * F(0.5) + shift[1], np.ones((H, W)), np.ones((H, W))], -1).astype(F)
    nrm = np.zeros((H, W, 4), F)
    nrm[..., 2], nrm[..., 3] = -1, 1
    ids = np.zeros((H, W, 4), np.uint32)
    ids[..., 3] = 1
    return {"color": rng.random((H, W, 4)).astype(F), "position": pos, "normal": nrm, "ids": ids}


def _reproject(cur, prev, hist, mom, view=None, **kw):
    st = dict(BASE)
    variance_in = kw.pop("variance_in", None)
    st.update(kw)
    return m.reproject(cur["color"], cur["position"], cur["normal"], cur["ids"], view or tc.exact_view(W, H), prev["position"], prev["normal"],
                       prev["ids"], hist, mom, variance_in=variance_in, want_info=True, **st)


def test_identical_aligned_frames_give_the_running_mean():
    """integer-aligned identical geometry and alpha_* = 0: out is the mean of the colours so far and N counts 1, 2, 3, ... up to max_history"""
    frames = [_flat_frame(s) for s in range(6)]
    out, mom = m.reset(frames[0]["color"], frames[0]["position"])
    assert np.all(mom[..., 2] == 1) and _same(out, frames[0]["color"])
    total = frames[0]["color"][..., :3].astype(np.float64)
    lum = [m.luminance(frames[0]["color"]).astype(np.float64)]
    for n, f in enumerate(frames[1:], start=2):
        out, mom, var, info = _reproject(f, frames[n - 2], out, mom, max_history=4.0)
        assert np.all(info["pixel"] == m.P_HISTORY) and np.all(info["kept"] == 1)  # the one tap with weight 1
        assert np.all(mom[..., 2] == min(n, 4))
        if n <= 4:
            total += f["color"][..., :3]
            lum.append(m.luminance(f["color"]).astype(np.float64))
            assert np.max(np.abs(out[..., :3] - total / n)) <= 4e-7 * n
            assert np.max(np.abs(mom[..., 0] - np.mean(lum, 0))) <= 1e-6 * n
            assert np.max(np.abs(var[..., 0] - np.maximum(np.mean(np.square(lum), 0) - np.mean(lum, 0) ** 2, 0))) <= 2e-5
        assert _same(out[..., 3], f["color"][..., 3])


def _one_pixel_case():
    """the centre pixel of a flat frame lands at (3.5, 2.5) of an identical previous frame: four valid taps of weight 1/4"""
    prev = _flat_frame(1)
    cur = _flat_frame(2, shift=(0.5, 0.5))
    out, mom = m.reset(prev["color"], prev["position"])
    return cur, prev, out, mom


def test_each_reject_class_alone():
    cur, prev, hist, mom = _one_pixel_case()
    y, x = 2, 3
    *_, info = _reproject(cur, prev, hist, mom, sigma_position=1.0)
    assert info["pixel"][y, x] == m.P_HISTORY and info["kept"][y, x] == 4 and np.all(info["tap"][y, x] == m.KEPT)
    assert info["x0"][y, x] == 3 and info["y0"][y, x] == 2

    def after(change, **kw):
        c, p = {k: v.copy() for k, v in cur.items()}, {k: v.copy() for k, v in prev.items()}
        change(c, p)
        out, mo, var, inf = _reproject(c, p, hist, mom, sigma_position=1.0, **kw)
        assert _same(out[y, x], c["color"][y, x])  # no history: the colour passes through
        l = m.luminance(c["color"])[y, x]
        assert _same(mo[y, x], np.array([l, l * l, 1, 0], F))
        return inf["pixel"][y, x], set(inf["tap"][y, x].tolist())

    def off_screen(c, p): c["position"][y, x, 0] = 100
    def behind(c, p): c["position"][y, x, 2] = -1
    def other_instance(c, p): c["ids"][y, x, 1] = 5
    def other_material(c, p): c["ids"][y, x, 2] = 5
    def other_prim(c, p): c["ids"][y, x, 0] = 5
    def moved(c, p): c["position"][y, x, 2] = 3; c["position"][y, x, :2] *= 3  # noqa: E702  the same (u, v), another depth
    def turned(c, p): c["normal"][y, x, :3] = (1, 0, 0)
    def prev_missed(c, p): p["position"][2:4, 3:5, 3] = 0

    assert after(off_screen) == (m.P_OFFSCREEN, {m.T_NONE})
    assert after(behind) == (m.P_BEHIND, {m.T_NONE})
    assert after(other_instance) == (m.P_NO_TAP_KEPT, {m.T_IDS})
    assert after(other_material) == (m.P_NO_TAP_KEPT, {m.T_IDS})
    assert after(other_prim, match_prim=True) == (m.P_NO_TAP_KEPT, {m.T_IDS})
    assert after(moved) == (m.P_NO_TAP_KEPT, {m.T_POSITION})
    assert after(turned) == (m.P_NO_TAP_KEPT, {m.T_NORMAL})
    assert after(prev_missed) == (m.P_NO_TAP_KEPT, {m.T_PREV_MISS})
    # without MATCH_PRIM another triangle of the same instance and material is history
    c = {k: v.copy() for k, v in cur.items()}
    other_prim(c, None)
    assert _reproject(c, prev, hist, mom, sigma_position=1.0)[3]["kept"][y, x] == 4


def test_a_zero_weight_tap_is_never_read():
    """fx == 0: the taps i = 1 have weight exactly 0; NaN planted in their history does not reach the result"""
    prev = _flat_frame(1)
    cur = _flat_frame(2, shift=(0.0, 0.5))  # lands on (x, y + 0.5)
    hist, mom = m.reset(prev["color"], prev["position"])
    clean = _reproject(cur, prev, hist, mom, sigma_position=2.0)
    y, x = 1, 2
    assert clean[3]["tap"][y, x].tolist() == [m.KEPT, m.T_ZERO_WEIGHT, m.KEPT, m.T_ZERO_WEIGHT]
    hist2, mom2 = hist.copy(), mom.copy()
    hist2[y:y + 2, x + 1], mom2[y:y + 2, x + 1] = NAN, NAN
    dirty = _reproject(cur, prev, hist2, mom2, sigma_position=2.0)
    for a, b in zip(clean[:3], dirty[:3]):
        assert _same(a[y, x], b[y, x]) and np.all(np.isfinite(b[y, x]))
    assert np.isnan(dirty[0][y, x + 1]).any()  # the neighbour, for which it is the tap of weight 1/2, does see it


def test_variance_falls_back_below_min_variance_history():
    cur, prev, hist, mom = _one_pixel_case()
    mom[..., 2] = np.arange(H * W).reshape(H, W) % 5 + 1  # histories of 1..5 frames
    vin = np.full((H, W, 4), 7, F)
    vin[..., 0] = np.random.default_rng(3).random((H, W))
    own = _reproject(cur, prev, hist, mom, sigma_position=1.0, min_variance_history=4.0)
    mixed = _reproject(cur, prev, hist, mom, sigma_position=1.0, min_variance_history=4.0, variance_in=vin)
    N = mixed[1][..., 2]
    young = N < 4
    assert 0 < young.sum() < young.size
    assert _same(mixed[2][..., 0][young], vin[..., 0][young]) and _same(mixed[2][..., 0][~young], own[2][..., 0][~young])
    m1, m2 = own[1][..., 0], own[1][..., 1]
    assert _same(own[2][..., 0], m.mx(m2 - (m1 * m1).astype(F), 0)) and np.all(mixed[2][..., 1:] == 0)
    for r in (own, mixed):
        assert _same(r[0], own[0]) and _same(r[1], own[1])  # variance_in changes the variance only


# ---- the inputs of the GPU cases -------------------------------------------------------------------------------------------------
def test_the_synthetic_cases_reach_every_rule():
    """over the sizes of the GPU test: every way a pixel and a tap can end, the four edge landings, exact integer landings"""
    pixels, taps, edges = collections.Counter(), collections.Counter(), collections.Counter()
    for (w, h), general in [(s, False) for s in tc.SIZES] + [((37, 23), True), ((64, 16), True)]:
        case = tc.synthetic(w, h, general)
        for match_prim in (False, True):
            out, mom, var, info = tc.model_on(case, tc.synthetic_settings(1.0, 0.0, match_prim), True, want_info=True)
            pixels.update(info["pixel"].ravel().tolist())
            taps.update(info["tap"].ravel().tolist())
            tapped = info["pixel"] >= m.P_NO_TAP_KEPT
            edges["x0=-1"] += int((info["x0"][tapped] == -1).sum())
            edges["x0=W-1"] += int((info["x0"][tapped] == w - 1).sum())
            edges["y0=-1"] += int((info["y0"][tapped] == -1).sum())
            edges["y0=H-1"] += int((info["y0"][tapped] == h - 1).sum())
            uu, vv = info["u"][tapped], info["v"][tapped]
            edges["integer u and v"] += int(((uu == np.floor(uu)) & (vv == np.floor(vv))).sum())
            edges["integer u"] += int(((uu == np.floor(uu)) & (vv != np.floor(vv))).sum())
            edges["integer v"] += int(((uu != np.floor(uu)) & (vv == np.floor(vv))).sum())
            edges["four kept"] += int((info["kept"] == 4).sum())
    print(pixels, taps, edges)
    assert all(pixels[k] >= 50 for k in range(5)) and all(taps[k] >= 50 for k in range(8))
    assert all(n >= 8 for n in edges.values()), edges


def test_the_two_camera_case_holds_every_class():
    """at least 8 pixels of each class between the two cameras of the GPU end-to-end case: it cannot pass emptily"""
    from oracle import pyoracle as po

    e = tc.e2e_model(po, TEAPOT)
    counts = {k: int(v.sum()) for k, v in m.classes(e["info"]).items()}
    print(counts)
    assert set(counts) == {"four_taps", "one_to_three_taps", "ids", "position", "normal", "offscreen", "miss"}
    assert all(n >= tc.E2E_MIN_PER_CLASS for n in counts.values()), counts
    assert len(np.unique(e["planes"][1]["ids"][..., 1][e["planes"][1]["ids"][..., 3] == 1])) == 2  # both instances in view


# ---- usefulness ------------------------------------------------------------------------------------------------------------------
def test_the_defaults_help_on_a_moving_camera():
    """the oracle's path-traced teapot (max_depth 3, 96 x 64, 8 spp), 8 frames with seeds s + i from a camera that moves 0.05 to the
    right per frame (two thirds of a pixel at the teapot), accumulated by the model with the defaults TemporalAccumulator ships: the
    last accumulated frame is closer to the 512-spp frame of the last camera than the last noisy frame is, and filtered by the
    a-trous model (the denoiser's defaults, the temporal variance) it is closer than the last noisy frame filtered alone"""
    from oracle import pyoracle as po
    from tests import aov_pass_model

    w, h, spp, seed, frames = 96, 64, 8, 0x5EED, 8
    b = po.Bvh.from_obj(TEAPOT)
    d = {k: v.default for k, v in inspect.signature(mp.TemporalAccumulator.__init__).parameters.items()}
    acc = m.Accumulator(**{k: d[k] for k in ("sigma_position", "normal_min", "max_history", "alpha_color", "alpha_moments",
                                             "min_variance_history", "match_prim")})
    for i in range(frames):
        cam = tc.oracle_camera(po, (0.05 * i, 2.0, 10.0), (0.05 * i, 1.5, 0.0), f_number=4.8, focus_distance=10.0)
        view, smp = tc.oracle_view(po, cam, (w, h))
        noisy = b.render_image_paths_mt(smp, w, h, spp, seed + i, 3, tile=32)[0]
        guides = aov_pass_model.planes(po, b.intersect, smp, w, spp, seed + i, (0, 0, w, h))
        out, var = acc.accumulate(noisy, guides["position"], guides["normal"], guides["ids"], view)
    ref = b.render_image_paths_mt(smp, w, h, 512, seed, 3, tile=32)[0]
    dd = {k: v.default for k, v in inspect.signature(mp.AtrousDenoiser.__init__).parameters.items()}
    kw = dict(iterations=dd["iterations"], k=dd["sigma_normal_pow2"], sigma_depth=dd["sigma_depth"], sigma_luminance=dd["sigma_luminance"])
    alone = denoise_model.atrous(noisy, guides["normal"], **kw)
    both = denoise_model.atrous(out, guides["normal"], variance=var, **kw)[0]

    def mse(a):
        return float(np.mean((a[..., :3].astype(np.float64) - ref[..., :3]) ** 2))
    N = acc.prev["moments"][..., 2]
    print("mse against 512 spp: noisy", mse(noisy), "accumulated", mse(out), "a-trous alone", mse(alone), "accumulated + a-trous", mse(both),
          "mean history at hits", float(N[N > 0].mean()))
    assert mse(out) < mse(noisy)
    assert mse(both) < mse(alone)


# ---- the library, before its first HIP call --------------------------------------------------------------------------------------
LW, LH = 6, 5
NO_DEVICE = 1 << 20  # no such GPU: were a call accepted by mistake, the runtime would refuse the device and nothing would be launched
INPUTS = ("color", "position", "normal", "ids", "variance_in", "prev_position", "prev_normal", "prev_ids", "hist_color", "hist_moments")
OUTPUTS = ("out", "moments_out", "variance_out")
ARGS = INPUTS + OUTPUTS


def _settings(**kw):
    v = dict(struct_size=C.sizeof(tp.TemporalSettings), width=LW, height=LH, flags=0, sigma_position=0.01, normal_min=0.9, max_history=32.0,
             alpha_color=0.2, alpha_moments=0.2, min_variance_history=4.0)
    v.update(kw)
    return tp.TemporalSettings(**v)


def test_struct_sizes_and_symbols():
    L = tp.lib()
    assert L.mpt_settings_size() == C.sizeof(tp.TemporalSettings) == 40
    assert C.sizeof(tp.TemporalView) == 60
    header = open(os.path.join(ROOT, "include", "minipath_temporal.h")).read()
    import re
    declared = set(re.findall(r"\b(mpt_[a-z_]+)\s*\(", header.split("#ifndef MINIPATH_TEMPORAL_H")[1]))
    assert declared == set(tp.SIGNATURES) and all(hasattr(L, n) for n in declared)
    assert mp.TemporalAccumulator is tp.TemporalAccumulator
    assert L.mpt_check_settings(C.byref(_settings())) == 0
    assert L.mpt_check_settings(C.byref(_settings(sigma_position=INF, max_history=INF, alpha_color=0.0, alpha_moments=1.0, min_variance_history=0.0,
                                                  normal_min=-1.0, flags=1, width=1 << 20, height=1 << 20))) == 0


def _buffers():
    # one allocation, so that "overlapping" can be asked for: plane k at word offset k * 2 * plane
    plane = LH * LW * 4
    whole = np.full(len(ARGS) * 2 * plane, SENTINEL, np.uint32)
    return whole, {k: whole[i * 2 * plane:].ctypes.data for i, k in enumerate(ARGS)}


def _call_reproject(st, device=NO_DEVICE, view=True, **replace):
    whole, ptr = _buffers()
    for k, v in replace.items():
        ptr[k] = None if v is None else (ptr[v[0]] + v[1] if isinstance(v, tuple) else ptr[v])
    before = tp.last_kernels()
    vw = tp.TemporalView()
    rc = tp.lib().mpt_reproject(device, None if st is None else C.byref(st), C.byref(vw) if view else None, *[ptr[k] for k in ARGS], None)
    assert tp.last_kernels() == before  # nothing was launched
    assert np.all(whole == SENTINEL)    # nothing was written (host memory here: a launch would not even get this far)
    return rc


BAD_SETTINGS = [dict(width=0), dict(height=0), dict(width=0, height=0), dict(width=(1 << 20) + 1), dict(height=(1 << 20) + 1),
                dict(sigma_position=0.0), dict(sigma_position=-1.0), dict(sigma_position=NAN), dict(normal_min=INF), dict(normal_min=-INF),
                dict(normal_min=NAN), dict(max_history=0.5), dict(max_history=NAN), dict(max_history=-INF), dict(alpha_color=-0.1),
                dict(alpha_color=1.5), dict(alpha_color=NAN), dict(alpha_moments=-0.1), dict(alpha_moments=1.5), dict(alpha_moments=NAN),
                dict(min_variance_history=-1.0), dict(min_variance_history=NAN), dict(struct_size=0), dict(struct_size=36), dict(flags=2),
                dict(flags=0x80000001)]
PLANE_BYTES = LH * LW * 16
BAD_ARGS = ([{k: None} for k in ARGS if k not in ("variance_in", "variance_out")]
            + [dict(variance_out=None), dict(device=-1), dict(settings=None), dict(view=False)]
            + [{o: i} for o in OUTPUTS for i in INPUTS]                                     # an output equal to an input
            + [dict(moments_out="out"), dict(variance_out="out"), dict(variance_out="moments_out")]
            + [dict(out=("color", 16)), dict(out=("hist_color", PLANE_BYTES - 16)), dict(color=("out", PLANE_BYTES - 16)),
               dict(moments_out=("out", 16)), dict(variance_out=("prev_ids", -16))])          # partial overlaps


def _id(d):
    return ",".join(f"{k}={v}" for k, v in d.items())


@pytest.mark.parametrize("bad", BAD_SETTINGS, ids=_id)
def test_reproject_refuses_settings(bad):
    assert _call_reproject(_settings(**bad)) == MP_ERR_INVALID
    assert tp.lib().mpt_last_error()
    assert tp.lib().mpt_check_settings(C.byref(_settings(**bad))) == MP_ERR_INVALID


@pytest.mark.parametrize("bad", BAD_ARGS, ids=_id)
def test_reproject_refuses_arguments(bad):
    bad = dict(bad)
    st = None if "settings" in bad and bad.pop("settings") is None else _settings()
    assert _call_reproject(st, **bad) == MP_ERR_INVALID
    assert tp.lib().mpt_last_error()


def test_reproject_accepts_what_is_not_refused():
    """the same call with nothing wrong, and its legal variations, get as far as the device (which does not exist): MP_ERR_HIP"""
    MP_ERR_HIP = 4
    assert _call_reproject(_settings()) == MP_ERR_HIP
    assert _call_reproject(_settings(), variance_in=None) == MP_ERR_HIP                       # variance_out alone is allowed
    assert _call_reproject(_settings(), variance_in=None, variance_out=None) == MP_ERR_HIP
    assert _call_reproject(_settings(), out=("color", PLANE_BYTES)) == MP_ERR_HIP               # adjacent is not overlapping
    assert _call_reproject(_settings(), position="color", prev_normal="prev_position") == MP_ERR_HIP  # inputs may alias inputs


RESET_ARGS = ("color", "position", "out", "moments_out")


@pytest.mark.parametrize("bad", [dict(color=None), dict(position=None), dict(out=None), dict(moments_out=None), dict(width=0), dict(height=0),
                                 dict(width=(1 << 20) + 1), dict(device=-1), dict(out="color"), dict(out="position"), dict(moments_out="color"),
                                 dict(moments_out="position"), dict(moments_out="out"), dict(out=("color", 16)), dict(moments_out=("out", -16))],
                         ids=_id)
def test_reset_refuses(bad):
    whole, ptr = _buffers()
    for k in RESET_ARGS:
        if k in bad:
            v = bad[k]
            ptr[k] = None if v is None else (ptr[v[0]] + v[1] if isinstance(v, tuple) else ptr[v])
    before = tp.last_kernels()
    rc = tp.lib().mpt_reset(bad.get("device", NO_DEVICE), bad.get("width", LW), bad.get("height", LH), *[ptr[k] for k in RESET_ARGS], None)
    assert rc == MP_ERR_INVALID and tp.lib().mpt_last_error()
    assert tp.last_kernels() == before and np.all(whole == SENTINEL)


def test_last_kernels_buffer_protocol():
    L = tp.lib()
    need = C.c_size_t(99)
    assert L.mpt_last_kernels(None, 0, C.byref(need)) == 0 and need.value == len("\n".join(tp.last_kernels()))
    assert L.mpt_last_kernels(None, 4, None) == MP_ERR_INVALID
    buf = C.create_string_buffer(b"xxxx", 4)
    assert L.mpt_last_kernels(buf, 1, None) == 0 and buf.raw[0] == 0  # cap 1: the terminating 0 alone
