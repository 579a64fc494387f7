"""GPU tests of the guided resampling (include/minipath_resample.h, minipath_amd.GuidedResampler).  Every comparison is on bit patterns
against the numpy model (tests/resample_model.py) with zero differences allowed: the copied planes carry NaNs, whose bits the
header specifies; no result of mpr_upsample here is a NaN.  Every buffer lies between sentinel guards, outputs are pre-filled with
the sentinel, and every call pins the kernel it reported.  The inputs are those of tests/resample_cases.py, which
tests/test_resample_cpu.py shows to reach every rule and every pixel class."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import resample as rs
from tests import resample_cases as tc, resample_model as m
from tests.conftest import TEAPOT
from tests.resample_model import F, bits

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
PAD = 4096
K_DOWN = {m.PICK_PHASE: "downsample_kernel<0>", m.PICK_NEAREST: "downsample_kernel<1>"}
K_UP = "upsample_kernel"


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module", autouse=True)
def _own_hip_errors_only(torch):
    """HIP's last-error state is per thread and sticky, and torch reads it after every kernel it launches.  Finalizers of what
    earlier test modules left behind can leave an error there whenever the garbage collector gets to them, and the next reader --
    a test here -- would be blamed for it.  So the garbage is collected now, and a call of the library, which clears the state
    before its launch, takes the error away (torch.empty launches nothing)."""
    import gc

    gc.collect()
    buf = torch.empty((3, 1, 1, 4), dtype=torch.float32, device="cuda")
    st = _settings(1, 1, 2)
    rs.check(rs.lib().mpr_downsample(0, C.byref(st), buf[0].data_ptr(), buf[1].data_ptr(), 0, None, None, buf[2].data_ptr(), None))
    torch.cuda.synchronize()


def _same(got, want, what):
    """zero differing words"""
    diff = bits(np.asarray(got)) != bits(np.asarray(want))
    assert int(diff.sum()) == 0, (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def _guarded(torch, a):
    """a copy of the host array of 4-byte words (or a buffer of sentinels for a shape) in the middle of a larger tensor of sentinels:
    (whole, view)"""
    shape = a if isinstance(a, tuple) else a.shape
    n = int(np.prod(shape))
    whole = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    view = whole[PAD:PAD + n]
    if not isinstance(a, tuple):
        view.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1)))
    return whole, view.view(shape)


def _guards_intact(torch, buffers):
    for name, (whole, _) in buffers.items():
        raw = whole.cpu().numpy()
        assert np.all(raw[:PAD] == SENTINEL) and np.all(raw[-PAD:] == SENTINEL), name


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _unchanged(dev, host):
    for k, a in host.items():
        assert np.array_equal(_words(dev[k][1]), bits(a)), ("input changed", k)


def _settings(W, H, f, pick_mode=m.PICK_PHASE, phase=0, k=0, sigma_plane=1.0):
    return rs.ResampleSettings(C.sizeof(rs.ResampleSettings), W, H, f, pick_mode, phase, float(k), float(sigma_plane))


# ---- mpr_downsample --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.down_cases(), ids=lambda c: "%dx%d_f%d_%s%d" % (*c[0], c[1], "phase" if c[2] == m.PICK_PHASE else "nearest", c[3]))
def test_downsample_matches_the_model(torch, case):
    """picks and the three destinations (position, normal and the int32 ids, NaN words included) equal the model in every word; every
    word of them is written (none keeps the sentinel they were filled with, which no expected word equals); guards and inputs are
    as they were"""
    (W, H), f, mode, phase = case
    c = tc.synthetic(W, H)
    want_picks, want_planes, _ = tc.downsampled(W, H, f, mode, phase)
    w, h = m.low_size(W, H, f)
    host = {k: c[k] for k in ("position", "normal", "ids")}
    src = {k: _guarded(torch, a) for k, a in host.items()}
    dst = {k + "_lo": _guarded(torch, (h, w, 4)) for k in host}
    picks = _guarded(torch, (h, w))
    st = _settings(W, H, f, mode, phase)
    rs.check(rs.lib().mpr_downsample(0, C.byref(st), src["position"][1].data_ptr(), src["normal"][1].data_ptr(), 3,
                                     rs.pointer_array([src[k][1].data_ptr() for k in host]), rs.pointer_array([dst[k + "_lo"][1].data_ptr() for k in host]),
                                     picks[1].data_ptr(), None))
    assert rs.last_kernels() == [K_DOWN[mode]]
    torch.cuda.synchronize()
    _same(_words(picks[1]), want_picks, "picks")
    for k, want in zip(host, want_planes):
        _same(_words(dst[k + "_lo"][1]), want, k + "_lo")
        assert not np.any(bits(want) == SENTINEL)  # so equality shows that every word was written
    assert not np.any(want_picks == SENTINEL)
    _guards_intact(torch, {**src, **dst, "picks": picks})
    _unchanged(src, host)


# ---- mpr_upsample ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", tc.FACTORS)
@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: "%dx%d" % s)
def test_upsample_matches_the_model(torch, size, f):
    """out equals the model in every word -- weighted means, nearest-tap fallbacks, holes and zero pixels alike --, on low planes
    taken as caller data (corrupted picks, colour alphas of 0, NaN points); every word of out is written; guards and inputs are as
    they were"""
    W, H = size
    c, u = tc.synthetic(W, H), tc.upsample_inputs(W, H, f)
    host = {"position": c["position"], "normal": c["normal"], "position_lo": u["position_lo"], "normal_lo": u["normal_lo"], "picks": u["picks"],
            "color_lo": u["color_lo"]}
    dev = {k: _guarded(torch, a) for k, a in host.items()}
    out = _guarded(torch, (H, W, 4))
    st = _settings(W, H, f, k=u["k"], sigma_plane=u["sigma_plane"])
    rs.check(rs.lib().mpr_upsample(0, C.byref(st), *[dev[k][1].data_ptr() for k in host], out[1].data_ptr(), None))
    assert rs.last_kernels() == [K_UP]
    torch.cuda.synchronize()
    assert not np.isnan(u["out"]).any() and not np.any(bits(u["out"]) == SENTINEL)
    _same(_words(out[1]), u["out"], "out")
    _guards_intact(torch, {**dev, "out": out})
    _unchanged(dev, host)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _render_planes(scene, cam, case):
    """the untiled feature planes of the case's frame, on the device"""
    fr = mp.FrameRenderer(scene, cam, mp.RenderSettings(case["tile"], case["spp"], case["res"], seed=case["seed"]))
    planes = fr.new_aov_planes(position=True)
    fr.render_aov_pass(planes)
    return {k: fr.untile_plane(t) for k, t in planes.items()}


def test_ambient_occlusion_at_half_resolution_end_to_end(torch, oracle):
    """the teapot at 48 x 32: the renderer's own planes through GuidedResampler.downsample, SecondaryVisibility at 24 x 16 and
    GuidedResampler.upsample with the shipped weights give the model's planes over the oracle's occlusion query in every word, for
    two phases with different picks; then the result goes through TemporalAccumulator and AtrousDenoiser at full resolution as a
    colour: shapes, alpha classes, finite values"""
    c = tc.E2E
    W, H = c["res"]
    e = tc.e2e_frame(oracle, TEAPOT)
    ctx = mp.Context(0)
    scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, ctx))
    cam = tc.secondary_cases.e2e_camera(mp, c)
    planes = _render_planes(scene, cam, c)
    torch.cuda.synchronize()
    for k in ("position", "normal", "ids"):
        assert np.array_equal(bits(planes[k].cpu().numpy()), bits(e["planes"][k])), ("the renderer's plane differs from the oracle's", k)
    resampler = mp.GuidedResampler(c["res"], c["factor"])
    assert resampler.low_resolution == (24, 16)
    assert (resampler.sigma_normal_pow2, resampler.sigma_plane) == (rs.DEFAULT_SIGMA_NORMAL_POW2, rs.DEFAULT_SIGMA_PLANE)
    vis = mp.SecondaryVisibility(scene, resampler.low_resolution, batch=c["batch"])
    acc = mp.TemporalAccumulator(c["res"], 0)
    dn = mp.AtrousDenoiser(c["res"], 0)
    all_picks = []
    for phase in (c["phase"], c["second_phase"]):
        lo = tc.e2e_low(oracle, TEAPOT, phase)
        want, _ = tc.e2e_up(oracle, TEAPOT, phase, rs.DEFAULT_SIGMA_NORMAL_POW2, rs.DEFAULT_SIGMA_PLANE)
        position_lo, normal_lo, ids_lo = resampler.downsample(planes["position"], planes["normal"], planes["ids"], phase=phase)
        assert resampler.last_kernels() == [K_DOWN[m.PICK_PHASE]]
        ao_lo, _ = vis.ambient_occlusion(position_lo, normal_lo, cam, c["samples"], c["radius"], seed=c["ao_seed"], bias=c["bias"])
        out = resampler.upsample(ao_lo, planes["position"], planes["normal"])
        assert resampler.last_kernels() == [K_UP]
        torch.cuda.synchronize()
        _same(_words(resampler.picks), lo["picks"], ("picks", phase))
        for got, k in ((position_lo, "position_lo"), (normal_lo, "normal_lo"), (ids_lo, "ids_lo"), (ao_lo, "ao_lo")):
            _same(_words(got), lo[k], (k, phase))
        assert ids_lo.dtype == planes["ids"].dtype and tuple(ids_lo.shape) == (16, 24, 4)
        _same(_words(out), want, ("out", phase))
        all_picks.append(_words(resampler.picks).copy())
        # the hand-over: a colour for the temporal stage and the denoiser
        out_host = out.cpu().numpy()
        hit = planes["position"].cpu().numpy()[..., 3] > 0
        assert hit.sum() >= 500 and (~hit).sum() >= 32
        assert np.all(out_host[~hit] == 0) and np.all(out_host[..., 3][hit] == 1)  # no holes on this frame
        acc_out, var = acc.accumulate(out, planes["position"], planes["normal"], planes["ids"], mp.TemporalAccumulator.view_of(cam, c["res"]))
        clean, _ = dn.denoise(acc_out, planes["normal"], variance=var)
        torch.cuda.synchronize()
        for name, t in (("accumulated", acc_out), ("denoised", clean)):
            a = t.cpu().numpy()
            assert a.shape == (H, W, 4) and a.dtype == F, name
            assert np.all(np.isfinite(a)) and a.min() >= 0 and a.max() <= 1, (name, float(a.min()), float(a.max()))
            assert np.all(a[..., 3][hit] == 1) and np.all(a[..., 3][~hit] == 0), name
    assert (all_picks[0] != all_picks[1]).sum() >= 32
    assert float(acc.history_length().max()) == 2  # the second frame found history
    for k in ("position", "normal", "ids"):
        assert np.array_equal(bits(planes[k].cpu().numpy()), bits(e["planes"][k])), ("a plane was changed", k)


def test_the_driver_checks_its_planes(torch):
    r = mp.GuidedResampler((8, 5), 3)
    assert r.low_resolution == (3, 2)
    good = torch.zeros((5, 8, 4), device="cuda")
    ids = torch.zeros((5, 8, 4), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        r.upsample(torch.zeros((2, 3, 4), device="cuda"), good, good)  # no picks yet
    for bad in (good[:, :4], good.cpu(), good.double(), torch.zeros((8, 5, 4), device="cuda"), None):
        with pytest.raises(ValueError):
            r.downsample(bad, good)
        with pytest.raises(ValueError):
            r.downsample(good, good, bad)
    with pytest.raises(ValueError):
        r.downsample(ids, good)  # the guides are float planes
    with pytest.raises(ValueError):
        r.downsample(good, good, ids, ids, ids)
    with pytest.raises(ValueError):
        r.downsample(good, good, pick="mean")
    with pytest.raises(mp.MinipathError):
        r.downsample(good, good, phase=9)
    for args in (dict(factor=1), dict(factor=5), dict(sigma_plane=0.0), dict(sigma_normal_pow2=9)):
        with pytest.raises(mp.MinipathError):
            mp.GuidedResampler((8, 5), **args)
    position_lo, normal_lo, ids_lo = r.downsample(good, good, ids, pick="nearest")  # all misses
    assert r.last_kernels() == [K_DOWN[m.PICK_NEAREST]]
    for bad in (good, torch.zeros((2, 3, 4), dtype=torch.int32, device="cuda")):
        with pytest.raises(ValueError):
            r.upsample(bad, good, good)
    out = r.upsample(torch.ones((2, 3, 4), device="cuda"), good, good)
    torch.cuda.synchronize()
    assert tuple(position_lo.shape) == (2, 3, 4) and ids_lo.dtype == torch.int32 and tuple(out.shape) == (5, 8, 4)
    assert np.all(_words(r.picks) == m.PICK_NONE) and float(out.abs().max()) == 0 and float(position_lo.abs().max()) == 0
