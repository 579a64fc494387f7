"""GPU tests of the secondary rays (include/minipath_secondary.h, minipath_amd.SecondaryVisibility).  Every comparison is on f32 bit
patterns against the numpy model (tests/secondary_model.py) with zero differences allowed; no result here is a NaN.  Every buffer
lies between sentinel guards, outputs are pre-filled with the sentinel, and every call pins the kernel it reported.  The inputs are
those of tests/secondary_cases.py, which tests/test_secondary_cpu.py shows to reach every rule and every pixel class."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import secondary as sv
from tests import secondary_cases as tc, secondary_model as m
from tests.conftest import TEAPOT
from tests.secondary_model import F, bits

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
PAD = 4096
K_GEN = {m.MODE_AO: "secondary_rays_kernel<0>", m.MODE_SUN: "secondary_rays_kernel<1>"}
K_RESOLVE = {False: "resolve_kernel<false>", True: "resolve_kernel<true>"}


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
    buf = torch.empty((2, 1, 1, 4), dtype=torch.float32, device="cuda")
    st = _settings(1, 1, dict(mode=m.MODE_AO, radius=1.0, bias=0.0), 1, 0)
    sv.check(sv.lib().mps_resolve(0, C.byref(st), buf[0].data_ptr(), buf[0].data_ptr(), buf[1].data_ptr(), None, None))
    torch.cuda.synchronize()


def _same(got, want, what):
    """zero differing words"""
    diff = bits(np.asarray(got)) != bits(np.asarray(want))
    assert int(diff.sum()) == 0, (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def _guarded(torch, a, dtype=None):
    """a copy of the host array (or a buffer of sentinels for a shape) in the middle of a larger tensor of sentinels: (whole, view).
    4-byte elements, or bytes with dtype = torch.uint8"""
    shape = a if isinstance(a, tuple) else a.shape
    n = int(np.prod(shape))
    if dtype is None:
        whole = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    else:
        whole = torch.full((PAD + n + PAD,), SENTINEL & 0xFF, dtype=dtype, device="cuda")
    view = whole[PAD:PAD + n]
    if not isinstance(a, tuple):
        host = np.ascontiguousarray(a)
        view.copy_(torch.from_numpy(host.reshape(-1) if dtype is not None else host.view(np.int32).reshape(-1)))
    return whole, view.view(shape)


def _guards_intact(torch, buffers):
    for name, (whole, _) in buffers.items():
        raw = whole.cpu().numpy()
        s = SENTINEL if raw.dtype.itemsize == 4 else SENTINEL & 0xFF
        assert np.all(raw[:PAD] == s) and np.all(raw[-PAD:] == s), name


def _host(t):
    return t.cpu().numpy().view(F)


def _settings(w, h, mode_kw, batch, sample_begin, flags=0, sample_count=tc.SAMPLE_COUNT, seed=tc.SEED, eye=tc.EYE):
    st = sv.SecondarySettings(C.sizeof(sv.SecondarySettings), w, h, mode_kw["mode"], flags, sample_count, sample_begin, batch, seed)
    st.eye[:], st.light[:] = eye, mode_kw.get("light", (0.0, 0.0, 1.0))
    st.radius, st.bias, st.spread = mode_kw["radius"], mode_kw["bias"], mode_kw.get("spread", 0.0)
    return st


# ---- mps_generate ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", tc.BATCHES, ids=lambda b: "B%d_from%d" % b)
@pytest.mark.parametrize("mode_name", list(tc.MODES))
@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: "%dx%d" % s)
def test_generate_matches_the_model(torch, oracle, size, mode_name, batch):
    """all seven arrays equal the model in every word, the zeros and codes of none and unlit rays included; nothing but the seven
    arrays is written (mps_generate is not given `occluded`, which stays all sentinel), and the planes are only read"""
    (w, h), (B, begin) = size, batch
    case, kw = tc.synthetic(w, h), tc.MODES[mode_name]
    want, info = tc.generated(oracle, w, h, mode_name, B, begin)
    planes = {k: _guarded(torch, case[k]) for k in ("position", "normal")}
    rays = {k: _guarded(torch, (B * h * w,)) for k in m.RAY_ARRAYS}
    occluded = _guarded(torch, (B * h * w,), torch.uint8)  # the query's output, allocated beside the rays as the driver does
    st = _settings(w, h, kw, B, begin)
    sv.check(sv.lib().mps_generate(0, C.byref(st), planes["position"][1].data_ptr(), planes["normal"][1].data_ptr(),
                                   *[rays[k][1].data_ptr() for k in m.RAY_ARRAYS], None))
    assert sv.last_kernels() == [K_GEN[kw["mode"]]]
    torch.cuda.synchronize()
    for k in m.RAY_ARRAYS:
        _same(_host(rays[k][1]), want[k], k)
    _guards_intact(torch, {**planes, **rays, "occluded": occluded})
    assert np.all(occluded[1].cpu().numpy() == SENTINEL & 0xFF)
    for k in planes:
        assert np.array_equal(bits(_host(planes[k][1])), bits(case[k])), ("input changed", k)
    # what the codes say, from what the GPU wrote
    tmax = _host(rays["tmax"][1]).reshape(B, h, w)
    assert np.array_equal(tmax[0] == 0, info["pixel"] <= m.P_NONE_NORMAL) and np.array_equal(tmax[0] == -1, info["pixel"] == m.P_UNLIT)


# ---- mps_resolve -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_out", [False, True], ids=["noout", "out"])
@pytest.mark.parametrize("accumulate", [False, True], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: "%dx%d" % s)
def test_resolve_matches_the_model(torch, size, B, accumulate, with_out):
    """random answers under every tmax code (0, -1, -0, 0.5, +inf, NaN, -2): counts and out are the model's bits; a counts plane of
    sentinels is fully overwritten without the flag, and with it .z and .w (NaN here) are replaced by zeros"""
    w, h = size
    r = tc.resolve_inputs(w, h, B)
    dev = {"tmax": _guarded(torch, r["tmax"]), "occluded": _guarded(torch, r["occluded"], torch.uint8)}
    outs = {"counts": _guarded(torch, r["counts"] if accumulate else (h, w, 4)), "out": _guarded(torch, (h, w, 4))}
    st = _settings(w, h, tc.MODES["ao"], B, 0, flags=sv.MPS_FLAG_ACCUMULATE if accumulate else 0)
    sv.check(sv.lib().mps_resolve(0, C.byref(st), dev["tmax"][1].data_ptr(), dev["occluded"][1].data_ptr(), outs["counts"][1].data_ptr(),
                                  outs["out"][1].data_ptr() if with_out else None, None))
    assert sv.last_kernels() == [K_RESOLVE[with_out]]
    torch.cuda.synchronize()
    want_counts, want_out = m.resolve(r["tmax"], r["occluded"], (h, w), B, counts=r["counts"] if accumulate else None, want_out=with_out)
    _same(_host(outs["counts"][1]), want_counts, "counts")
    if with_out:
        _same(_host(outs["out"][1]), want_out, "out")
    else:
        assert np.all(outs["out"][1].cpu().numpy() == SENTINEL)
    _guards_intact(torch, {**dev, **outs})
    assert np.array_equal(bits(_host(dev["tmax"][1])), bits(r["tmax"])) and np.array_equal(dev["occluded"][1].cpu().numpy(), r["occluded"])


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _render_planes(scene, cam, case):
    """the untiled feature planes of the case's frame, on the device"""
    fr = mp.FrameRenderer(scene, cam, mp.RenderSettings(case["tile"], case["spp"], case["res"], seed=case["seed"]))
    planes = fr.new_aov_planes(position=True)
    fr.render_aov_pass(planes)
    return {k: fr.untile_plane(t) for k, t in planes.items()}


def _count(cls, keys):
    return {k: int(cls[k].sum()) for k in keys}


def test_ambient_occlusion_end_to_end(torch, oracle):
    """the teapot at 48 x 32: the renderer's own planes -- bit-equal to the oracle's -- through SecondaryVisibility.ambient_occlusion
    with 8 samples in batches of 3 + 3 + 2 and again in one batch of 8 give the model's counts over the oracle's occlusion query in
    every word, and the same plane both times; the frame holds every pixel class"""
    c = tc.E2E_AO
    e = tc.e2e_ao(oracle, TEAPOT)
    ctx = mp.Context(0)
    scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, ctx))
    cam = tc.e2e_camera(mp, c)
    planes = _render_planes(scene, cam, c)
    torch.cuda.synchronize()
    for k in ("position", "normal"):
        assert np.array_equal(bits(planes[k].cpu().numpy()), bits(e["planes"][k])), ("the renderer's plane differs from the oracle's", k)
    assert np.array_equal(np.array(mp.SecondaryVisibility.eye_of(cam), F), e["eye"])
    results = []
    for batch in (c["batch"], c["samples"]):
        vis = mp.SecondaryVisibility(scene, c["res"], batch=batch)
        out, counts = vis.ambient_occlusion(planes["position"], planes["normal"], cam, c["samples"], c["radius"], seed=c["ao_seed"], bias=c["bias"])
        assert vis.last_kernels() == [K_RESOLVE[True]] and ctx.last_kernels()  # the query ran on the scene's context
        torch.cuda.synchronize()
        results.append((out.cpu().numpy(), counts.cpu().numpy()))
        _same(results[-1][1], e["counts"], ("counts", batch))
        _same(results[-1][0], e["out"], ("out", batch))
    _same(results[0][1], results[1][1], "counts of 3 + 3 + 2 against 8")
    got = _count(tc.classes(results[0][1], e["info"]), ("partly", "free", "dark", "flipped"))
    assert got == _count(tc.classes(e["counts"], e["info"]), got) and all(n >= tc.E2E_MIN_PER_CLASS for n in got.values()), got


def test_sun_visibility_end_to_end(torch, oracle):
    """two teapot instances (the scene of tests/test_gpu_temporal.py): sun_visibility with a hard and a soft light on the planes the
    GPU rendered gives the bits of the model fed the same planes, downloaded; unlit and shadowed pixels are re-counted"""
    c = tc.E2E_SUN
    e = tc.e2e_sun(oracle, TEAPOT)
    ctx = mp.Context(0)
    base = mp.TriangleBvh.with_obj(TEAPOT, ctx)
    scene = mp.Scene(mp.Instances(base, np.array(c["instances"], F)))
    cam = tc.e2e_camera(mp, c)
    planes = _render_planes(scene, cam, c)
    torch.cuda.synchronize()
    position, normal = planes["position"].cpu().numpy(), planes["normal"].cpu().numpy()
    eye = np.array(mp.SecondaryVisibility.eye_of(cam), F)
    vis = mp.SecondaryVisibility(scene, c["res"], batch=c["batch"])
    for spread in c["spreads"]:
        want_out, want_counts, info = tc.sun_model(oracle, e["bvh"].occluded, position, normal, eye, spread)
        out, counts = vis.sun_visibility(planes["position"], planes["normal"], cam, tc.e2e_light(), c["samples"], spread=spread, seed=c["sun_seed"],
                                         bias=c["bias"])
        assert vis.last_kernels() == [K_RESOLVE[True]]
        torch.cuda.synchronize()
        got_counts = counts.cpu().numpy()
        _same(got_counts, want_counts, ("counts", spread))
        _same(out.cpu().numpy(), want_out, ("out", spread))
        got = _count(tc.classes(got_counts, info), ("unlit", "shadowed", "flipped", "free"))
        assert all(n >= tc.E2E_MIN_PER_CLASS for n in got.values()), got
        assert np.all(got_counts[..., 0][info["pixel"] == m.P_UNLIT] == 0)
    assert np.array_equal(bits(planes["position"].cpu().numpy()), bits(position))  # the planes are only read


def test_visibility_feeds_the_accumulator_and_the_denoiser(torch):
    """two frames of a moving camera: the visibility plane goes through TemporalAccumulator.accumulate and AtrousDenoiser.denoise as a
    colour: shapes are accepted, every value is finite and in [0, 1], and misses pass through all three stages bit for bit"""
    c = tc.E2E_AO
    w, h = c["res"]
    ctx = mp.Context(0)
    scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, ctx))
    vis = mp.SecondaryVisibility(scene, c["res"])
    acc = mp.TemporalAccumulator(c["res"], 0)
    dn = mp.AtrousDenoiser(c["res"], 0)
    (ex, ey, ez), at = c["camera"]
    for i in range(2):
        cam = mp.Camera.default().look_at((ex + 0.1 * i, ey, ez), at, (0.0, 1.0, 0.0)).f_number(float("inf"))
        planes = _render_planes(scene, cam, dict(c, seed=c["seed"] + i))
        ao, counts = vis.ambient_occlusion(planes["position"], planes["normal"], cam, c["samples"], c["radius"], seed=c["ao_seed"] + i)
        ao_host = ao.cpu().numpy()  # the next call overwrites vis's plane
        out, var = acc.accumulate(ao, planes["position"], planes["normal"], planes["ids"], mp.TemporalAccumulator.view_of(cam, c["res"]))
        clean, clean_var = dn.denoise(out, planes["normal"], variance=var)
        torch.cuda.synchronize()
        miss = planes["position"].cpu().numpy()[..., 3] == 0
        assert miss.sum() >= 32 and (~miss).sum() >= 32
        assert np.all(bits(ao_host[miss]) == bits(np.array([1, 1, 1, 0], F)))
        for name, t in (("accumulated", out), ("denoised", clean)):
            a = t.cpu().numpy()
            assert a.shape == (h, w, 4) and a.dtype == F, name
            assert np.all(np.isfinite(a)) and a.min() >= 0 and a.max() <= 1, (name, float(a.min()), float(a.max()))
            assert np.array_equal(bits(a[miss]), bits(ao_host[miss])), (name, "a miss was changed")
            assert np.all(a[..., 3][~miss] == 1), name
    assert float(acc.history_length().max()) == 2  # the second frame found history


def test_the_driver_checks_its_planes(torch):
    ctx = mp.Context(0)
    scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, ctx))
    vis = mp.SecondaryVisibility(scene, (8, 4), batch=2)
    good = torch.zeros((4, 8, 4), device="cuda")
    for bad in (good[:, :4], good.cpu(), good.double(), torch.zeros((8, 4, 4), device="cuda"), None):
        with pytest.raises(ValueError):
            vis.ambient_occlusion(bad, good, (0, 0, 5), 4, 1.0)
        with pytest.raises(ValueError):
            vis.sun_visibility(good, bad, (0, 0, 5), (0, 0, 1), 4)
    for samples in (0, 65537):
        with pytest.raises(ValueError):
            vis.ambient_occlusion(good, good, (0, 0, 5), samples, 1.0)
    with pytest.raises(mp.MinipathError):
        vis.ambient_occlusion(good, good, (0, 0, 5), 4, radius=0.0)
    with pytest.raises(mp.MinipathError):
        mp.SecondaryVisibility(scene, (8, 4), batch=0)
    out, counts = vis.ambient_occlusion(good, good, (0, 0, 5), 3, 1.0)  # all misses, batches of 2 + 1
    torch.cuda.synchronize()
    assert tuple(out.shape) == (4, 8, 4) and float(counts.abs().max()) == 0 and np.all(out.cpu().numpy() == np.array([1, 1, 1, 0], F))
