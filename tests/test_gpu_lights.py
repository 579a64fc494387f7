"""GPU tests of the lights (include/minipath_lights.h, minipath_amd.LocalLights).  Every comparison is on f32 bit patterns against the
numpy model (tests/lights_model.py) with zero differences allowed; no result here is a NaN.  Every buffer lies between sentinel
guards, outputs are pre-filled with the sentinel, and every call pins the kernel it reported.  The inputs are those of
tests/lights_cases.py, which tests/test_lights_cpu.py shows to reach every rule and every pixel class."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import lights as ll
from tests import lights_cases as tc, lights_model as m, secondary_cases
from tests.conftest import TEAPOT
from tests.lights_model import F, bits

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
PAD = 4096
K_GEN = {False: "light_rays_kernel<false>", True: "light_rays_kernel<true>"}
K_RESOLVE = {False: "irradiance_kernel<false>", True: "irradiance_kernel<true>"}


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module", autouse=True)
def _own_hip_errors_only(torch):
    """As in tests/test_gpu_secondary.py: what earlier test modules left in HIP's sticky per-thread error state is not this
    module's; a call of the library, which clears the state before its launch, takes it away."""
    import gc

    gc.collect()
    buf = torch.zeros((3, 1, 1, 4), dtype=torch.float32, device="cuda")
    st = _settings(1, 1, 1, 1, 0)
    ll.check(ll.lib().mpl_resolve(0, C.byref(st), ll.light_table(tc.TABLES["point"]), buf[0].data_ptr(), buf[1].data_ptr(), buf[1].data_ptr(),
                                  buf[2].data_ptr(), None, None))
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


def _settings(w, h, light_count, batch, sample_begin, flags=0, sample_count=tc.SAMPLE_COUNT, seed=tc.SEED, eye=tc.EYE, bias=tc.BIAS,
              margin=tc.MARGIN):
    st = ll.LightsSettings(C.sizeof(ll.LightsSettings), w, h, flags, sample_count, sample_begin, batch, light_count, seed)
    st.eye[:] = eye
    st.bias, st.margin = bias, margin
    return st


# ---- mpl_generate ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", tc.BATCHES, ids=lambda b: "B%d_from%d" % b)
@pytest.mark.parametrize("table_name", list(tc.TABLES))
@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: "%dx%d" % s)
def test_generate_matches_the_model(torch, oracle, size, table_name, batch):
    """all eight arrays equal the model in every word, the zeros and codes of none and unlit rays included; nothing but the eight
    arrays is written (mpl_generate is not given `occluded`, which stays all sentinel), and the planes are only read.  The table of
    point lights alone runs the kernel without the RNG, the others the one with it"""
    (w, h), (B, begin) = size, batch
    case, lights = tc.synthetic(w, h), tc.TABLES[table_name]
    L = len(lights)
    want, info = tc.generated(oracle, w, h, table_name, B, begin)
    planes = {k: _guarded(torch, case[k]) for k in ("position", "normal")}
    rays = {k: _guarded(torch, (B * L * h * w,)) for k in m.RAY_ARRAYS}
    occluded = _guarded(torch, (B * L * h * w,), torch.uint8)  # the query's output, allocated beside the rays as the driver does
    st = _settings(w, h, L, B, begin)
    ll.check(ll.lib().mpl_generate(0, C.byref(st), ll.light_table(lights), planes["position"][1].data_ptr(), planes["normal"][1].data_ptr(),
                                   *[rays[k][1].data_ptr() for k in m.RAY_ARRAYS], None))
    assert ll.last_kernels() == [K_GEN[table_name != "point"]]
    torch.cuda.synchronize()
    for k in m.RAY_ARRAYS:
        _same(_host(rays[k][1]), want[k], k)
    _guards_intact(torch, {**planes, **rays, "occluded": occluded})
    assert np.all(occluded[1].cpu().numpy() == SENTINEL & 0xFF)
    for k in planes:
        assert np.array_equal(bits(_host(planes[k][1])), bits(case[k])), ("input changed", k)
    # what the codes say, from what the GPU wrote
    tmax = _host(rays["tmax"][1]).reshape(B, L, h, w)
    assert np.array_equal(tmax[0, 0] == 0, info["pixel"] != m.P_LIVE) and np.array_equal(tmax > 0, info["lit"])
    assert np.array_equal(tmax == -1, ~info["lit"] & (info["pixel"] == m.P_LIVE))


# ---- mpl_resolve -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_out", [False, True], ids=["noout", "out"])
@pytest.mark.parametrize("accumulate", [False, True], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("shape", tc.RESOLVE_SHAPES, ids=lambda s: "B%d_%s" % s)
@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: "%dx%d" % s)
def test_resolve_matches_the_model(torch, size, shape, accumulate, with_out):
    """random answers and weights under every tmax code (0, -1, -0, 0.5, +inf, NaN, -2): sums and out are the model's bits; a sums
    plane of sentinels is fully overwritten without the flag and continued with it"""
    (w, h), (B, table_name) = size, shape
    lights = tc.TABLES[table_name]
    r = tc.resolve_inputs(w, h, B, table_name)
    dev = {"tmax": _guarded(torch, r["tmax"]), "weight": _guarded(torch, r["weight"]), "occluded": _guarded(torch, r["occluded"], torch.uint8)}
    outs = {"sums": _guarded(torch, r["sums"] if accumulate else (h, w, 4)), "out": _guarded(torch, (h, w, 4))}
    st = _settings(w, h, len(lights), B, 0, flags=ll.MPL_FLAG_ACCUMULATE if accumulate else 0)
    ll.check(ll.lib().mpl_resolve(0, C.byref(st), ll.light_table(lights), dev["tmax"][1].data_ptr(), dev["weight"][1].data_ptr(),
                                  dev["occluded"][1].data_ptr(), outs["sums"][1].data_ptr(), outs["out"][1].data_ptr() if with_out else None, None))
    assert ll.last_kernels() == [K_RESOLVE[with_out]]
    torch.cuda.synchronize()
    want_sums, want_out = m.resolve(r["tmax"], r["weight"], r["occluded"], lights, (h, w), B, sums=r["sums"] if accumulate else None, want_out=with_out)
    assert np.all(np.isfinite(want_sums))
    _same(_host(outs["sums"][1]), want_sums, "sums")
    if with_out:
        _same(_host(outs["out"][1]), want_out, "out")
    else:
        assert np.all(outs["out"][1].cpu().numpy() == SENTINEL)
    _guards_intact(torch, {**dev, **outs})
    for k in ("tmax", "weight"):
        assert np.array_equal(bits(_host(dev[k][1])), bits(r[k])), ("input changed", k)
    assert np.array_equal(dev["occluded"][1].cpu().numpy(), r["occluded"])


def test_a_refused_call_leaves_its_outputs_alone(torch):
    """real device buffers full of sentinels, a device that exists: calls refused for their settings, their lights or an overlap
    launch nothing and write nothing"""
    w, h, B = 37, 23, 2
    lights = tc.TABLES["mixed"]
    L, n = len(lights), 37 * 23 * 2 * 3
    planes = {k: _guarded(torch, tc.synthetic(w, h)[k]) for k in ("position", "normal")}
    rays = {k: _guarded(torch, (n,)) for k in m.RAY_ARRAYS}
    occluded = _guarded(torch, (n,), torch.uint8)
    outs = {k: _guarded(torch, (h, w, 4)) for k in ("sums", "out")}
    good, table = _settings(w, h, L, B, 0), ll.light_table(lights)
    ll.check(ll.lib().mpl_resolve(0, C.byref(_settings(1, 1, 1, 1, 0)), ll.light_table(tc.TABLES["point"]), rays["tmax"][1].data_ptr(),
                                  rays["weight"][1].data_ptr(), occluded[1].data_ptr(), outs["sums"][1].data_ptr(), None, None))
    torch.cuda.synchronize()
    outs["sums"][1].view(torch.int32).fill_(SENTINEL)
    record = ll.last_kernels()
    assert record == [K_RESOLVE[False]]
    bad_table = ll.light_table(lights)
    bad_table[1].radius = -1.0
    ptr = {k: v[1].data_ptr() for k, v in {**planes, **rays, **outs, "occluded": occluded}.items()}
    gen = lambda st, tb, **kw: ll.lib().mpl_generate(0, C.byref(st), tb, *[{**ptr, **kw}[k] for k in ("position", "normal") + m.RAY_ARRAYS], None)  # noqa: E731
    res = lambda st, tb, **kw: ll.lib().mpl_resolve(0, C.byref(st), tb, *[{**ptr, **kw}[k] for k in ("tmax", "weight", "occluded", "sums", "out")], None)  # noqa: E731
    refused = [gen(_settings(w, h, L, B, 7), table), gen(good, bad_table), gen(good, table, weight=ptr["tmax"]), gen(good, table, dz=ptr["normal"] + 16),
               gen(_settings(w, h, L, B, 0, margin=float("nan")), table), gen(_settings(w, h, 9, B, 0), table),
               res(_settings(w, h, L, B, 0, flags=2), table), res(good, bad_table), res(good, table, out=ptr["sums"]), res(good, table, sums=ptr["weight"] + 4)]
    torch.cuda.synchronize()
    assert refused == [1] * len(refused) and ll.last_kernels() == record
    for name, (whole, _) in {**rays, **outs, "occluded": occluded}.items():
        raw = whole.cpu().numpy()
        assert np.all(raw == (SENTINEL if raw.dtype.itemsize == 4 else SENTINEL & 0xFF)), name


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _render_planes(scene, cam, case):
    """the untiled feature planes of the case's frame, on the device"""
    fr = mp.FrameRenderer(scene, cam, mp.RenderSettings(case["tile"], case["spp"], case["res"], seed=case["seed"]))
    planes = fr.new_aov_planes(position=True)
    fr.render_aov_pass(planes)
    return {k: fr.untile_plane(t) for k, t in planes.items()}


def test_irradiance_end_to_end(torch, oracle):
    """the teapot at 24 x 16 under a point and a sphere light: the renderer's own planes through LocalLights.irradiance with 8 samples
    in batches of 3 + 3 + 2 and again in one batch of 8 give, in every word, the model's out and sums over the oracle's occlusion
    query with a tmax per ray, fed the same planes, and the same planes both times; every pixel class is re-counted from the sums and
    the ray buffers the GPU left"""
    c = tc.E2E
    w, h = c["res"]
    ctx = mp.Context(0)
    scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, ctx))
    cam = secondary_cases.e2e_camera(mp, c)
    planes = _render_planes(scene, cam, c)
    torch.cuda.synchronize()
    position, normal = planes["position"].cpu().numpy(), planes["normal"].cpu().numpy()
    eye = np.array(mp.LocalLights.eye_of(cam), F)
    e = tc.e2e(oracle, TEAPOT)
    assert np.array_equal(eye, e["eye"])
    want_out, want_sums, want_rays = m.run(oracle, e["bvh"].occluded, position, normal, c["lights"], c["light_seed"], c["samples"], c["batch"], eye,
                                           want_rays=True, bias=c["bias"], margin=c["margin"])
    results = []
    for batch in (c["batch"], c["samples"]):
        lights = mp.LocalLights(scene, c["res"], batch=batch)
        out, sums = lights.irradiance(planes["position"], planes["normal"], cam, c["lights"], c["samples"], seed=c["light_seed"], bias=c["bias"],
                                      margin=c["margin"])
        assert lights.last_kernels() == [K_RESOLVE[True]] and ctx.last_kernels()  # the query ran on the scene's context
        torch.cuda.synchronize()
        results.append((out.cpu().numpy(), sums.cpu().numpy()))
        _same(results[-1][1], want_sums, ("sums", batch))
        _same(results[-1][0], want_out, ("out", batch))
    _same(results[0][0], results[1][0], "out of 3 + 3 + 2 against 8")
    # the last object ran one batch of all 8 samples: its ray buffers hold every ray of the frame
    b = lights._buffers
    got_rays = {"tmax": b["tmax"].cpu().numpy().reshape(c["samples"], 2, h, w), "occluded": b["occluded"].cpu().numpy().reshape(c["samples"], 2, h, w)}
    _same(got_rays["tmax"], want_rays["tmax"], "tmax")
    assert np.array_equal(got_rays["occluded"] != 0, want_rays["occluded"] != 0)
    got = {k: int(v.sum()) for k, v in tc.classes(results[1][1], got_rays).items()}
    assert got == {k: int(v.sum()) for k, v in tc.classes(want_sums, want_rays).items()}
    assert all(got[k] >= tc.E2E_MIN_PER_CLASS for k in tc.E2E_CLASSES), got
    assert np.array_equal(bits(planes["position"].cpu().numpy()), bits(position))  # the planes are only read


def test_irradiance_feeds_the_accumulator_and_the_denoiser(torch):
    """two frames of a moving camera: the irradiance plane goes through TemporalAccumulator.accumulate and AtrousDenoiser.denoise as a
    colour: shapes are accepted, every value is finite where alpha is 1, and misses (alpha 0) stay 0 through all three stages"""
    c = tc.E2E
    w, h = c["res"]
    ctx = mp.Context(0)
    scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, ctx))
    lights = mp.LocalLights(scene, c["res"])
    acc = mp.TemporalAccumulator(c["res"], 0)
    dn = mp.AtrousDenoiser(c["res"], 0)
    (ex, ey, ez), at = c["camera"]
    for i in range(2):
        cam = mp.Camera.default().look_at((ex + 0.1 * i, ey, ez), at, (0.0, 1.0, 0.0)).f_number(float("inf"))
        planes = _render_planes(scene, cam, dict(c, seed=c["seed"] + i))
        light, sums = lights.irradiance(planes["position"], planes["normal"], cam, c["lights"], c["samples"], seed=c["light_seed"] + i, margin=c["margin"])
        light_host = light.cpu().numpy()  # the next call overwrites the object's plane
        out, var = acc.accumulate(light, planes["position"], planes["normal"], planes["ids"], mp.TemporalAccumulator.view_of(cam, c["res"]))
        clean, clean_var = dn.denoise(out, planes["normal"], variance=var)
        torch.cuda.synchronize()
        miss = planes["position"].cpu().numpy()[..., 3] == 0
        assert miss.sum() >= 32 and (~miss).sum() >= 32
        assert not light_host[miss].any() and np.all(light_host[..., 3][~miss] == 1) and light_host[..., :3].max() > 0
        for name, t in (("accumulated", out), ("denoised", clean)):
            a = t.cpu().numpy()
            assert a.shape == (h, w, 4) and a.dtype == F, name
            assert np.all(np.isfinite(a[~miss])) and a[~miss].min() >= 0, name
            assert not a[miss].any(), (name, "a miss was changed")
            assert np.all(a[..., 3][~miss] == 1), name
    assert float(acc.history_length().max()) == 2  # the second frame found history


def test_the_driver_checks_its_arguments(torch):
    ctx = mp.Context(0)
    scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, ctx))
    lights = mp.LocalLights(scene, (8, 4), batch=2)
    good = torch.zeros((4, 8, 4), device="cuda")
    lamp = [((0.0, 5.0, 0.0), 0.5, (1.0, 1.0, 1.0))]
    for bad in (good[:, :4], good.cpu(), good.double(), torch.zeros((8, 4, 4), device="cuda"), None):
        with pytest.raises(ValueError):
            lights.irradiance(bad, good, (0, 0, 5), lamp, 4)
        with pytest.raises(ValueError):
            lights.irradiance(good, bad, (0, 0, 5), lamp, 4)
    for samples in (0, 65537):
        with pytest.raises(ValueError):
            lights.irradiance(good, good, (0, 0, 5), lamp, samples)
    for table in ([], lamp * 9):
        with pytest.raises(ValueError):
            lights.irradiance(good, good, (0, 0, 5), table, 4)
    with pytest.raises(mp.MinipathError):
        lights.irradiance(good, good, (0, 0, 5), [((0.0, 5.0, 0.0), -0.5, (1.0, 1.0, 1.0))], 4)
    with pytest.raises(mp.MinipathError):
        lights.irradiance(good, good, (0, 0, 5), lamp, 4, margin=-1.0)
    with pytest.raises(mp.MinipathError):
        mp.LocalLights(scene, (8, 4), batch=0)
    out, sums = lights.irradiance(good, good, (0, 0, 5), lamp, 3)  # all misses, batches of 2 + 1
    out2, _ = lights.irradiance(good, good, (0, 0, 5), lamp * 3, 3)  # more lights: the ray buffers grow, the planes stay
    torch.cuda.synchronize()
    assert out2.data_ptr() == out.data_ptr() and tuple(out.shape) == (4, 8, 4) and float(sums.abs().max()) == 0 and float(out.abs().max()) == 0
