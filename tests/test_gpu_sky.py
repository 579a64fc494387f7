"""GPU tests of the sky lighting (include/minipath_sky.h, minipath_amd.SkyLight).  Every comparison is on f32 bit patterns against the
numpy model (tests/sky_model.py) with zero differences allowed.  Every buffer lies between sentinel guards, outputs are pre-filled
with the sentinel, and every call pins the kernel it reported.  The inputs are those of tests/sky_cases.py, which
tests/test_sky_cpu.py shows to reach every rule and every pixel class.  The stream test runs by the method, and with the helpers, of
tests/test_gpu_streams.py."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import secondary as sv
from minipath_amd import sky
from tests import secondary_cases, sky_cases as tc, sky_model as m
from tests.conftest import TEAPOT
from tests.sky_model import F, bits
from tests.test_gpu_streams import _control, _p, _stage, delay, side  # noqa: F401  (delay and side are fixtures)

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
PAD = 4096
K_RESOLVE = {False: "sky_resolve_kernel<false>", True: "sky_resolve_kernel<true>"}
K_GRADIENT = "sky_gradient_kernel"
READ = ("dx", "dy", "dz", "tmax")


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module", autouse=True)
def _own_hip_errors_only(torch):
    """As in tests/test_gpu_lights.py: what earlier test modules left in HIP's sticky per-thread error state is not this
    module's; a call of the library, which clears the state before its launch, takes it away."""
    import gc

    gc.collect()
    env = mp.gradient_sky(1, (1, 1, 1), (1, 1, 1), (0, 0, 0), 0)
    torch.cuda.synchronize()
    assert env.shape == (1, 1, 4)


def _same(got, want, what):
    """zero differing words"""
    diff = bits(np.asarray(got)) != bits(np.asarray(want))
    assert int(diff.sum()) == 0, (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def _guarded(torch, a, dtype=None, offset=0):
    """a copy of the host array (or a buffer of sentinels for a shape) in the middle of a larger tensor of sentinels: (whole, view).
    4-byte elements, or bytes with dtype = torch.uint8; the view starts `offset` elements after the front guard"""
    shape = a if isinstance(a, tuple) else a.shape
    n = int(np.prod(shape))
    if dtype is None:
        whole = torch.full((PAD + offset + n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    else:
        whole = torch.full((PAD + offset + n + PAD,), SENTINEL & 0xFF, dtype=dtype, device="cuda")
    view = whole[PAD + offset:PAD + offset + n]
    if not isinstance(a, tuple):
        host = np.ascontiguousarray(a)
        view.copy_(torch.from_numpy(host.reshape(-1) if dtype is not None else host.view(np.int32).reshape(-1)))
    return whole, view.view(shape)


def _guards_intact(torch, buffers, offset=0):
    for name, (whole, _) in buffers.items():
        raw = whole.cpu().numpy()
        s = SENTINEL if raw.dtype.itemsize == 4 else SENTINEL & 0xFF
        assert np.all(raw[:PAD + offset] == s) and np.all(raw[-PAD:] == s), name


def _host(t):
    return t.cpu().numpy().view(F)


def _settings(w, h, batch, n, pole, flags=0, sample_begin=0, sample_count=tc.SAMPLE_COUNT):
    return sky.SkySettings(C.sizeof(sky.SkySettings), w, h, flags, sample_count, sample_begin, batch, n, pole)


def _resolve(st, dev, env, sums, out):
    return sky.lib().mpe_resolve(0, C.byref(st), env.data_ptr(), *[dev[k][1].data_ptr() for k in READ], dev["occluded"][1].data_ptr(),
                                 sums.data_ptr(), None if out is None else out.data_ptr(), None)


# ---- mpe_fill_gradient ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", tc.MAPS)
def test_fill_gradient_matches_the_model(torch, n):
    """the map of the end-to-end case's three colours (nine different components), and one with negative components, in every word,
    .w included; nothing beside the map is written"""
    for zenith, horizon, ground in ((tc.E2E["zenith"], tc.E2E["horizon"], tc.E2E["ground"]), ((-1.0, 0.0, 3.5), (0.25, -0.75, 1e-3), (7.0, 1e30, -2.0))):
        env = _guarded(torch, (n, n, 4))
        f3 = lambda c: (C.c_float * 3)(*c)  # noqa: E731
        sky.check(sky.lib().mpe_fill_gradient(0, n, f3(zenith), f3(horizon), f3(ground), env[1].data_ptr(), None))
        assert sky.last_kernels() == [K_GRADIENT]
        torch.cuda.synchronize()
        _same(_host(env[1]), m.fill_gradient(n, zenith, horizon, ground), ("gradient", n))
        _guards_intact(torch, {"env": env})
    got = mp.gradient_sky(n, tc.E2E["zenith"], tc.E2E["horizon"], tc.E2E["ground"], 0)  # the wrapper, on the current stream
    torch.cuda.synchronize()
    _same(got.cpu().numpy(), m.fill_gradient(n, tc.E2E["zenith"], tc.E2E["horizon"], tc.E2E["ground"]), ("gradient_sky", n))


# ---- mpe_resolve on synthetic ray buffers -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", tc.MAPS, ids=lambda n: "N%d" % n)
@pytest.mark.parametrize("batch", tc.BATCHES, ids=lambda b: "B%d" % b)
@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: "%dx%d" % s)
def test_resolve_matches_the_model(torch, size, batch, n):
    """every planted direction and random ones under every tmax code and answer, in a map with a different value in every texel:
    for every pole, with and without MPE_FLAG_ACCUMULATE, with and without out, sums and out are the model's bits; a sums plane of
    sentinels is fully overwritten without the flag and continued with it; the inputs are only read"""
    w, h = size
    r = tc.resolve_inputs(w, h, batch, n)
    env_host = tc.texel_map(n)
    env = _guarded(torch, env_host)
    fixed = {"tmax": _guarded(torch, r["tmax"]), "occluded": _guarded(torch, r["occluded"], torch.uint8)}
    for pole in tc.POLES:
        d = m.from_map(r["m"], pole)
        dev = dict(fixed, **{k: _guarded(torch, np.ascontiguousarray(d[:, i])) for i, k in enumerate(("dx", "dy", "dz"))})
        for accumulate in (False, True):
            for with_out in (False, True):
                what = (pole, accumulate, with_out)
                outs = {"sums": _guarded(torch, r["sums"] if accumulate else (h, w, 4)), "out": _guarded(torch, (h, w, 4))}
                st = _settings(w, h, batch, n, pole, flags=sky.MPE_FLAG_ACCUMULATE if accumulate else 0)
                sky.check(_resolve(st, dev, env[1], outs["sums"][1], outs["out"][1] if with_out else None))
                assert sky.last_kernels() == [K_RESOLVE[with_out]], what
                torch.cuda.synchronize()
                want_sums, want_out = m.resolve(env_host, d[:, 0], d[:, 1], d[:, 2], r["tmax"], r["occluded"], (h, w), batch, pole,
                                                sums=r["sums"] if accumulate else None, want_out=with_out)
                assert np.all(np.isfinite(want_sums)), what
                _same(_host(outs["sums"][1]), want_sums, ("sums",) + what)
                if with_out:
                    _same(_host(outs["out"][1]), want_out, ("out",) + what)
                else:
                    assert np.all(outs["out"][1].cpu().numpy() == SENTINEL), what
                _guards_intact(torch, outs)
        _guards_intact(torch, dev)
        for i, k in enumerate(("dx", "dy", "dz")):
            assert np.array_equal(bits(_host(dev[k][1])), bits(d[:, i])), ("input changed", k)
    _guards_intact(torch, {"env": env})
    assert np.array_equal(bits(_host(env[1])), bits(env_host)) and np.array_equal(bits(_host(fixed["tmax"][1])), bits(r["tmax"]))
    assert np.array_equal(fixed["occluded"][1].cpu().numpy(), r["occluded"])


@pytest.mark.parametrize("n", tc.MAPS, ids=lambda n: "N%d" % n)
def test_resolve_in_batches_of_3_3_2_equals_8(torch, n):
    """the eight samples of the 64 x 16 case in one call, and in three calls on the slabs of the same buffers that continue the sums:
    the same bits, and the model's"""
    w, h = 64, 16
    r = tc.resolve_inputs(w, h, 8, n)
    pole, pixels = 1, w * h
    d = m.from_map(r["m"], pole)
    env_host = tc.texel_map(n)
    env = _guarded(torch, env_host)
    dev = {k: _guarded(torch, np.ascontiguousarray(d[:, i])) for i, k in enumerate(("dx", "dy", "dz"))}
    dev.update(tmax=_guarded(torch, r["tmax"]), occluded=_guarded(torch, r["occluded"], torch.uint8))
    whole = {k: _guarded(torch, (h, w, 4)) for k in ("sums", "out")}
    sky.check(_resolve(_settings(w, h, 8, n, pole), dev, env[1], whole["sums"][1], whole["out"][1]))
    split = {k: _guarded(torch, (h, w, 4)) for k in ("sums", "out")}
    for begin, b in ((0, 3), (3, 3), (6, 2)):
        part = {k: (None, v[1][begin * pixels:(begin + b) * pixels]) for k, v in dev.items()}
        st = _settings(w, h, b, n, pole, flags=sky.MPE_FLAG_ACCUMULATE if begin else 0, sample_begin=begin)
        sky.check(_resolve(st, part, env[1], split["sums"][1], split["out"][1] if begin == 6 else None))
        assert sky.last_kernels() == [K_RESOLVE[begin == 6]]
    torch.cuda.synchronize()
    want_sums, want_out = m.resolve(env_host, d[:, 0], d[:, 1], d[:, 2], r["tmax"], r["occluded"], (h, w), 8, pole)
    for k, want in (("sums", want_sums), ("out", want_out)):
        _same(_host(whole[k][1]), want, (k, "8"))
        _same(_host(split[k][1]), want, (k, "3 + 3 + 2"))
    _guards_intact(torch, {**dev, **whole, **{"split " + k: v for k, v in split.items()}, "env": env})


def test_a_refused_call_leaves_its_outputs_alone(torch):
    """real device buffers full of sentinels, a device that exists: calls refused for their settings, an overlap or an alignment
    launch nothing and write nothing"""
    w, h, B, n = 37, 23, 2, 5
    rays = w * h * B
    dev = {k: _guarded(torch, (rays,)) for k in READ}
    dev["occluded"] = _guarded(torch, (rays,), torch.uint8)
    outs = {k: _guarded(torch, (h, w, 4)) for k in ("sums", "out", "env")}
    sky.check(sky.lib().mpe_fill_gradient(0, n, *[(C.c_float * 3)(1, 2, 3)] * 3, outs["env"][1].data_ptr(), None))
    torch.cuda.synchronize()
    outs["env"][1].view(torch.int32).fill_(SENTINEL)
    record = sky.last_kernels()
    assert record == [K_GRADIENT]
    ptr = {k: v[1].data_ptr() for k, v in {**dev, **outs}.items()}
    res = lambda st, **kw: sky.lib().mpe_resolve(0, C.byref(st), *[{**ptr, **kw}[k] for k in ("env",) + READ + ("occluded", "sums", "out")], None)  # noqa: E731
    grad = lambda n_, colour, p: sky.lib().mpe_fill_gradient(0, n_, (C.c_float * 3)(*colour), (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0), p, None)  # noqa: E731
    good = _settings(w, h, B, n, 1)
    refused = [res(_settings(w, h, B, n, 3)), res(_settings(w, h, B, 0, 1)), res(_settings(w, h, B, 8193, 1)), res(_settings(w, h, B, n, 1, flags=2)),
               res(_settings(w, h, B, n, 1, sample_begin=7)), res(_settings(w, h, 0, n, 1)), res(good, out=ptr["sums"]), res(good, sums=ptr["env"]),
               res(good, out=ptr["tmax"] + 64), res(good, sums=ptr["sums"] + 4), res(good, env=ptr["env"] + 8), res(good, dx=ptr["dx"] + 2),
               res(good, occluded=None), grad(0, (1, 1, 1), ptr["env"]), grad(n, (1, float("inf"), 1), ptr["env"]), grad(n, (1, 1, 1), ptr["env"] + 4),
               grad(n, (1, 1, float("nan")), ptr["env"])]
    torch.cuda.synchronize()
    assert refused == [1] * len(refused) and sky.last_kernels() == record
    for name, (whole, _) in {**dev, **outs}.items():
        raw = whole.cpu().numpy()
        assert np.all(raw == (SENTINEL if raw.dtype.itemsize == 4 else SENTINEL & 0xFF)), name


def test_aligned_offset_views_are_accepted(torch):
    """planes and the map that start a whole number of pixels into an allocation and ray arrays that start at an odd word (`occluded`
    at an odd byte) are accepted and give the model's bits; the words before the views stay sentinels"""
    w, h, B, n, pole = 37, 23, 3, 5, 0
    r = tc.resolve_inputs(w, h, B, n)
    d = m.from_map(r["m"], pole)
    env_host = tc.texel_map(n)
    env = _guarded(torch, env_host, offset=12)  # three texels in
    dev = {k: _guarded(torch, np.ascontiguousarray(d[:, i]), offset=1 + 2 * i) for i, k in enumerate(("dx", "dy", "dz"))}
    dev.update(tmax=_guarded(torch, r["tmax"], offset=7), occluded=_guarded(torch, r["occluded"], torch.uint8, offset=3))
    outs = {"sums": _guarded(torch, (h, w, 4), offset=4), "out": _guarded(torch, (h, w, 4), offset=20)}
    assert all(v[1].data_ptr() % 16 == 0 for v in (env, outs["sums"], outs["out"])) and dev["dx"][1].data_ptr() % 16 == 4
    sky.check(_resolve(_settings(w, h, B, n, pole), dev, env[1], outs["sums"][1], outs["out"][1]))
    torch.cuda.synchronize()
    want_sums, want_out = m.resolve(env_host, d[:, 0], d[:, 1], d[:, 2], r["tmax"], r["occluded"], (h, w), B, pole)
    _same(_host(outs["sums"][1]), want_sums, "sums")
    _same(_host(outs["out"][1]), want_out, "out")
    for name, (whole, view) in {**dev, **outs, "env": env}.items():
        raw = whole.cpu().numpy()
        s = SENTINEL if raw.dtype.itemsize == 4 else SENTINEL & 0xFF
        assert np.all(raw[:-(view.numel() + PAD)] == s) and np.all(raw[-PAD:] == s), name
    # a plane 4 bytes off is refused, by the library and by the driver
    assert _resolve(_settings(w, h, B, n, pole), dev, env[1], outs["sums"][1].view(-1)[1:], None) == 1
    ctx = mp.Context(0)
    light = mp.SkyLight(mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, ctx)), (4, 2))
    plane = torch.zeros(4 * 2 * 4 + 4, device="cuda")
    good, odd = plane[4:].view(2, 4, 4), plane[1:-3].view(2, 4, 4)
    env_view = env[1].view(torch.float32)
    with pytest.raises(ValueError):
        light.light(odd, good, (0, 0, 5), env_view, 2)
    with pytest.raises(ValueError):
        light.light(good, good, (0, 0, 5), torch.zeros(5 * 5 * 4 + 4, device="cuda")[1:-3].view(5, 5, 4), 2)
    out, sums = light.light(good, good, (0, 0, 5), env_view, 2)  # the offset map through the driver: all misses
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0 and float(sums.abs().max()) == 0


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _render_planes(scene, cam, case):
    """the untiled feature planes of the case's frame, on the device"""
    fr = mp.FrameRenderer(scene, cam, mp.RenderSettings(case["tile"], case["spp"], case["res"], seed=case["seed"]))
    planes = fr.new_aov_planes(position=True)
    fr.render_aov_pass(planes)
    return {k: fr.untile_plane(t) for k, t in planes.items()}


def test_sky_light_end_to_end(torch, oracle):
    """the teapot at 24 x 16 under a three-colour gradient sky of 16 x 16 texels: the renderer's own planes through SkyLight.light with
    8 samples in batches of 3 + 3 + 2 and again in one batch of 8 give, in every word, the model's out and sums over the oracle's
    occlusion query, fed the same planes, and the same planes both times; with visibility=True the ambient-occlusion plane and its
    counts are, bit for bit, those of SecondaryVisibility for the same seed; every pixel class and both halves of the map are
    re-counted from the sums and the ray buffers the GPU left"""
    c = tc.E2E
    w, h = c["res"]
    ctx = mp.Context(0)
    scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, ctx))
    cam = secondary_cases.e2e_camera(mp, c)
    planes = _render_planes(scene, cam, c)
    env = mp.gradient_sky(c["map_size"], c["zenith"], c["horizon"], c["ground"], 0)
    torch.cuda.synchronize()
    position, normal = planes["position"].cpu().numpy(), planes["normal"].cpu().numpy()
    eye = np.array(mp.SkyLight.eye_of(cam), F)
    e = tc.e2e(oracle, TEAPOT)
    assert np.array_equal(eye, e["eye"])
    _same(env.cpu().numpy(), e["env"], "the map")
    assert np.unique(e["env"][..., :3]).size > 9 and len(set(c["zenith"] + c["horizon"] + c["ground"])) == 9
    want_out, want_sums, want_ao, want_counts, want_rays = m.run(oracle, e["bvh"].occluded, position, normal, e["env"], c["sky_seed"], c["samples"],
                                                                 c["batch"], eye, pole=c["pole"], radius=c["radius"], bias=c["bias"],
                                                                 visibility=True, want_rays=True)
    kw = dict(seed=c["sky_seed"], pole=c["pole"], radius=c["radius"], bias=c["bias"])
    results = []
    for batch in (c["batch"], c["samples"]):
        light = mp.SkyLight(scene, c["res"], batch=batch)
        out, sums = light.light(planes["position"], planes["normal"], cam, env, c["samples"], **kw)
        assert light.last_kernels() == [K_RESOLVE[True]] and ctx.last_kernels()  # the query ran on the scene's context
        torch.cuda.synchronize()
        results.append((out.cpu().numpy(), sums.cpu().numpy()))
        _same(results[-1][1], want_sums, ("sums", batch))
        _same(results[-1][0], want_out, ("out", batch))
        out, sums, ao, counts = light.light(planes["position"], planes["normal"], cam, env, c["samples"], visibility=True, **kw)
        assert sv.last_kernels() == ["resolve_kernel<true>"]
        torch.cuda.synchronize()
        _same(out.cpu().numpy(), want_out, ("out with visibility", batch))
        _same(sums.cpu().numpy(), want_sums, ("sums with visibility", batch))
        _same(ao.cpu().numpy(), want_ao, ("ao", batch))
        _same(counts.cpu().numpy(), want_counts, ("counts", batch))
    _same(results[0][0], results[1][0], "out of 3 + 3 + 2 against 8")
    # one trace for both: SecondaryVisibility alone gives the same ambient occlusion for the same seed
    vis = mp.SecondaryVisibility(scene, c["res"], batch=c["batch"])
    ao_alone, counts_alone = vis.ambient_occlusion(planes["position"], planes["normal"], cam, c["samples"], c["radius"], seed=c["sky_seed"], bias=c["bias"])
    torch.cuda.synchronize()
    _same(ao_alone.cpu().numpy(), ao.cpu().numpy(), "ao against SecondaryVisibility")
    _same(counts_alone.cpu().numpy(), counts.cpu().numpy(), "counts against SecondaryVisibility")
    # the last object ran one batch of all 8 samples: its ray buffers hold every ray of the frame
    b = light._buffers
    got_rays = {"d": np.stack([b[k].cpu().numpy().reshape(c["samples"], h, w) for k in ("dx", "dy", "dz")], -1),
                "tmax": b["tmax"].cpu().numpy().reshape(c["samples"], h, w), "occluded": b["occluded"].cpu().numpy().reshape(c["samples"], h, w)}
    _same(got_rays["d"], want_rays["d"], "directions")
    _same(got_rays["tmax"], want_rays["tmax"], "tmax")
    assert np.array_equal(got_rays["occluded"] != 0, want_rays["occluded"] != 0)
    got = {k: int(v.sum()) for k, v in tc.classes(results[1][1], got_rays).items()}
    assert got == {k: int(v.sum()) for k, v in tc.classes(want_sums, want_rays).items()}
    assert all(got[k] >= tc.E2E_MIN_PER_CLASS for k in tc.E2E_CLASSES), got
    halves = tc.open_rays_per_half(got_rays, c["pole"])
    assert halves == tc.open_rays_per_half(want_rays, c["pole"]) and min(halves) >= tc.E2E_MIN_RAYS_PER_HALF, halves
    assert np.array_equal(bits(planes["position"].cpu().numpy()), bits(position))  # the planes are only read
    _same(env.cpu().numpy(), e["env"], "the map is only read")


def test_sky_light_feeds_the_accumulator_and_the_denoiser(torch):
    """two frames of a moving camera: the sky plane goes through TemporalAccumulator.accumulate and AtrousDenoiser.denoise as a
    colour: shapes are accepted, every value is finite where alpha is 1, and misses (alpha 0) stay 0 through all three stages"""
    c = tc.E2E
    w, h = c["res"]
    ctx = mp.Context(0)
    scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, ctx))
    light = mp.SkyLight(scene, c["res"])
    env = mp.gradient_sky(c["map_size"], c["zenith"], c["horizon"], c["ground"], 0)
    acc = mp.TemporalAccumulator(c["res"], 0)
    dn = mp.AtrousDenoiser(c["res"], 0)
    (ex, ey, ez), at = c["camera"]
    for i in range(2):
        cam = mp.Camera.default().look_at((ex + 0.1 * i, ey, ez), at, (0.0, 1.0, 0.0)).f_number(float("inf"))
        planes = _render_planes(scene, cam, dict(c, seed=c["seed"] + i))
        out_sky, sums = light.light(planes["position"], planes["normal"], cam, env, c["samples"], seed=c["sky_seed"] + i, pole=c["pole"])
        sky_host = out_sky.cpu().numpy()  # the next call overwrites the object's plane
        out, var = acc.accumulate(out_sky, planes["position"], planes["normal"], planes["ids"], mp.TemporalAccumulator.view_of(cam, c["res"]))
        clean, clean_var = dn.denoise(out, planes["normal"], variance=var)
        torch.cuda.synchronize()
        miss = planes["position"].cpu().numpy()[..., 3] == 0
        assert miss.sum() >= 32 and (~miss).sum() >= 32
        assert not sky_host[miss].any() and np.all(sky_host[..., 3][~miss] == 1) and sky_host[..., :3].max() > 0
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
    light = mp.SkyLight(scene, (8, 4), batch=2)
    good = torch.zeros((4, 8, 4), device="cuda")
    env = mp.gradient_sky(2, (1, 1, 1), (1, 1, 1), (0, 0, 0), 0)
    for bad in (good[:, :4], good.cpu(), good.double(), torch.zeros((8, 4, 4), device="cuda"), None):
        with pytest.raises(ValueError):
            light.light(bad, good, (0, 0, 5), env, 4)
        with pytest.raises(ValueError):
            light.light(good, bad, (0, 0, 5), env, 4)
    for bad_env in (env[:, :1], env.cpu(), env.double(), torch.zeros((2, 3, 4), device="cuda"), torch.zeros((2, 2, 3), device="cuda"), None):
        with pytest.raises(ValueError):
            light.light(good, good, (0, 0, 5), bad_env, 4)
    for samples in (0, 65537):
        with pytest.raises(ValueError):
            light.light(good, good, (0, 0, 5), env, samples)
    with pytest.raises(mp.MinipathError):
        light.light(good, good, (0, 0, 5), env, 4, pole=3)
    with pytest.raises(mp.MinipathError):
        light.light(good, good, (0, 0, 5), env, 4, radius=0.0)  # mps_generate's refusal
    with pytest.raises(mp.MinipathError):
        mp.SkyLight(scene, (8, 4), batch=0)
    for bad_n in (0, 8193):
        with pytest.raises(ValueError):
            mp.gradient_sky(bad_n, (1, 1, 1), (1, 1, 1), (0, 0, 0), 0)
    with pytest.raises(mp.MinipathError):
        mp.gradient_sky(2, (1, float("nan"), 1), (1, 1, 1), (0, 0, 0), 0)
    out, sums = light.light(good, good, (0, 0, 5), env, 3)  # all misses, batches of 2 + 1
    torch.cuda.synchronize()
    assert tuple(out.shape) == (4, 8, 4) and float(sums.abs().max()) == 0 and float(out.abs().max()) == 0


# ---- the calling context: a side stream ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def teapot(torch):
    return mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, mp.Context(0)))


def test_sky_light_behind_a_stalled_side_stream(torch, delay, side, oracle, teapot):  # noqa: F811
    """SkyLight.light enqueued on a side stream behind a delay and behind the copies that put the true planes and the true map into
    buffers that hold another case's: the results are the model's on the true inputs, so every launch of the chain (mps_generate,
    mp_occluded_rays, mpe_resolve) went to the current stream and nothing waited for it"""
    case = tc.stream_stage(oracle, TEAPOT)
    c = tc.E2E

    def make():
        light = mp.SkyLight(teapot, case.res, batch=tc.STREAM_BATCH)

        def body(b):
            out, sums = light.light(b["position"], b["normal"], [float(v) for v in case.eye], b["env"], c["samples"], seed=c["sky_seed"],
                                    pole=c["pole"], radius=c["radius"], bias=c["bias"])
            assert light.last_kernels() == [K_RESOLVE[True]]
            return {"out": out, "sums": sums}
        return body
    _stage(torch, delay, side, "sky", case, make)


def test_control_sky(torch, delay, side):  # noqa: F811
    """the positive control: mpe_resolve on the NULL stream while the side stream is stalled reads the other case's buffers and gives
    the other case's result"""
    case, c = tc.stream_control(), tc.CONTROL

    def call(b, o):
        st = _settings(c["w"], c["h"], c["batch"], c["n"], c["pole"])
        sky.check(sky.lib().mpe_resolve(0, C.byref(st), _p(b["env"]), _p(b["dx"]), _p(b["dy"]), _p(b["dz"]), _p(b["tmax"]), _p(b["occluded"]),
                                        _p(o["sums"]), _p(o["out"]), None))
    _control(torch, delay, side, "sky", case, call, {k: ((c["h"], c["w"], 4), torch.float32) for k in ("sums", "out")})
