"""GPU tests of the temporal reprojection (include/minipath_temporal.h, minipath_amd.TemporalAccumulator).  Every comparison is on
f32 and u32 bit patterns against the numpy model (tests/temporal_model.py) with zero differences allowed -- only where the model's
result is NaN, whose bits the header leaves open, a NaN of any bits is asked for; a colour that merely passes through is compared bit
for bit, NaN or not.  Every buffer lies between sentinel guards, outputs are pre-filled with the sentinel, and every case pins the
kernel the call reported.  The inputs are those of tests/temporal_cases.py, which tests/test_temporal_cpu.py shows to reach every rule."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import temporal as tp
from tests import denoise_model, temporal_cases as tc, temporal_model as m
from tests.conftest import TEAPOT
from tests.temporal_model import F, bits

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
PAD = 4096
K_VAR, K_PLAIN, K_RESET = "reproject_kernel<true>", "reproject_kernel<false>", "reset_kernel"
INF = float("inf")
# max_history 1 and +inf, alpha 0 and 1
COMBOS = [(1.0, 0.0), (INF, 1.0), (INF, 0.0), (1.0, 1.0)]
# (width, height, previous view in general position)
SHAPES = [(w, h, False) for w, h in tc.SIZES] + [(37, 23, True), (64, 16, True)]


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
    buf = torch.empty((4, 1, 1, 4), dtype=torch.float32, device="cuda")
    tp.check(tp.lib().mpt_reset(0, 1, 1, buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), buf[3].data_ptr(), None))
    torch.cuda.synchronize()


def _same(got, want, what):
    """zero differing words, a NaN of the model standing for any NaN"""
    got, want = np.asarray(got), np.asarray(want)
    diff = bits(got) != bits(want)
    if want.dtype == F:
        diff &= ~(np.isnan(want) & np.isnan(got))
    assert int(diff.sum()) == 0, (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def _guarded(torch, a):
    """a copy of the host array (or a plane of sentinels for a shape) in the middle of a larger tensor of sentinels: (whole, view)"""
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


def _host(t):
    return t.cpu().numpy().view(F)


def _settings(w, h, st):
    return tp.TemporalSettings(C.sizeof(tp.TemporalSettings), w, h, tp.MPT_FLAG_MATCH_PRIM if st["match_prim"] else 0, st["sigma_position"],
                               st["normal_min"], st["max_history"], st["alpha_color"], st["alpha_moments"], st["min_variance_history"])


def _view(v):
    return tp.TemporalView.from_buffer_copy(v.floats().tobytes())


def _reproject(torch, dev, w, h, view, st, with_variance, want_variance=True):
    """mpt_reproject on guarded device buffers `dev` (name -> (whole, view)) into fresh guarded outputs: (out, moments, variance) on the host"""
    outs = {k: _guarded(torch, (h, w, 4)) for k in ("out", "moments_out", "variance_out")}
    p = lambda k: dev[k][1].data_ptr()  # noqa: E731
    settings, vw = _settings(w, h, st), _view(view)
    tp.check(tp.lib().mpt_reproject(0, C.byref(settings), C.byref(vw), p("color"), p("position"), p("normal"), p("ids"),
                                    p("variance") if with_variance else None, p("prev_position"), p("prev_normal"), p("prev_ids"),
                                    p("hist_color"), p("hist_moments"), outs["out"][1].data_ptr(), outs["moments_out"][1].data_ptr(),
                                    outs["variance_out"][1].data_ptr() if want_variance else None, None))
    assert tp.last_kernels() == [K_VAR if with_variance else K_PLAIN]
    torch.cuda.synchronize()
    _guards_intact(torch, outs)
    if not want_variance:
        assert np.all(outs["variance_out"][1].cpu().numpy() == SENTINEL)
    return tuple(_host(outs[k][1]) for k in ("out", "moments_out", "variance_out"))


def _upload(torch, case):
    cur, prev = case["cur"], case["prev"]
    host = {"color": cur["color"], "position": cur["position"], "normal": cur["normal"], "ids": cur["ids"], "variance": cur["variance"],
            "prev_position": prev["position"], "prev_normal": prev["normal"], "prev_ids": prev["ids"], "hist_color": prev["color"],
            "hist_moments": prev["moments"]}
    return host, {k: _guarded(torch, a) for k, a in host.items()}


def _check_against_model(got, want, info, color):
    _same(got[0], want[0], "out")
    _same(got[1], want[1], "moments_out")
    _same(got[2], want[2], "variance_out")
    through = info["pixel"] != m.P_HISTORY  # out = color bit for bit, whatever the colour is
    assert np.array_equal(bits(got[0])[through], bits(color)[through])


@pytest.mark.parametrize("match_prim", [False, True], ids=["anyprim", "matchprim"])
@pytest.mark.parametrize("with_variance", [False, True], ids=["novar", "var"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d%s" % (s[0], s[1], "_general" if s[2] else ""))
def test_synthetic_planes_match_the_model(torch, shape, with_variance, match_prim):
    w, h, general = shape
    case = tc.synthetic(w, h, general)
    host, dev = _upload(torch, case)
    for max_history, alpha in COMBOS:
        st = tc.synthetic_settings(max_history, alpha, match_prim)
        *want, info = tc.model_on(case, st, with_variance, want_info=True)
        got = _reproject(torch, dev, w, h, case["view"], st, with_variance)
        _check_against_model(got, want, info, host["color"])
    # without variance_out nothing of it is written, and the rest is the same
    got = _reproject(torch, dev, w, h, case["view"], st, False, want_variance=False)
    want = tc.model_on(case, st, False)
    _same(got[0], want[0], "out, no variance_out")
    _same(got[1], want[1], "moments_out, no variance_out")
    _guards_intact(torch, dev)
    for k, a in host.items():  # the inputs are only read
        assert np.array_equal(bits(_host(dev[k][1])), bits(a)), ("input changed", k)


@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: "%dx%d" % s)
def test_reset_matches_the_model(torch, size):
    w, h = size
    cur = tc.synthetic(w, h)["cur"]
    dev = {k: _guarded(torch, cur[k]) for k in ("color", "position")}
    outs = {k: _guarded(torch, (h, w, 4)) for k in ("out", "moments_out")}
    tp.check(tp.lib().mpt_reset(0, w, h, dev["color"][1].data_ptr(), dev["position"][1].data_ptr(), outs["out"][1].data_ptr(),
                                outs["moments_out"][1].data_ptr(), None))
    assert tp.last_kernels() == [K_RESET]
    torch.cuda.synchronize()
    want = m.reset(cur["color"], cur["position"])
    assert np.array_equal(bits(_host(outs["out"][1])), bits(want[0]))  # the colour, bit for bit
    _same(_host(outs["moments_out"][1]), want[1], "moments_out")
    _guards_intact(torch, {**dev, **outs})
    for k in dev:
        assert np.array_equal(bits(_host(dev[k][1])), bits(cur[k])), ("input changed", k)


def _render_planes(scene, cam, res, spp, seed, tile=32):
    """the untiled feature planes of one frame, on the device"""
    fr = mp.FrameRenderer(scene, cam, mp.RenderSettings(tile, spp, res, seed=seed))
    planes = fr.new_aov_planes(position=True, shade_sq=True)
    fr.render_aov_pass(planes)
    return {k: fr.untile_plane(t) for k, t in planes.items()}


def test_two_cameras_end_to_end(torch, oracle):
    """two teapot instances from the two cameras of tests/temporal_cases.py, 96 x 64 x 8 spp: the renderer's own untiled planes --
    bit-equal to the oracle's -- through mpt_reset and mpt_reproject give the model's bits, and the frame holds every pixel class"""
    e = tc.e2e_model(oracle, TEAPOT)
    ctx = mp.Context(0)
    base = mp.TriangleBvh.with_obj(TEAPOT, ctx)
    scene = mp.Scene(mp.Instances(base, np.array(tc.E2E["instances"], F)))
    res, st = tc.E2E["res"], tc.E2E["settings"]
    w, h = res
    frames = [_render_planes(scene, tc.e2e_camera(mp, i), res, tc.E2E["spp"], tc.E2E["seeds"][i], tc.E2E["tile"]) for i in range(2)]
    torch.cuda.synchronize()
    for i in range(2):
        for k in ("shade", "position", "normal", "ids"):
            assert np.array_equal(bits(frames[i][k].cpu().numpy()), bits(e["planes"][i][k])), ("the renderer's plane differs from the oracle's", i, k)
    views = [mp.TemporalAccumulator.view_of(tc.e2e_camera(mp, i), res) for i in range(2)]
    assert np.array_equal(np.frombuffer(bytes(views[0]), np.uint32), bits(e["views"][0].floats()))
    # frame 1: reset
    first = {k: _guarded(torch, (h, w, 4)) for k in ("out", "moments_out")}
    tp.check(tp.lib().mpt_reset(0, w, h, frames[0]["shade"].data_ptr(), frames[0]["position"].data_ptr(), first["out"][1].data_ptr(),
                                first["moments_out"][1].data_ptr(), None))
    assert tp.last_kernels() == [K_RESET]
    torch.cuda.synchronize()
    _guards_intact(torch, first)
    assert np.array_equal(bits(_host(first["out"][1])), bits(e["first"][0])) and np.array_equal(bits(_host(first["moments_out"][1])), bits(e["first"][1]))
    # frame 2: reproject
    dev = {"color": (None, frames[1]["shade"]), "position": (None, frames[1]["position"]), "normal": (None, frames[1]["normal"]),
           "ids": (None, frames[1]["ids"]), "prev_position": (None, frames[0]["position"]), "prev_normal": (None, frames[0]["normal"]),
           "prev_ids": (None, frames[0]["ids"]), "hist_color": first["out"], "hist_moments": first["moments_out"]}
    got = _reproject(torch, dev, w, h, e["views"][0], st, False)
    for g, want, what in zip(got, e["second"], ("out", "moments_out", "variance_out")):
        assert np.array_equal(bits(g), bits(want)), what  # no NaN anywhere here
    # the classes, from what the GPU wrote: a miss has N = 0, a pixel without history N = 1 and its colour, the others N = 2
    classes = {k: v for k, v in m.classes(e["info"]).items()}
    N = got[1][..., 2]
    no_history = classes["ids"] | classes["position"] | classes["normal"] | classes["offscreen"]
    assert int((N == 0).sum()) == int(classes["miss"].sum()) >= tc.E2E_MIN_PER_CLASS
    assert np.array_equal(N == 2, classes["four_taps"] | classes["one_to_three_taps"])
    assert np.all(N[no_history] == 1) and np.array_equal(bits(got[0])[no_history], bits(frames[1]["shade"].cpu().numpy())[no_history])
    assert all(int(v.sum()) >= tc.E2E_MIN_PER_CLASS for v in classes.values())


def test_accumulator_over_four_frames(torch):
    """TemporalAccumulator on four frames of a moving camera gives the bits of four chained model calls, although the caller
    overwrites its guide tensors after every frame; after reset() a frame is a first frame; the result feeds the denoiser"""
    ctx = mp.Context(0)
    scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, ctx))
    res, spp = (72, 40), 8
    w, h = res
    acc = mp.TemporalAccumulator(res, 0, min_variance_history=3.0)
    dn = mp.AtrousDenoiser(res, 0)
    d = acc.settings
    model = m.Accumulator(sigma_position=d.sigma_position, normal_min=d.normal_min, max_history=d.max_history, alpha_color=d.alpha_color,
                          alpha_moments=d.alpha_moments, min_variance_history=d.min_variance_history, match_prim=False)
    with pytest.raises(ValueError):
        acc.history_length()
    expected_kernels = [K_RESET, K_VAR, K_VAR, K_VAR, K_RESET]
    for i in range(5):
        if i == 4:
            acc.reset()
            model.reset()
        cam = mp.Camera.default().look_at((0.3 * i, 2.0, 10.0), (0.1 * i, 1.5, 0.0), (0.0, 1.0, 0.0)).f_number(4.8).focus_distance(10.0)
        pl = _render_planes(scene, cam, res, spp, 40 + i)
        var_in = dn.variance_from_moments(pl["shade"], pl["shade_sq"], spp)
        host = {k: pl[k].cpu().numpy() for k in ("shade", "position", "normal", "ids")}
        host_var = var_in.cpu().numpy()
        view = mp.TemporalAccumulator.view_of(cam, res)
        out, var = acc.accumulate(pl["shade"], pl["position"], pl["normal"], pl["ids"], view, variance=var_in)
        assert acc.last_kernels() == [expected_kernels[i]]
        for k in ("shade", "position", "normal"):  # the caller reuses its tensors at once
            pl[k].fill_(float("nan"))
        pl["ids"].fill_(-1)
        var_in.fill_(float("nan"))
        center, forward, up, right = cam.center_forward_up_right()
        mview = m.view_of(center, forward, up, right, cam.focal_length, cam.build_sampler(res).as_array()[12], res)
        want_out, want_var = model.accumulate(host["shade"], host["position"], host["normal"], host["ids"], mview, variance=host_var)
        torch.cuda.synchronize()
        _same(out.cpu().numpy(), want_out, ("out", i))
        _same(var.cpu().numpy(), want_var, ("var", i))
        _same(acc.history_length().cpu().numpy(), model.prev["moments"][..., 2], ("history length", i))
        if i == 3:
            N = model.prev["moments"][..., 2]
            assert N.max() == 4 and (N == 1).sum() > 8 and (N == 0).sum() > 8  # full histories, fresh pixels and misses
            assert (want_var[..., 0][N >= 3] > 0).any() and np.array_equal(bits(want_var[..., 0][(N > 0) & (N < 3)]), bits(host_var[..., 0][(N > 0) & (N < 3)]))
        if i == 4:
            assert np.array_equal(bits(want_out), bits(host["shade"])) and np.all(model.prev["moments"][..., 2] <= 1)
    # into the denoiser with the temporal variance
    normal = torch.from_numpy(host["normal"]).cuda()
    clean, clean_var = dn.denoise(out, normal, variance=var)
    assert dn.last_kernels() == ["atrous_kernel<true>"]
    s = dn.settings
    want = denoise_model.atrous(want_out, host["normal"], variance=want_var, iterations=s.iterations, k=int(s.sigma_normal_pow2),
                                sigma_depth=s.sigma_depth, sigma_luminance=s.sigma_luminance)
    _same(clean.cpu().numpy(), want[0], "denoised colour")
    _same(clean_var.cpu().numpy(), want[1], "denoised variance")


def test_accumulator_checks_its_planes(torch):
    acc = mp.TemporalAccumulator((8, 4), 0)
    good = torch.zeros((4, 8, 4), device="cuda")
    ids = torch.zeros((4, 8, 4), dtype=torch.int32, device="cuda")
    view = mp.TemporalAccumulator.view_of(mp.Camera.teapot_view(), (8, 4))
    for bad in (good[:, :4], good.cpu(), good.double(), torch.zeros((8, 4, 4), device="cuda"), None):
        with pytest.raises(ValueError):
            acc.accumulate(bad, good, good, ids, view)
        with pytest.raises(ValueError):
            acc.accumulate(good, good, bad, ids, view)
    with pytest.raises(ValueError):
        acc.accumulate(good, good, good, good, view)  # ids are integers
    with pytest.raises(ValueError):
        acc.accumulate(good, good, good, ids, None)
    with pytest.raises(mp.MinipathError):
        mp.TemporalAccumulator((8, 4), 0, alpha_color=1.5)
    out, var = acc.accumulate(good, good, good, ids, view)
    assert acc.last_kernels() == [K_RESET] and tuple(out.shape) == (4, 8, 4) and float(acc.history_length().max()) == 0  # all misses
