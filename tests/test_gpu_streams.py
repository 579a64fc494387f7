"""GPU tests of the calling context the drivers promise beyond the null stream: "on the current torch stream without a host
synchronisation".  torch's side streams do not block against the null stream, so a launch on the wrong stream or a stray
synchronous call gives the right bits in every other test of the suite and wrong pixels in a pipelined frame loop.

The method, for every stage (stalled() below): on one side stream S a delay is enqueued, then device-to-device copies of the TRUE
inputs into input buffers that hold a POISON (the inputs of another valid case: tests/stream_cases.py), then the stage through its
Python driver, then clones of its results.  An event recorded right after the delay must still be unfinished once the host has
enqueued all of this -- else the stage waited for the stream somewhere, or the delay was too short, and the test fails: it would
have proved nothing.  After S.synchronize() the clones must be the model's bits on the true inputs.  A kernel launched on another
stream runs while S still sleeps, reads the poison and gives the model's bits on the poison instead, which differ
(tests/test_stream_cases_cpu.py); the positive controls do exactly that on purpose, once per library, and must see it.  Before its
stalled run every stage runs once, un-stalled, on the poison: that loads the library's code, fills the tile-list cache, and shows
that the GPU gives model(poison) on the poison.  The side stream is one that is shown not to share a hardware queue with the null
stream (the fixture `side`): on a shared queue the two run in order and the method could not tell a wrong stream from the right one.

Then: two driver objects on two streams, called alternately, for the stages that keep state (and one shared Context for the two
that trace).  No graph capture; nothing here provokes a fault; every kernel involved runs elsewhere in the suite at these sizes."""
import ctypes as C
import time

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib
from minipath_amd import adaptive as ad
from minipath_amd import denoise as dn
from minipath_amd import lights as ll
from minipath_amd import resample as rs
from minipath_amd import secondary as sv
from minipath_amd import temporal as tp
from tests import adaptive_model as am
from tests import aov_pass_model
from tests import lights_model as lm
from tests import resample_model as rm
from tests import secondary_cases as sc
from tests import secondary_model as sm
from tests import stream_cases as cases
from tests.conftest import TEAPOT
from tests.stream_cases import BATCH, F, H, SAMPLES, W, bits, differing

pytestmark = pytest.mark.gpu

DELAY_MS = 250.0  # the stall: the host enqueues a stage in a few milliseconds (the margins are printed)
MARGINS = []      # (what, milliseconds between the end of enqueueing and the end of the delay)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module", autouse=True)
def _own_hip_errors_only(torch):
    """As in tests/test_gpu_temporal.py: what earlier test modules left in HIP's sticky per-thread error state is not this module's."""
    import gc

    gc.collect()
    buf = torch.empty((4, 1, 1, 4), dtype=torch.float32, device="cuda")
    tp.check(tp.lib().mpt_reset(0, 1, 1, buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), buf[3].data_ptr(), None))
    torch.cuda.synchronize()
    yield
    if MARGINS:
        print("\nstream tests: delay %.0f ms; smallest margin %.1f ms (%s), largest %.1f ms, over %d stalled runs"
              % (DELAY_MS, min(MARGINS, key=lambda m: m[1])[1], min(MARGINS, key=lambda m: m[1])[0], max(m[1] for m in MARGINS), len(MARGINS)))


@pytest.fixture(scope="module")
def ctx(torch):
    return mp.Context(0)


@pytest.fixture(scope="module")
def teapot(ctx):
    return mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, ctx))


class Delay:
    """DELAY_MS of work on the current stream: torch.cuda._sleep where it exists, its cycles per millisecond measured once, else
    in-place elementwise passes over a large tensor, counted the same way"""

    def __init__(self, torch):
        self.torch = torch
        self.big = None
        self.sleep = getattr(torch.cuda, "_sleep", None)
        unit = 1_000_000
        if self.sleep is not None:
            ms = self._time(lambda: self.sleep(unit))
            if ms < 0.05:  # a sleep that does not sleep
                self.sleep = None
        if self.sleep is None:
            self.big = torch.zeros(32 << 20, dtype=torch.float32, device="cuda")
            unit = 1
            ms = self._time(lambda: self.big.add_(1.0))
        self.count = max(1, int(unit * DELAY_MS / ms))
        self.measured = self._time(self.enqueue)
        assert 0.5 * DELAY_MS < self.measured < 4 * DELAY_MS, (self.measured, self.count)

    def _time(self, work):
        torch = self.torch
        work()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        work()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def enqueue(self, part=1.0):
        count = max(1, int(self.count * part))
        if self.sleep is not None:
            self.sleep(count)
        else:
            for _ in range(count):
                self.big.add_(1.0)


@pytest.fixture(scope="module")
def delay(torch):
    d = Delay(torch)
    print("\ndelay: %s x %d = %.1f ms" % ("torch.cuda._sleep" if d.sleep is not None else "add_ on 128 MiB", d.count, d.measured))
    return d


@pytest.fixture(scope="module")
def side(torch, delay):
    """A side stream on which a delay does not hold up the null stream.  Streams share a few hardware queues, and two streams on one
    queue run in order whatever their flags say: a kernel on the null stream would then wait behind the delay, and neither a
    launch on the wrong stream nor the positive controls could be told from the real thing.  So candidates are probed with a
    tenth of the delay; the streams of torch's pool keep their queues.  Without such a stream the first is taken, and the positive
    controls fail and say so."""
    probe = torch.zeros(64, device="cuda")
    first = None
    for _ in range(16):
        s = torch.cuda.Stream()
        first = first or s
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            delay.enqueue(0.1)
            after = torch.cuda.Event()
            after.record(s)
        probe.add_(1.0)
        torch.cuda.default_stream().synchronize()
        independent = not after.query()
        torch.cuda.synchronize()
        if independent:
            return s
    return first


def _up(torch, a):
    """a host array on the device, uint32 as int32 words"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _host(t):
    return t.cpu().numpy()


def _same(got, want, what):
    """zero differing words; arrays of the model's shape or flat"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.size == want.size and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, got.dtype, want.shape, want.dtype)
    got = got.reshape(want.shape)
    if got.dtype.itemsize == 4 and want.dtype == F:
        got = got.view(F)
    n = differing(got, want)
    assert n == 0, (what, n, np.argwhere(bits(got) != bits(want))[:4].tolist())


def _same_all(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        _same(got[k], want[k], (what, k))


def stalled(torch, delay, S, what, pairs, body):
    """`pairs`: [(input buffer holding the poison, device tensor of its true contents)]; body() -> {name: result tensor}, called
    under the side stream S.  Returns the results on the host."""
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        delay.enqueue()
        after_delay = torch.cuda.Event()
        after_delay.record(S)
        for dst, src in pairs:
            dst.copy_(src, non_blocking=True)
        clones = {k: v.clone() for k, v in body().items()}
    t0 = time.perf_counter()
    unfinished = not after_delay.query()
    assert unfinished, f"{what}: delay too short: the delay had ended when the host had enqueued the stage (it waited for the stream, or took {DELAY_MS} ms)"
    after_delay.synchronize()
    MARGINS.append((what, (time.perf_counter() - t0) * 1e3))
    S.synchronize()
    return {k: _host(v) for k, v in clones.items()}


def _stage(torch, delay, side, what, case, make_body):
    """the un-stalled run on the poison (a driver object of its own), then the stalled run: make_body() -> body(buffers) -> results"""
    poison = {k: _up(torch, v) for k, v in case.poison.items()}
    warm = make_body()(poison)
    torch.cuda.synchronize()
    _same_all({k: _host(v) for k, v in warm.items()}, case.want("model", "poison"), (what, "un-stalled, on the poison"))
    for k, v in case.poison.items():  # the inputs are only read
        _same(_host(poison[k]), v, (what, "input changed", k))
    true = {k: _up(torch, v) for k, v in case.true.items()}
    body = make_body()
    got = stalled(torch, delay, side, what, [(poison[k], true[k]) for k in true], lambda: body(poison))
    _same_all(got, case.want("model", "true"), what)


# ---- A. every stage behind a stalled side stream ----------------------------------------------------------------------------------
def _denoise_body():
    d = cases.DENOISE
    den = mp.AtrousDenoiser((W, H), 0, iterations=d["iterations"], sigma_normal_pow2=d["k"], sigma_depth=d["sigma_depth"],
                            sigma_luminance=d["sigma_luminance"])

    def body(b):
        color, variance = den.denoise(b["color"], b["normal"], variance=b["variance"])
        return {"color": color, "variance": variance, "moments": den.variance_from_moments(b["shade"], b["shade_sq"], cases.MOMENT_SAMPLES)}
    return body


def test_denoise_and_variance_from_moments(torch, delay, side):
    _stage(torch, delay, side, "denoise", cases.denoise(), _denoise_body)


def _temporal_view(case):
    return tp.TemporalView.from_buffer_copy(case.view.floats().tobytes())


def _temporal_body():
    acc = mp.TemporalAccumulator((W, H), 0, **cases.TEMPORAL)
    view = _temporal_view(cases.temporal())

    def body(b):
        """two frames: reset, then reproject; the first frame's planes are cloned before the second call"""
        acc.reset()
        out1, var1 = acc.accumulate(b["color1"], b["position1"], b["normal1"], b["ids1"], view)
        r = {"out1": out1.clone(), "var1": var1.clone()}
        out2, var2 = acc.accumulate(b["color2"], b["position2"], b["normal2"], b["ids2"], view, variance=b["variance2"])
        assert acc.last_kernels() == ["reproject_kernel<true>"]
        r.update(out2=out2, var2=var2)
        return r
    return body


def test_temporal_reset_and_reproject(torch, delay, side):
    _stage(torch, delay, side, "temporal", cases.temporal(), _temporal_body)


def _resample_body():
    r = mp.GuidedResampler((W, H), factor=cases.FACTOR, sigma_normal_pow2=cases.UP_K, sigma_plane=cases.UP_SIGMA)

    def body(b):
        position_lo, normal_lo, ids_lo = r.downsample(b["position"], b["normal"], b["ids"], phase=cases.PHASE)
        out = r.upsample(b["color_lo"], b["position"], b["normal"])
        return {"picks": r.picks, "position_lo": position_lo, "normal_lo": normal_lo, "ids_lo": ids_lo, "out": out}
    return body


def test_resample_down_then_up(torch, delay, side):
    _stage(torch, delay, side, "resample", cases.resample(), _resample_body)


def _secondary_body(scene):
    def make():
        vis = mp.SecondaryVisibility(scene, (W, H), batch=BATCH)
        ao, sun = sc.MODES["ao"], sc.MODES["sun_soft"]

        def body(b):
            """8 samples in batches of 3 + 3 + 2: generate -> mp_occluded_rays -> resolve three times, twice with ACCUMULATE"""
            out, counts = vis.ambient_occlusion(b["position"], b["normal"], sc.EYE, SAMPLES, ao["radius"], seed=sc.SEED, bias=ao["bias"])
            r = {"ao_out": out.clone(), "ao_counts": counts.clone()}  # the next call overwrites the object's planes
            out, counts = vis.sun_visibility(b["position"], b["normal"], sc.EYE, sun["light"], SAMPLES, spread=sun["spread"], radius=sun["radius"],
                                             seed=sc.SEED, bias=sun["bias"])
            r.update(sun_soft_out=out, sun_soft_counts=counts)
            return r
        return body
    return make


def test_secondary_visibility(torch, delay, side, oracle, teapot):
    _stage(torch, delay, side, "secondary", cases.secondary(oracle), _secondary_body(teapot))


def _lights_body(scene, case):
    def make():
        lights = mp.LocalLights(scene, case.res, batch=BATCH)

        def body(b):
            out, sums = lights.irradiance(b["position"], b["normal"], [float(v) for v in case.eye], case.table, SAMPLES, seed=case.seed, **case.kw)
            return {"out": out, "sums": sums}
        return body
    return make


def test_local_lights(torch, delay, side, oracle, teapot):
    case = cases.lights(oracle)
    _stage(torch, delay, side, "lights", case, _lights_body(teapot, case))


def _queries_body(torch, obj):
    def make():
        def body(b):
            r = obj.intersect(b["o"], b["d"], full=True, tmax=b["tmax"])
            r["occluded"] = obj.occluded(b["o"], b["d"], tmax=b["tmax"]).view(torch.uint8)
            return r
        return body
    return make


def test_ray_queries_with_a_bound_per_ray(torch, delay, side, oracle, teapot):
    _stage(torch, delay, side, "ray queries", cases.queries(oracle), _queries_body(torch, teapot.object))


# The renders' inputs are the running sums of the earlier passes.  True: the state after the first FIRST samples of the frame;
# poison: that state of the frame with another seed.  The stalled run copies the true state in, renders the remaining samples on
# top and un-tiles; the frame is the oracle's.
RENDER = dict(tile=16, spp=8, res=(W, H), seed=41, first=3)


def _frame_renderer(scene, seed, max_depth=0):
    st = mp.RenderSettings(RENDER["tile"], RENDER["spp"], RENDER["res"], seed=seed, max_depth=max_depth)
    return mp.FrameRenderer(scene, mp.Camera.teapot_view(), st)


def _oracle_sampler(oracle):
    return oracle.build_sampler(oracle.teapot_camera(), W, H)


@pytest.mark.parametrize("max_depth", [0, 8], ids=["primary", "paths_depth8"])
def test_render_pass(torch, delay, side, oracle, teapot, teapot_oracle_bvh, max_depth):
    """FrameRenderer.render_pass and untile; at depth 8 the path kernels with their asynchronous pool and work-queue heads"""
    c = RENDER
    other = _frame_renderer(teapot, c["seed"] + 1, max_depth)  # the poison, and the un-stalled run of the same kernels and tile list
    other.render_pass(0, c["first"])
    poison = other.tile_buf.clone()
    other.render_pass(c["first"])
    other.untile()
    fr = _frame_renderer(teapot, c["seed"], max_depth)
    fr.render_pass(0, c["first"])
    true = fr.tile_buf.clone()
    fr.tile_buf.copy_(poison)
    torch.cuda.synchronize()
    assert differing(_host(true), _host(poison)) >= cases.MIN_DIFFERENT

    def body():
        fr.render_pass(c["first"])
        img, img8 = fr.untile()
        return {"image": img, "u8": img8}
    got = stalled(torch, delay, side, f"render_pass, depth {max_depth}", [(fr.tile_buf, true)], body)
    s = _oracle_sampler(oracle)
    if max_depth:
        want, want8 = teapot_oracle_bvh.render_tile_paths(s, W, H, c["spp"], c["seed"], max_depth, 0, 0, W, H)[:2]
    else:
        want, want8 = teapot_oracle_bvh.render_tile(s, W, H, c["spp"], c["seed"], 0, 0, W, H)
    assert (want[..., 3] > 0).sum() >= cases.MIN_DIFFERENT
    _same(got["image"], want, "image")
    assert np.array_equal(got["u8"], want8)


def test_render_aov_pass_and_untile_plane(torch, delay, side, oracle, teapot, teapot_oracle_bvh):
    c = RENDER
    names = mp.FrameRenderer.AOV_PLANES
    other = _frame_renderer(teapot, c["seed"] + 1)
    poison = other.new_aov_planes(position=True, shade_sq=True)
    other.render_aov_pass(poison, 0, c["first"])
    fr = _frame_renderer(teapot, c["seed"])
    true = fr.new_aov_planes(position=True, shade_sq=True)
    fr.render_aov_pass(true, 0, c["first"])
    planes = {k: poison[k].clone() for k in names}
    done = {k: v.clone() for k, v in poison.items()}  # the un-stalled run of the same kernels and tile list
    other.render_aov_pass(done, c["first"])
    for k in names:
        other.untile_plane(done[k])
    torch.cuda.synchronize()
    assert all(differing(_host(true[k]), _host(poison[k])) >= cases.MIN_DIFFERENT for k in names)

    def body():
        fr.render_aov_pass(planes, c["first"])
        return {k: fr.untile_plane(planes[k]) for k in names}
    got = stalled(torch, delay, side, "render_aov_pass", [(planes[k], true[k]) for k in names], body)
    want = aov_pass_model.planes(oracle, teapot_oracle_bvh.intersect, _oracle_sampler(oracle), W, c["spp"], c["seed"], (0, 0, W, H))
    _same_all(got, want, "feature planes")


ADAPTIVE_PLANES = ("shade", "shade_sq", "normal")


def _sampler(scene, threshold, seed=am.CASE["seed"]):
    c = am.CASE
    st = mp.RenderSettings(c["ts"], c["spp"], c["res"], seed=seed)
    return mp.AdaptiveSampler(scene, mp.Camera.teapot_view(), st, threshold, floor=c["floor"], min_samples=c["min_samples"],
                              round_samples=c["round_samples"], planes=ADAPTIVE_PLANES)


def _owned(tiles, ts):
    own = np.zeros((len(tiles), ts, ts), bool)
    for i, t in enumerate(tiles):
        own[i, : t.height(), : t.width()] = True
    return own


def _same_owned(got, want, own, what):
    for k in ADAPTIVE_PLANES:
        n = int(np.sum(bits(got[k])[own] != bits(want[k])[own]))
        assert n == 0, (what, k, n)


def test_adaptive_last_step_and_finish(torch, delay, side, teapot):
    """the case of tests/adaptive_model.py: three rounds as usual (each ends with the round's synchronisation, which the driver
    documents), then, stalled, the last round -- gather, render, scatter; it has no check -- and finish().  True: the sampler's own
    planes after three rounds; poison: those of a sampler with another seed.  A sampler of the same case runs to its end first: the
    tile lists of its rounds are then in the context's cache."""
    _, exp, tiles = am.teapot_case()
    assert len(exp.bounds) == 5
    _sampler(teapot, am.CASE["threshold"]).render()
    other, smp = _sampler(teapot, am.CASE["threshold"], seed=am.CASE["seed"] + 1), _sampler(teapot, am.CASE["threshold"])
    for _ in range(3):
        assert other.step() and smp.step()
    assert smp.active and len(smp.active) < len(tiles), "the last round is a compact one"
    true = {k: v.clone() for k, v in smp.planes.items()}
    for k in smp.planes:
        smp.planes[k].copy_(other.planes[k])
    torch.cuda.synchronize()
    own = _owned(tiles, am.CASE["ts"])
    assert all(int(np.sum(bits(_host(true[k]))[own] != bits(_host(other.planes[k]))[own])) >= cases.MIN_DIFFERENT for k in ADAPTIVE_PLANES)

    def body():
        assert smp.step() is True and smp.active == []
        smp.finish()
        return dict(smp.planes)
    got = stalled(torch, delay, side, "adaptive", [(smp.planes[k], true[k]) for k in true], body)
    _same_owned(got, exp.planes, own, "finished frame")
    assert np.array_equal(smp.samples, exp.samples)


# ---- the positive controls: one call per library on the NULL stream while the side stream is stalled -------------------------------
def _control(torch, delay, S, what, case, call, outputs):
    """`call(buffers, outs)` makes the library's call with stream = None; outs: {name: (shape, torch dtype)}.  The call reads the
    poison, because the copies of the true inputs wait behind the delay on another stream"""
    bufs = {k: _up(torch, v) for k, v in case.poison.items()}
    true = {k: _up(torch, v) for k, v in case.true.items()}
    outs = {k: torch.zeros(shape, dtype=dt, device="cuda") for k, (shape, dt) in outputs.items()}
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        delay.enqueue()
        after_delay = torch.cuda.Event()
        after_delay.record(S)
        for k in bufs:
            bufs[k].copy_(true[k], non_blocking=True)
    call(bufs, outs)
    torch.cuda.default_stream().synchronize()
    if after_delay.query():
        pytest.fail(f"{what}: a call on the null stream waited for the delay on the side stream: the delay method has no teeth on this machine")
    torch.cuda.synchronize()
    got = {k: _host(v) for k, v in outs.items()}
    want_true, want_poison = case.want("control", "true"), case.want("control", "poison")
    if all(differing(got[k].reshape(want_true[k].shape), want_true[k]) == 0 for k in got):
        pytest.fail(f"{what}: a call on the null stream waited for the side stream: the delay method has no teeth on this machine")
    _same_all(got, want_poison, (what, "control"))
    for k in bufs:  # and the copies did land afterwards
        _same(_host(bufs[k]), case.true[k], (what, "true input", k))


def _p(t):
    return t.data_ptr()


def test_control_denoise(torch, delay, side):
    def call(b, o):
        dn.check(dn.lib().mpd_variance_from_moments(0, W, H, cases.MOMENT_SAMPLES, _p(b["shade"]), _p(b["shade_sq"]), _p(o["moments"]), None))
    _control(torch, delay, side, "denoise", cases.denoise(), call, {"moments": ((H, W, 4), torch.float32)})


def test_control_temporal(torch, delay, side):
    def call(b, o):
        tp.check(tp.lib().mpt_reset(0, W, H, _p(b["color1"]), _p(b["position1"]), _p(o["out"]), _p(o["moments"]), None))
    _control(torch, delay, side, "temporal", cases.temporal(), call, {k: ((H, W, 4), torch.float32) for k in ("out", "moments")})


def _resample_settings():
    return rs.ResampleSettings(C.sizeof(rs.ResampleSettings), W, H, cases.FACTOR, rs.MPR_PICK_PHASE, cases.PHASE, float(cases.UP_K), cases.UP_SIGMA)


def test_control_resample(torch, delay, side):
    lw, lh = rm.low_size(W, H, cases.FACTOR)

    def call(b, o):
        st = _resample_settings()
        src = rs.pointer_array([_p(b[k]) for k in ("position", "normal", "ids")])
        dst = rs.pointer_array([_p(o[k]) for k in ("position_lo", "normal_lo", "ids_lo")])
        rs.check(rs.lib().mpr_downsample(0, C.byref(st), _p(b["position"]), _p(b["normal"]), 3, src, dst, _p(o["picks"]), None))
    outs = {"picks": ((lh, lw), torch.int32), "position_lo": ((lh, lw, 4), torch.float32), "normal_lo": ((lh, lw, 4), torch.float32),
            "ids_lo": ((lh, lw, 4), torch.int32)}
    _control(torch, delay, side, "resample", cases.resample(), call, outs)


def _secondary_settings(mode_kw, batch, begin, flags=0):
    st = sv.SecondarySettings(C.sizeof(sv.SecondarySettings), W, H, mode_kw["mode"], flags, SAMPLES, begin, batch, sc.SEED)
    st.eye[:], st.light[:] = sc.EYE, mode_kw.get("light", (0.0, 0.0, 1.0))
    st.radius, st.bias, st.spread = mode_kw["radius"], mode_kw["bias"], mode_kw.get("spread", 0.0)
    return st


def test_control_secondary(torch, delay, side, oracle):
    def call(b, o):
        st = _secondary_settings(sc.MODES["sun_soft"], BATCH, 0)
        sv.check(sv.lib().mps_generate(0, C.byref(st), _p(b["position"]), _p(b["normal"]), *[_p(o[k]) for k in sm.RAY_ARRAYS], None))
    _control(torch, delay, side, "secondary", cases.secondary(oracle), call, {k: ((W * H * BATCH,), torch.float32) for k in sm.RAY_ARRAYS})


def _lights_settings(case, batch, begin, flags=0, res=None):
    w, h = res or case.res
    st = ll.LightsSettings(C.sizeof(ll.LightsSettings), w, h, flags, SAMPLES, begin, batch, len(case.table), case.seed)
    st.eye[:] = [float(v) for v in case.eye]
    st.bias, st.margin = case.kw["bias"], case.kw["margin"]
    return st


def test_control_lights(torch, delay, side, oracle):
    case = cases.lights(oracle)
    n = case.res[0] * case.res[1] * BATCH * len(case.table)

    def call(b, o):
        st = _lights_settings(case, BATCH, 0)
        ll.check(ll.lib().mpl_generate(0, C.byref(st), ll.light_table(case.table), _p(b["position"]), _p(b["normal"]),
                                       *[_p(o[k]) for k in lm.RAY_ARRAYS], None))
    _control(torch, delay, side, "lights", case, call, {k: ((n,), torch.float32) for k in lm.RAY_ARRAYS})


def test_control_adaptive(torch, delay, side):
    case, c = cases.adaptive_check(), cases.CHECK
    wh = _up(torch, case.wh)

    def call(b, o):
        ad.check(ad.lib().mpa_tile_error(0, c["ts"], c["n"], c["k"], c["threshold"], c["floor"], _p(b["shade"]), _p(b["shade_sq"]), _p(wh),
                                         _p(o["open"]), _p(o["max_err"]), None))
    _control(torch, delay, side, "adaptive", case, call, {"open": ((c["n"],), torch.int32), "max_err": ((c["n"],), torch.float32)})


def test_control_ray_queries(torch, delay, side, oracle, ctx, teapot):
    case = cases.queries(oracle)

    def call(b, o):
        oc, dc = b["o"].t().contiguous(), b["d"].t().contiguous()  # on the null stream too
        _lib.check(_lib.lib().mp_occluded_rays(ctx.handle, teapot.object.handle, _p(oc[0]), _p(oc[1]), _p(oc[2]), _p(dc[0]), _p(dc[1]), _p(dc[2]),
                                               _p(b["tmax"]), cases.N_RAYS, _p(o["occluded"]), None))
    _control(torch, delay, side, "ray queries", case, call, {"occluded": ((cases.N_RAYS,), torch.uint8)})


# ---- two objects on two streams, called alternately ---------------------------------------------------------------------------------
def _two_streams(torch, what, case, make_body, rounds=3):
    """object 0 on the true inputs, object 1 on the poison (the other valid case), each on a stream of its own; each round's results
    are cloned on the object's stream, the last round's are compared"""
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    inputs = [{k: _up(torch, v) for k, v in case.true.items()}, {k: _up(torch, v) for k, v in case.poison.items()}]
    bodies = [make_body(), make_body()]
    torch.cuda.synchronize()
    got = [None, None]
    for _ in range(rounds):  # interleaved, so the two have work in flight together
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                got[i] = {k: v.clone() for k, v in bodies[i](inputs[i]).items()}
    torch.cuda.synchronize()
    for i, of in enumerate(("true", "poison")):
        _same_all({k: _host(v) for k, v in got[i].items()}, case.want("model", of), (what, "stream", i))


def test_two_streams_temporal(torch):
    _two_streams(torch, "temporal", cases.temporal(), _temporal_body)


def test_two_streams_resample(torch):
    _two_streams(torch, "resample", cases.resample(), _resample_body)


def test_two_streams_secondary_share_a_context(torch, oracle, teapot):
    _two_streams(torch, "secondary", cases.secondary(oracle), _secondary_body(teapot))


def test_two_streams_lights_share_a_context(torch, oracle, teapot):
    case = cases.lights(oracle)
    _two_streams(torch, "lights", case, _lights_body(teapot, case))


def test_two_streams_adaptive(torch, teapot):
    """two samplers of one scene with two thresholds, stepped alternately to their ends: each frame is its own model's"""
    frame, exp, tiles = am.teapot_case()
    c = am.CASE
    other = am.Expected(frame, tiles, c["ts"], 0.1, c["floor"], c["min_samples"], c["round_samples"])
    assert not np.array_equal(other.samples, exp.samples)
    want, thresholds = [exp, other], [c["threshold"], 0.1]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    samplers = [_sampler(teapot, t) for t in thresholds]
    torch.cuda.synchronize()
    busy = [True, True]
    while any(busy):
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                busy[i] = samplers[i].step()
    for i in (0, 1):
        with torch.cuda.stream(streams[i]):
            samplers[i].finish()
    torch.cuda.synchronize()
    own = _owned(tiles, c["ts"])
    for i in (0, 1):
        _same_owned({k: _host(v) for k, v in samplers[i].planes.items()}, want[i].planes, own, ("adaptive, stream", i))
        assert np.array_equal(samplers[i].samples, want[i].samples)


# ---- B. offset buffers ------------------------------------------------------------------------------------------------------------
# Every other GPU test puts its buffers on 16-byte boundaries (a fresh allocation, or 4096 elements into one).  The headers ask that
# of planes only: a ray array may start at any word and `occluded` at any byte.  Here every ray array starts at another odd word of
# its 16 bytes, `occluded` 1, 2 and 3 bytes past a boundary, all between guards; and the drivers get planes that are aligned views
# into larger tensors (a storage offset that is not zero).
SENTINEL = 0x5A5A5A5A
PAD = 4096
WORD_OFFSETS = (1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 14, 15)  # words past a 16-byte boundary: 4, 8 or 12 bytes into their 16


class Guarded:
    """a host array (or `shape` sentinels) on the device, `offset` elements past a 16-byte boundary in the middle of a larger tensor
    of sentinels; 4-byte elements, or bytes"""

    def __init__(self, torch, a, offset, dtype=None):
        shape = a if isinstance(a, tuple) else a.shape
        self.n, self.offset, self.shape = int(np.prod(shape)), offset, shape
        byte = dtype is not None
        self.fill = SENTINEL & 0xFF if byte else SENTINEL
        self.whole = torch.full((PAD + 16 + self.n + PAD,), self.fill, dtype=dtype if byte else torch.int32, device="cuda")
        assert self.whole.data_ptr() % 16 == 0
        self.view = self.whole[PAD + offset:PAD + offset + self.n]
        if not isinstance(a, tuple):
            host = np.ascontiguousarray(a).reshape(-1)
            self.view.copy_(torch.from_numpy(host if byte else host.view(np.int32)))
        self.ptr = self.view.data_ptr()
        assert self.ptr % 16 == (offset * (1 if byte else 4)) % 16

    def host(self, dtype=F):
        a = self.view.cpu().numpy()
        return (a if a.dtype.itemsize == 1 else a.view(dtype)).reshape(self.shape)

    def guards_intact(self):
        raw = self.whole.cpu().numpy()
        lo = PAD + self.offset
        return bool(np.all(raw[:lo] == self.fill) and np.all(raw[lo + self.n:] == self.fill))


def _offsets(names, turn):
    """another odd word offset for every array, turned by `turn`"""
    return {k: WORD_OFFSETS[(i + 4 * turn) % len(WORD_OFFSETS)] for i, k in enumerate(names)}


def _check_guards(buffers):
    for k, g in buffers.items():
        assert g.guards_intact(), k


@pytest.mark.parametrize("occluded_at", [1, 2, 3])
def test_secondary_rays_at_odd_offsets(torch, oracle, occluded_at):
    from tests import secondary_cases as tc

    mode_name = list(tc.MODES)[occluded_at - 1]
    case, kw = tc.synthetic(W, H), tc.MODES[mode_name]
    want, _ = tc.generated(oracle, W, H, mode_name, BATCH, 0)
    off = _offsets(sm.RAY_ARRAYS, occluded_at)
    planes = {k: Guarded(torch, case[k], 0) for k in ("position", "normal")}
    rays = {k: Guarded(torch, (BATCH * H * W,), off[k]) for k in sm.RAY_ARRAYS}
    st = _secondary_settings(kw, BATCH, 0)
    sv.check(sv.lib().mps_generate(0, C.byref(st), planes["position"].ptr, planes["normal"].ptr, *[rays[k].ptr for k in sm.RAY_ARRAYS], None))
    torch.cuda.synchronize()
    for k in sm.RAY_ARRAYS:
        _same(rays[k].host(), want[k], (mode_name, k))
    _check_guards({**planes, **rays})
    # resolve: tmax at an odd word, occluded at an odd byte, continuing earlier counts
    r = tc.resolve_inputs(W, H, BATCH)
    dev = {"tmax": Guarded(torch, r["tmax"], WORD_OFFSETS[occluded_at]), "occluded": Guarded(torch, r["occluded"], occluded_at, torch.uint8)}
    outs = {"counts": Guarded(torch, r["counts"], 0), "out": Guarded(torch, (H, W, 4), 0)}
    st = _secondary_settings(tc.MODES["ao"], BATCH, 0, flags=sv.MPS_FLAG_ACCUMULATE)
    sv.check(sv.lib().mps_resolve(0, C.byref(st), dev["tmax"].ptr, dev["occluded"].ptr, outs["counts"].ptr, outs["out"].ptr, None))
    torch.cuda.synchronize()
    want_counts, want_out = sm.resolve(r["tmax"], r["occluded"], (H, W), BATCH, counts=r["counts"], want_out=True)
    _same(outs["counts"].host(), want_counts, "counts")
    _same(outs["out"].host(), want_out, "out")
    _check_guards({**dev, **outs})
    assert np.array_equal(dev["occluded"].host(), r["occluded"]) and np.array_equal(bits(dev["tmax"].host()), bits(r["tmax"]))


@pytest.mark.parametrize("occluded_at", [1, 2, 3])
def test_light_rays_at_odd_offsets(torch, oracle, occluded_at):
    from tests import lights_cases as tc

    table_name = list(tc.TABLES)[occluded_at - 1]
    case, lights = tc.synthetic(W, H), tc.TABLES[table_name]
    L = len(lights)
    want, _ = tc.generated(oracle, W, H, table_name, BATCH, 0)
    off = _offsets(lm.RAY_ARRAYS, occluded_at)
    planes = {k: Guarded(torch, case[k], 0) for k in ("position", "normal")}
    rays = {k: Guarded(torch, (BATCH * L * H * W,), off[k]) for k in lm.RAY_ARRAYS}

    def settings(flags=0):
        st = ll.LightsSettings(C.sizeof(ll.LightsSettings), W, H, flags, tc.SAMPLE_COUNT, 0, BATCH, L, tc.SEED)
        st.eye[:] = tc.EYE
        st.bias, st.margin = tc.BIAS, tc.MARGIN
        return st
    st = settings()
    ll.check(ll.lib().mpl_generate(0, C.byref(st), ll.light_table(lights), planes["position"].ptr, planes["normal"].ptr,
                                   *[rays[k].ptr for k in lm.RAY_ARRAYS], None))
    torch.cuda.synchronize()
    for k in lm.RAY_ARRAYS:
        _same(rays[k].host(), want[k], (table_name, k))
    _check_guards({**planes, **rays})
    r = tc.resolve_inputs(W, H, BATCH, table_name)
    dev = {"tmax": Guarded(torch, r["tmax"], WORD_OFFSETS[occluded_at]), "weight": Guarded(torch, r["weight"], WORD_OFFSETS[occluded_at + 3]),
           "occluded": Guarded(torch, r["occluded"], occluded_at, torch.uint8)}
    outs = {"sums": Guarded(torch, r["sums"], 0), "out": Guarded(torch, (H, W, 4), 0)}
    st = settings(ll.MPL_FLAG_ACCUMULATE)
    ll.check(ll.lib().mpl_resolve(0, C.byref(st), ll.light_table(lights), dev["tmax"].ptr, dev["weight"].ptr, dev["occluded"].ptr, outs["sums"].ptr,
                                  outs["out"].ptr, None))
    torch.cuda.synchronize()
    want_sums, want_out = lm.resolve(r["tmax"], r["weight"], r["occluded"], lights, (H, W), BATCH, sums=r["sums"], want_out=True)
    _same(outs["sums"].host(), want_sums, "sums")
    _same(outs["out"].host(), want_out, "out")
    _check_guards({**dev, **outs})


@pytest.mark.parametrize("occluded_at", [1, 2, 3])
def test_ray_queries_at_odd_offsets(torch, oracle, ctx, teapot, occluded_at):
    """mp_trace_rays_bounded and mp_occluded_rays: the six ray arrays, the bounds and every array of the hit records at odd words,
    `occluded` at an odd byte"""
    case = cases.queries(oracle)
    i, n = case.true, cases.N_RAYS
    orc = case.oracle_scene
    cols = {"ox": i["o"][:, 0], "oy": i["o"][:, 1], "oz": i["o"][:, 2], "dx": i["d"][:, 0], "dy": i["d"][:, 1], "dz": i["d"][:, 2], "tmax": i["tmax"]}
    off = _offsets(cols, occluded_at)
    rays = {k: Guarded(torch, v, off[k]) for k, v in cols.items()}
    want = case.want("model", "true")
    full = ("t", "prim", "u", "v", "point", "normal", "tex", "material", "instance")
    hoff = _offsets(full, occluded_at + 1)
    hits = {k: Guarded(torch, want[k].shape, hoff[k]) for k in full}
    occluded = Guarded(torch, (n,), occluded_at, torch.uint8)
    soa = _lib.HitsSoA(*[hits[k].ptr for k in full])
    args = [rays[k].ptr for k in cols]
    _lib.check(_lib.lib().mp_trace_rays_bounded(ctx.handle, teapot.object.handle, *args, n, C.byref(soa), None))
    _lib.check(_lib.lib().mp_occluded_rays(ctx.handle, teapot.object.handle, *args, n, occluded.ptr, None))
    torch.cuda.synchronize()
    for k in full:
        _same(hits[k].host(want[k].dtype), want[k], k)
    _same(occluded.host(), want["occluded"], "occluded")
    _check_guards({**rays, **hits, "occluded": occluded})
    assert orc is not None and int(want["occluded"].sum()) >= cases.MIN_DIFFERENT


def _views(torch, inputs, lead):
    """the inputs as views `lead` floats into larger tensors: contiguous, aligned, with a storage offset"""
    out = {}
    for k, a in inputs.items():
        t = _up(torch, a)
        whole = torch.zeros(lead + t.numel() + 8, dtype=t.dtype, device="cuda")
        v = whole[lead:lead + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.storage_offset() == lead and v.data_ptr() % 16 == 0 and v.data_ptr() != whole.data_ptr()
        out[k] = v
    return out


LEADS = [4, 1024 + 4]  # floats: 16 bytes, and 4096 + 16 bytes


@pytest.mark.parametrize("lead", LEADS, ids=lambda v: "%dB" % (4 * v))
@pytest.mark.parametrize("stage", ["denoise", "temporal", "resample", "secondary", "lights"])
def test_drivers_take_aligned_views(torch, oracle, teapot, stage, lead):
    """the bits of fresh tensors (the model's), from planes that begin inside larger tensors"""
    if stage == "secondary":
        case, make = cases.secondary(oracle), _secondary_body(teapot)
    elif stage == "lights":
        case = cases.lights(oracle)
        make = _lights_body(teapot, case)
    else:
        case, make = getattr(cases, stage)(), {"denoise": _denoise_body, "temporal": _temporal_body, "resample": _resample_body}[stage]
    got = make()(_views(torch, case.true, lead))
    torch.cuda.synchronize()
    _same_all({k: _host(v) for k, v in got.items()}, case.want("model", "true"), (stage, lead))


@pytest.mark.parametrize("lead", LEADS, ids=lambda v: "%dB" % (4 * v))
def test_adaptive_sampler_on_aligned_views(torch, teapot, lead):
    """the sampler's canonical planes replaced, before the first round, by zeroed views that begin inside larger tensors"""
    _, exp, tiles = am.teapot_case()
    smp = _sampler(teapot, am.CASE["threshold"])
    smp.planes = _views(torch, {k: np.zeros(tuple(v.shape), F) for k, v in smp.planes.items()}, lead)
    smp.render()
    torch.cuda.synchronize()
    _same_owned({k: _host(v) for k, v in smp.planes.items()}, exp.planes, _owned(tiles, am.CASE["ts"]), ("adaptive", lead))
    assert np.array_equal(smp.samples, exp.samples)


def test_a_misaligned_view_is_refused_by_the_driver_and_by_the_library(torch):
    """whole[1:1 + n].view(h, w, 4) is contiguous and starts 4 bytes off: the wrapper raises, and the library, given the pointer
    directly, refuses it and leaves the output alone"""
    case = cases.denoise()
    n = H * W * 4
    whole = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    off = whole[1:1 + n].view(H, W, 4)
    good = _up(torch, case.true["shade"])
    den = mp.AtrousDenoiser((W, H), 0)
    for args in ((off, good), (good, off)):
        with pytest.raises(ValueError, match="16-byte aligned"):
            den.variance_from_moments(*args, cases.MOMENT_SAMPLES)
    with pytest.raises(ValueError, match="16-byte aligned"):
        den.denoise(good, good, out=off)
    out = Guarded(torch, (H, W, 4), 1)
    before = dn.last_kernels()
    assert dn.lib().mpd_variance_from_moments(0, W, H, cases.MOMENT_SAMPLES, good.data_ptr(), good.data_ptr(), out.ptr, None) == 1
    assert dn.lib().mpd_last_error() == b"a plane is not 16-byte aligned" and dn.last_kernels() == before
    torch.cuda.synchronize()
    assert np.all(out.whole.cpu().numpy() == SENTINEL)
