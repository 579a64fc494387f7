"""The inputs of the stream-ordering tests (tests/test_gpu_streams.py), shared with the CPU test that shows they are not vacuous
(tests/test_stream_cases_cpu.py).  Every stage gets a Case: its TRUE inputs, a POISON of the same shapes and dtypes -- the inputs of
another valid case of the existing cases modules, so that the stage's model is defined on it --, the model of the whole stage
through its driver and the model of the one C ABI call the library's positive control makes.  A stage that reads its input buffers
before the copies of the true inputs have landed in them (a launch on the wrong stream) computes model(poison), not model(true);
the CPU test shows that the two differ in at least MIN_DIFFERENT words of every output.  Everything is made once and never changed.
"""
import functools

import numpy as np

from tests import denoise_model as dm
from tests import lights_cases as lc
from tests import lights_model as lm
from tests import ray_query_scenes as rq
from tests import resample_cases as rc
from tests import resample_model as rm
from tests import secondary_cases as sc
from tests import secondary_model as sm
from tests import temporal_cases as tc
from tests import temporal_model as tm
from tests.conftest import TEAPOT

F = np.float32
W, H = 37, 23         # the smallest ragged size every cases module carries
SAMPLES, BATCH = 8, 3  # 3 + 3 + 2: the three-call chains run three times, twice with ACCUMULATE
MIN_DIFFERENT = 16     # words of every output in which model(poison) differs from model(true): the MIN_PER_RULE of the cases modules


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint8)


def differing(got, want):
    """the number of differing words (bytes of a byte array), a NaN of `want` standing for any NaN as in the temporal tests"""
    got, want = np.asarray(got), np.asarray(want)
    diff = bits(got) != bits(want)
    if want.dtype == F:
        diff &= ~(np.isnan(want) & np.isnan(got))
    return int(diff.sum())


class Case:
    """true, poison: {name: array}; model(inputs) and control(inputs): {name: array}"""

    def __init__(self, true, poison, model, control, **extra):
        assert sorted(true) == sorted(poison)
        for k in true:
            assert true[k].shape == poison[k].shape and true[k].dtype == poison[k].dtype, k
        self.true, self.poison, self.model, self.control = true, poison, model, control
        self.constant = ()  # outputs that do not depend on the buffers' contents in this case, with the reason where they are named
        self.__dict__.update(extra)
        self._memo = {}

    def want(self, which="model", of="true"):
        """model or control of the true or the poison inputs, computed once"""
        if (which, of) not in self._memo:
            self._memo[which, of] = getattr(self, which)(getattr(self, of))
        return self._memo[which, of]


# ---- denoise ----------------------------------------------------------------------------------------------------------------------
DENOISE = dict(iterations=3, k=7, sigma_depth=0.4, sigma_luminance=0.8)  # tests/test_gpu_denoise.py's (37, 23, 3) with its sigmas
MOMENT_SAMPLES = 12


def _moment_planes(seed):
    """the shade and shade_sq planes of tests/test_gpu_denoise.py::test_variance_from_moments_matches_the_model for a seed"""
    rng = np.random.default_rng(seed)
    n = MOMENT_SAMPLES
    alpha = (rng.integers(0, n + 1, (H, W)) / n).astype(F)
    shade, sq = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
    c = rng.random((H, W, n)).astype(F) * (rng.random((H, W, n)) < alpha[..., None])
    shade[..., 0], sq[..., 0] = c.mean(-1), (c * c).mean(-1)
    shade[..., 3] = sq[..., 3] = alpha
    shade[alpha == 0, 0] = 5
    return shade, sq


@functools.lru_cache(maxsize=None)
def denoise():
    def inputs(seed, moment_seed):
        p = dm.synthetic(W, H, seed)
        shade, sq = _moment_planes(moment_seed)
        return {"color": p["color"], "normal": p["normal"], "variance": p["variance"], "shade": shade, "shade_sq": sq}

    def control(i):
        return {"moments": dm.variance_from_moments(i["shade"], i["shade_sq"], MOMENT_SAMPLES)}

    def model(i):
        c, v = dm.atrous(i["color"], i["normal"], variance=i["variance"], iterations=DENOISE["iterations"], k=DENOISE["k"],
                         sigma_depth=DENOISE["sigma_depth"], sigma_luminance=DENOISE["sigma_luminance"])
        return {"color": c, "variance": v, **control(i)}

    return Case(inputs(1000 * W + H, 7), inputs(4242, 8), model, control)


# ---- temporal ---------------------------------------------------------------------------------------------------------------------
TEMPORAL = tc.synthetic_settings(4.0, 0.0, True)


@functools.lru_cache(maxsize=None)
def temporal():
    """two frames: the synthetic case's previous frame through reset, its current frame through reproject under the case's view"""
    def inputs(case):
        cur, prev = case["cur"], case["prev"]
        return {"color1": prev["color"], "position1": prev["position"], "normal1": prev["normal"], "ids1": prev["ids"],
                "color2": cur["color"], "position2": cur["position"], "normal2": cur["normal"], "ids2": cur["ids"], "variance2": cur["variance"]}

    view = tc.synthetic(W, H)["view"]

    def control(i):
        out, moments = tm.reset(i["color1"], i["position1"])
        return {"out": out, "moments": moments}

    def model(i):
        first = control(i)
        out, _, var = tm.reproject(i["color2"], i["position2"], i["normal2"], i["ids2"], view, i["position1"], i["normal1"], i["ids1"], first["out"],
                                   first["moments"], variance_in=i["variance2"], **TEMPORAL)
        return {"out1": first["out"], "var1": np.zeros((H, W, 4), F), "out2": out, "var2": var}

    # var1: a first frame without a variance plane hands on zeros
    return Case(inputs(tc.synthetic(W, H)), inputs(tc.synthetic(W, H, True)), model, control, view=view, constant=("var1",))


# ---- resample ---------------------------------------------------------------------------------------------------------------------
FACTOR, PHASE = 3, 4
UP_K, UP_SIGMA = rc.UP_WEIGHTS[FACTOR]


@functools.lru_cache(maxsize=None)
def resample():
    c = rc.synthetic(W, H)
    color_lo = rc.upsample_inputs(W, H, FACTOR)["color_lo"]
    rng = np.random.default_rng(99)
    # the same planes turned by half a turn: the misses, and with them the picks, lie elsewhere
    other = {k: np.ascontiguousarray(c[k][::-1, ::-1]) for k in ("position", "normal")}
    other_color = np.concatenate([rng.uniform(0.0, 1.0, color_lo.shape[:2] + (3,)), np.ones(color_lo.shape[:2] + (1,))], -1).astype(F)
    true = {"position": c["position"], "normal": c["normal"], "ids": c["ids"], "color_lo": color_lo}
    poison = {"position": other["position"], "normal": other["normal"],
              "ids": rng.integers(-2 ** 31, 2 ** 31, c["ids"].shape, dtype=np.int64).astype(np.int32), "color_lo": other_color}

    def control(i):
        picks, lows = rm.downsample(i["position"], i["normal"], [i["position"], i["normal"], i["ids"]], FACTOR, rm.PICK_PHASE, PHASE)
        return {"picks": picks, "position_lo": lows[0], "normal_lo": lows[1], "ids_lo": lows[2]}

    def model(i):
        low = control(i)
        out = rm.upsample(i["position"], i["normal"], low["position_lo"], low["normal_lo"], low["picks"], i["color_lo"], FACTOR, UP_K, UP_SIGMA)
        return {**low, "out": out}

    return Case(true, poison, model, control)


# ---- secondary visibility and lights, over the teapot -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def teapot_bvh(po):
    return po.Bvh.from_obj(TEAPOT)


def _mode_kw(name):
    return {k: v for k, v in sc.MODES[name].items() if k != "mode"}


@functools.lru_cache(maxsize=None)
def secondary(po):
    """ambient occlusion and the soft sun of tests/secondary_cases.py on its synthetic planes, the lights' planes as poison"""
    eye = np.array(sc.EYE, F)
    pick = lambda c: {"position": c["position"], "normal": c["normal"]}  # noqa: E731

    def control(i):
        g = sm.generate(po, i["position"], i["normal"], seed=sc.SEED, sample_count=SAMPLES, sample_begin=0, batch=BATCH, eye=sc.EYE,
                        **sc.MODES["sun_soft"])  # the sun: which rays are unlit (tmax -1) depends on the normals
        return {k: g[k] for k in sm.RAY_ARRAYS}

    def model(i):
        out = {}
        for name, mode in (("ao", sm.MODE_AO), ("sun_soft", sm.MODE_SUN)):
            o, counts = sm.run(po, teapot_bvh(po).occluded, i["position"], i["normal"], mode, sc.SEED, SAMPLES, BATCH, eye, **_mode_kw(name))
            out[name + "_out"], out[name + "_counts"] = o, counts
        return out

    return Case(pick(sc.synthetic(W, H)), pick(lc.synthetic(W, H)), model, control)


@functools.lru_cache(maxsize=None)
def lights(po):
    """the "mixed" table on the 24 x 16 teapot frame of lights_cases.E2E, the lights' synthetic planes of that size as poison"""
    e, c = lc.e2e(po, TEAPOT), lc.E2E
    table = lc.TABLES["mixed"]
    kw = dict(bias=c["bias"], margin=c["margin"])
    pick = lambda p: {"position": p["position"], "normal": p["normal"]}  # noqa: E731

    def control(i):
        g = lm.generate(po, i["position"], i["normal"], table, c["light_seed"], SAMPLES, 0, BATCH, e["eye"], **kw)
        return {k: g[k] for k in lm.RAY_ARRAYS}

    def model(i):
        out, sums = lm.run(po, e["bvh"].occluded, i["position"], i["normal"], table, c["light_seed"], SAMPLES, BATCH, e["eye"], **kw)
        return {"out": out, "sums": sums}

    return Case(pick(e["planes"]), pick(lc.synthetic(*c["res"])), model, control, eye=e["eye"], table=table, res=c["res"], seed=c["light_seed"], kw=kw)


# ---- the ray queries --------------------------------------------------------------------------------------------------------------
N_RAYS = W * H * BATCH


def ray_bounds(ts, hit, seed):
    """one bound per ray: around t* for hits, finite values for misses, and the values that are not walked on three rays in ten"""
    rng = np.random.default_rng(seed)
    n = ts.shape[0]
    tsf = np.where(hit, ts, F(1)).astype(F)
    around = [tsf * F(1 - 2 ** -8), tsf, np.nextafter(tsf, F(np.inf)), tsf * F(1 + 2 ** -8), tsf * F(2)]
    tmax = np.where(hit, np.stack(around)[rng.integers(0, len(around), n), np.arange(n)], np.exp(rng.uniform(-3, 9, n))).astype(F)
    special = np.array([0.0, -1.0, np.nan, np.float32(1e-45), np.float32(3e-39), -0.0, -np.inf, np.inf], F)
    pick = rng.random(n) < 0.3
    tmax[pick] = special[rng.integers(0, special.shape[0], int(pick.sum()))]
    return tmax


@functools.lru_cache(maxsize=None)
def queries(po):
    """37 * 23 * 3 rays of the teapot scene of tests/ray_query_scenes.py (random and camera rays) with a bound per ray; the poison is
    the same rays and bounds in reverse order"""
    _, orc, o, d = rq.make("teapot", None, po)
    o, d = np.ascontiguousarray(o[10800:10800 + N_RAYS]), np.ascontiguousarray(d[10800:10800 + N_RAYS])
    ts, prim = orc.trace(o, d)[:2]
    true = {"o": o, "d": d, "tmax": ray_bounds(ts, prim != rq.NO, 5)}
    poison = {k: np.ascontiguousarray(v[::-1]) for k, v in true.items()}

    def control(i):
        return {"occluded": orc.occluded(i["o"], i["d"], i["tmax"]).astype(np.uint8)}

    def model(i):
        return {**orc.trace_bounded(i["o"], i["d"], i["tmax"]), **control(i)}

    # the teapot has no texture coordinates, one material and one instance
    return Case(true, poison, model, control, oracle_scene=orc, constant=("tex", "material", "instance"))


# ---- adaptive sampling: the convergence check on synthetic state planes (the driver's own inputs are renders) ----------------------
CHECK = dict(n=24, ts=16, k=16, threshold=0.1, floor=0.05)


@functools.lru_cache(maxsize=None)
def adaptive_check():
    from tests import adaptive_model as am

    n, ts, k = CHECK["n"], CHECK["ts"], CHECK["k"]
    kinds = [(ts, ts), (1, 1), (ts, 1), (1, ts), (ts // 2 + 1, ts - 1), (ts - 1, ts // 2 + 1), (ts, ts // 2), (2, 3)]
    wh = np.array([kinds[i % len(kinds)] for i in range(n)], np.uint32)

    def inputs(seed):
        """{sum, sum, sum, hits} planes after k samples"""
        rng = np.random.default_rng(seed)
        hits = rng.integers(0, 5, (n, ts, ts)) / 4.0
        mean = rng.random((n, ts, ts))
        spread = rng.random((n, ts, ts)) * rng.choice([0.0, 0.02, 0.3], (n, ts, ts))
        shade, sq = np.zeros((n, ts, ts, 4), F), np.zeros((n, ts, ts, 4), F)
        shade[..., :3] = (mean * hits * k).astype(F)[..., None]
        sq[..., :3] = ((mean * mean + spread) * hits * k).astype(F)[..., None]
        shade[..., 3] = sq[..., 3] = (hits * k).astype(F)
        return {"shade": shade, "shade_sq": sq}

    def control(i):
        opened, err = am.tile_error(i["shade"], i["shade_sq"], wh, k, CHECK["threshold"], CHECK["floor"])
        return {"open": opened, "max_err": err}

    return Case(inputs(21), inputs(22), control, control, wh=wh)
