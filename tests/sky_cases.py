"""The inputs the CPU and the GPU tests of the sky lighting share: environment maps with a distinct value in every texel, synthetic
ray buffers on which every special direction and every tmax code of include/minipath_sky.h is planted, the end-to-end case on the
teapot and the two cases of the stream test.  Everything here is made once and never changed; the CPU tests show that the inputs
reach every rule (tests/test_sky_cpu.py), the GPU tests compare bits."""
import functools

import numpy as np

from tests import lights_cases, secondary_cases, sky_model as m
from tests.secondary_model import F

# one pixel, ragged against the 256-pixel block and the 64-pixel wave (6 pixels), and whole blocks (1024 pixels)
SIZES = [(1, 1), (3, 2), (64, 16)]
BATCHES = [1, 3, 8]
MAPS = [1, 2, 5, 64]
POLES = [0, 1, 2]
SAMPLE_COUNT = 8
TMAX_CODES = secondary_cases.TMAX_CODES  # 0, -1, -0, 0.5, +inf, NaN, -2
MIN_PER_RULE = 16  # rays of the largest synthetic case that reach each rule, looked up (tests/test_sky_cpu.py)
NAN, INF = float("nan"), float("inf")


@functools.lru_cache(maxsize=None)
def texel_map(n, seed=0):
    """[n, n, 4]: random colours in [0.5, 4), a different one in every texel and channel, and a NaN in every .w (it is never read)"""
    rng = np.random.default_rng(7919 * n + seed)
    values = np.unique(rng.uniform(0.5, 4.0, 4 * 3 * n * n).astype(F))  # distinct as float32
    env = np.full((n, n, 4), np.nan, F)
    env[..., :3] = rng.permutation(values)[:3 * n * n].reshape(n, n, 3)
    return env


def index_map(n):
    """[n, n, 4]: the texel T[y][x] holds {x, y, y * n + x, NaN}"""
    y, x = np.mgrid[0:n, 0:n]
    return np.stack([x, y, y * n + x, np.full((n, n), np.nan)], -1).astype(F)


@functools.lru_cache(maxsize=None)
def planted(n):
    """[(kind, m)]: the directions planted for a map of n texels, in the map's frame"""
    rng = np.random.default_rng(31 * n + 1)
    out = []
    add = lambda kind, rows: out.extend((kind, tuple(float(v) for v in r)) for r in np.asarray(rows, F).reshape(-1, 3))  # noqa: E731
    add("axis", [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])
    add("diagonal", [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)])
    add("horizon +0", [(0.3, -0.7, 0.0), (-1.0, 0.0, 0.0), (0.0, 2.0, 0.0), (-0.25, 0.25, 0.0)])
    add("horizon -0", [(0.3, -0.7, -0.0), (-1.0, 0.0, -0.0), (0.0, 2.0, -0.0), (-0.25, 0.25, -0.0)])
    centres, _ = m.texel_directions(n)
    centres = centres.reshape(-1, 3)
    add("texel centre", centres[rng.permutation(max(len(centres), 48))[:48] % len(centres)])  # 48 of them; every one of a small map
    # texel edges: points of the grid lines px = 2 i / n - 1, lifted to the upper and to the lower half of the octahedron
    line = (np.arange(n + 1, dtype=F) * F(2) / F(n) - F(1)).astype(F)
    px, py = rng.choice(line, 48), rng.uniform(-1, 1, 48).astype(F)
    swap = rng.random(48) < 0.5
    px, py = np.where(swap, py, px), np.where(swap, px, py)
    z = ((F(1) - np.abs(px)) - np.abs(py)).astype(F)
    qx, qy = m.fold(px, py)
    add("texel edge", np.stack([np.where(z < 0, qx, px), np.where(z < 0, qy, py), z], -1))
    # the fold's border (one of px, py is 0 below the horizon: the other folds onto +-1) and its corners (both are 0, of either sign)
    add("border", [(0.5, 0.0, -0.5), (-0.25, 0.0, -0.75), (0.0, 0.75, -0.25), (-0.0, -0.5, -0.5), (0.125, -0.0, -2.0)])
    add("corner", [(0.0, 0.0, -1.0), (-0.0, 0.0, -1.0), (0.0, -0.0, -3.0), (-0.0, -0.0, -0.5)])
    general = rng.normal(0, 1, (6, 3)).astype(F)
    add("subnormal", general * F(2.0 ** -140))
    add("scaled 2^100", general * F(2.0 ** 100))
    add("l1 overflows", [(3e38, 3e38, 1e38), (-3e38, 2e38, -3e38), (2e38, -2e38, 0.0), (-1e38, -1e38, 3e38)])
    add("zero", [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (0.0, -0.0, 0.0), (-0.0, -0.0, -0.0)])
    add("nan", [(NAN, 0.5, 0.5), (0.5, NAN, -0.5), (0.5, 0.5, NAN)])
    add("inf", [(INF, 0.5, 0.5), (0.5, -INF, -0.5), (0.5, 0.5, -INF), (INF, INF, INF)])
    return out


KINDS = ("axis", "diagonal", "horizon +0", "horizon -0", "texel centre", "texel edge", "border", "corner", "subnormal", "scaled 2^100",
         "l1 overflows", "zero", "nan", "inf", "random")


@functools.lru_cache(maxsize=None)
def resolve_inputs(w, h, batch, n):
    """{"m" [rays, 3], "kind" [rays], "tmax", "occluded", "sums"} for an image, a batch and a map size: the planted directions of the
    map on every even ray in turn and normally distributed ones on the odd rays, in the MAP's frame (a test turns them into the
    directions of a pole with sky_model.from_map, so every pole sees every planted direction); tmax codes and occluded bytes (0, 1,
    and other non-zero values) drawn independently, about two rays in three traced; and a sums plane of earlier sums with integer counts,
    a -0 among them"""
    rng = np.random.default_rng(1009 * w + 13 * h + 7 * batch + n)
    rays = w * h * batch
    plant = planted(n)
    mm = rng.normal(0, 1, (rays, 3)).astype(F)
    kind = np.full(rays, KINDS.index("random"))
    start = int(rng.integers(0, len(plant)))
    for k in range(0, rays, 2):
        name, v = plant[(start + k // 2) % len(plant)]
        mm[k], kind[k] = v, KINDS.index(name)
    codes = np.array(TMAX_CODES, F)
    tmax = np.where(rng.random(rays) < 0.5, rng.choice(codes, rays), rng.choice(np.array([0.5, INF, 3.0], F), rays)).astype(F)
    sums = np.concatenate([rng.uniform(0.0, 50.0, (h, w, 3)), rng.integers(0, 9, (h, w, 1))], -1).astype(F)
    sums[rng.random((h, w)) < 0.1, 1] = F(-0.0)
    return {"m": mm, "kind": kind, "tmax": tmax, "occluded": rng.choice(np.array([0, 0, 0, 1, 255, 2], np.uint8), rays), "sums": sums}


# ---- end to end -------------------------------------------------------------------------------------------------------------------
# The teapot at 24 x 16 from the camera of the secondary rays' and the lights' cases: above the teapot and a little to the side,
# looking down, the planes rendered at one sample per pixel.  The scene is y-up, so pole = 1.  The lid and the top of the body see
# the whole sky (every sample open), the flanks, the spout and the handle send part of their rays into the body or under it
# (mixed; a ray that leaves a flank downwards escapes, there is no floor: the lower, folded half of the map), and the background is
# never counted.  Counted with the oracle by tests/test_sky_cpu.py.
E2E = dict(res=(24, 16), spp=1, tile=8, seed=81, camera=secondary_cases.E2E_CAMERA, instances=None, samples=8, batch=3, sky_seed=2300, pole=1, radius=float("inf"), bias=1e-4, map_size=16,
           zenith=(0.125, 0.375, 1.0), horizon=(1.5, 0.875, 0.625), ground=(0.0625, 0.25, 0.03125))
E2E_MIN_PER_CLASS = 5
E2E_CLASSES = ("none", "open", "mixed")
E2E_MIN_RAYS_PER_HALF = 20


def e2e_map():
    return m.fill_gradient(E2E["map_size"], E2E["zenith"], E2E["horizon"], E2E["ground"])


def classes(sums, rays):
    """the pixel classes of a result, boolean maps, from the sums plane and the [samples, H, W] tmax and occluded of its rays: no
    counted sample; every sample open (counted, and every ray traced and unoccluded); mixed (some rays open, some occluded)"""
    traced = rays["tmax"] > 0
    opened = traced & (rays["occluded"] == 0)
    n_open, n = opened.sum(0), traced.shape[0]
    counted = sums[..., 3] > 0
    return {"none": ~counted, "open": counted & (n_open == n), "mixed": counted & (n_open > 0) & (n_open < traced.sum(0))}


def open_rays_per_half(rays, pole):
    """(upper, folded): the open rays whose direction has m.z >= 0 and m.z < 0"""
    opened = (rays["tmax"] > 0) & (rays["occluded"] == 0)
    mz = m.to_map(rays["d"], pole)[..., 2]
    return int((opened & ~(mz < 0)).sum()), int((opened & (mz < 0)).sum())


_e2e = {}


def e2e(po, teapot_obj):
    """{"planes", "eye", "bvh", "env", "out", "sums", "ao", "counts", "rays"}: the model's sky light and visibility over the oracle, in
    batches of 3 + 3 + 2; made once"""
    if "e2e" not in _e2e:
        c = E2E
        b, planes, eye = secondary_cases._oracle_frame(po, teapot_obj, c)
        env = e2e_map()
        out, sums, ao, counts, rays = m.run(po, b.occluded, planes["position"], planes["normal"], env, c["sky_seed"], c["samples"], c["batch"],
                                            eye, pole=c["pole"], radius=c["radius"], bias=c["bias"], visibility=True, want_rays=True)
        _e2e["e2e"] = dict(planes=planes, eye=eye, bvh=b, env=env, out=out, sums=sums, ao=ao, counts=counts, rays=rays)
    return _e2e["e2e"]


# ---- the stream test (the method and the Case of tests/stream_cases.py) ------------------------------------------------------------
STREAM_BATCH = 3


@functools.lru_cache(maxsize=None)
def stream_stage(po, teapot_obj):
    """SkyLight on the end-to-end frame and its map; the poison is the lights' synthetic planes of that size and a map of random
    texels of the same size"""
    from tests import stream_cases

    e, c = e2e(po, teapot_obj), E2E
    pick = lambda p, env: {"position": p["position"], "normal": p["normal"], "env": env}  # noqa: E731
    poison_env = np.array(texel_map(c["map_size"], seed=5))
    poison_env[..., 3] = 1  # (a NaN would only be compared as itself; nothing reads it)

    def model(i):
        out, sums = m.run(po, e["bvh"].occluded, i["position"], i["normal"], i["env"], c["sky_seed"], c["samples"], STREAM_BATCH, e["eye"],
                          pole=c["pole"], radius=c["radius"], bias=c["bias"])
        return {"out": out, "sums": sums}

    return stream_cases.Case(pick(e["planes"], e["env"]), pick(lights_cases.synthetic(*c["res"]), poison_env), model, model, eye=e["eye"],
                             res=c["res"])


CONTROL = dict(w=37, h=23, batch=3, n=5, pole=2)


@functools.lru_cache(maxsize=None)
def stream_control():
    """one mpe_resolve on synthetic ray buffers; the poison is the buffers of another seed (another image width) and another map"""
    from tests import stream_cases

    c = CONTROL

    def inputs(r, env):
        d = m.from_map(r["m"], c["pole"])
        env = np.array(env)
        env[..., 3] = 1
        return {"env": env, "dx": np.ascontiguousarray(d[:, 0]), "dy": np.ascontiguousarray(d[:, 1]), "dz": np.ascontiguousarray(d[:, 2]),
                "tmax": r["tmax"], "occluded": r["occluded"]}

    def control(i):
        sums, out = m.resolve(i["env"], i["dx"], i["dy"], i["dz"], i["tmax"], i["occluded"], (c["h"], c["w"]), c["batch"], c["pole"])
        return {"sums": sums, "out": out}

    true = inputs(resolve_inputs(c["w"], c["h"], c["batch"], c["n"]), texel_map(c["n"]))
    poison = inputs(resolve_inputs(c["h"], c["w"], c["batch"], c["n"]), texel_map(c["n"], seed=9))
    return stream_cases.Case(true, poison, control, control)
