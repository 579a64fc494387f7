"""The inputs the CPU and the GPU tests of the lights share: seeded synthetic plane sets on which every special value of
include/minipath_lights.h is planted, three light tables, and the end-to-end case on the teapot.  Everything here is made once and
never changed; the CPU tests show that the inputs reach every rule (tests/test_lights_cpu.py), the GPU tests compare bits."""
import numpy as np

from tests import lights_model as lm
from tests import secondary_cases
from tests.secondary_model import F

# one pixel, ragged against the 256-pixel block and the 64-pixel wave (851 pixels), and whole blocks (1024 pixels)
SIZES = [(1, 1), (37, 23), (64, 16)]
BATCHES = [(1, 0), (3, 0), (1, 5), (3, 5)]  # (B, sample_begin) of SAMPLE_COUNT samples
SAMPLE_COUNT = 8
SEED = 0xB1C2
EYE = (0.3, -0.2, 0.1)  # inside the cloud of points, so that normals of every direction are flipped and kept
BIAS = 2.0 ** -13       # a power of two: the planted origins P + n * bias are exact
MARGIN = 0.25
# The first light's x is a subnormal: a surface whose origin has x == 0 and whose normal is the x axis sees it at a cosine that is a
# subnormal (the grazing rule).  All three coordinates are dyadic (2^-130 keeps two bits to spare below it, for the alphas), so that
# a planted origin can equal the light in every bit.
C0 = (2.0 ** -130, -0.25, 0.75)
C1 = (-0.75, 0.5, -0.5)
R1 = 0.3
# name -> light table.  "mixed": the middle light is the only sphere, so a stream's first draw belongs to the second light (the
# draw-skipping rule); "spheres": eight spheres, the first two at the centres of the first two lights of the other tables.
TABLES = {
    "point": [(C0, 0.0, (3.0, 2.0, 1.0))],
    "mixed": [(C0, 0.0, (3.0, 2.0, 1.0)), (C1, R1, (0.5, 0.0, 4.0)), ((1.5, -1.0, 1.25), 0.0, (0.25, 8.0, 0.125))],
    "spheres": [(C0, 0.05, (3.0, 2.0, 1.0)), (C1, R1, (0.5, 0.0, 4.0)), ((1.5, -1.0, 1.25), 0.125, (0.25, 8.0, 0.125)),
                ((0.0, 0.0, -3.0), 0.5, (1.0, 1.0, 1.0)), ((0.0, 2.5, 0.0), 1.0, (0.0, 0.0, 0.0)), ((-2.5, -2.5, 2.5), 0.01, (9.0, 0.5, 0.25)),
                ((0.25, 0.25, 0.25), 0.2, (0.125, 0.25, 0.5)), ((3.0, 0.0, 0.0), 2.0, (2.0, 3.0, 5.0))],
}
KINDS = 16
MIN_PER_RULE = 16  # pixels over the three sizes that reach each rule (tests/test_lights_cpu.py)

_synthetic = {}


def synthetic(w, h):
    """{"position", "normal", "kind"} for a size.  Points uniform in [-2, 2]^3 around EYE, unit normals of every direction, both
    planes weighted by an alpha of 1, 0.5 or 0.375 as the renderer's means are.  Planted, cycling over the pixels (kind = index % 16,
    so that the single pixel of 1 x 1 is a plain hit):
      1 a miss (alpha 0, the planes' zeros)   2 a NaN alpha   3 a negative alpha   4 a zero normal   5 a NaN in the normal
      6 at the light: the normal is the z axis and P = C0 -+ z * BIAS, so that the origin is C0 in every bit (dd == 0)
      7 inside the sphere light at C1: P within R1 / 2 of its centre
      8 within the margin: P is 0.1 beyond C0 as seen from EYE, the normal along that line, so that the surface faces the light at
        a distance below MARGIN
      9 grazing: the normal is the x axis and P.x = -BIAS, so that the origin's x is 0 and n.d = C0.x, a subnormal
    6 and 9 have power-of-two alphas so that the planted values stay exact."""
    key = (w, h)
    if key in _synthetic:
        return _synthetic[key]
    rng = np.random.default_rng(15485863 * w + 17 * h)
    kind = (np.arange(h * w).reshape(h, w) % KINDS)
    alpha = rng.choice([1.0, 1.0, 0.5, 0.375], (h, w))
    pts = rng.uniform(-2.0, 2.0, (h, w, 3))
    nrm = rng.normal(0, 1, (h, w, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    c0, c1, eye = np.array(C0, np.float64), np.array(C1, np.float64), np.array(EYE, np.float64)
    for k in (6, 9):
        alpha[kind == k] = rng.choice([1.0, 0.5, 0.25], int((kind == k).sum()))
    # 6: C0.z > EYE.z, so the z axis is turned to -z and the origin is P - z * BIAS
    pts[kind == 6] = c0 + np.array([0.0, 0.0, BIAS])
    nrm[kind == 6] = (0.0, 0.0, 1.0)
    off = rng.normal(0, 1, (h, w, 3))
    off *= (rng.uniform(0.0, R1 / 2, (h, w)) / np.linalg.norm(off, axis=-1))[..., None]
    pts[kind == 7] = (c1 + off)[kind == 7]
    away = (c0 - eye) / np.linalg.norm(c0 - eye)
    pts[kind == 8] = c0 + 0.1 * away
    nrm[kind == 8] = away
    # 9: P.x < EYE.x, so the x axis is kept and the origin's x is -BIAS + BIAS
    pts[kind == 9, 0] = -BIAS
    nrm[kind == 9] = (1.0, 0.0, 0.0)
    position = np.concatenate([pts * alpha[..., None], alpha[..., None]], -1).astype(F)
    normal = np.concatenate([nrm * alpha[..., None], (rng.uniform(1.0, 4.0, (h, w)) * alpha)[..., None]], -1).astype(F)
    position[kind == 1] = 0
    normal[kind == 1] = 0
    position[kind == 2, 3] = np.nan
    position[kind == 3, 3] *= F(-1)
    normal[kind == 4, :3] = 0
    normal[kind == 5, rng.integers(0, 3)] = np.nan
    _synthetic[key] = {"position": position, "normal": normal, "kind": kind}
    return _synthetic[key]


_generated = {}


def generated(po, w, h, table_name, batch, sample_begin):
    """(the model's ray arrays, info) of a synthetic case: made once"""
    key = (w, h, table_name, batch, sample_begin)
    if key not in _generated:
        c = synthetic(w, h)
        _generated[key] = lm.generate(po, c["position"], c["normal"], TABLES[table_name], seed=SEED, sample_count=SAMPLE_COUNT,
                                      sample_begin=sample_begin, batch=batch, eye=EYE, bias=BIAS, margin=MARGIN, want_info=True)
    return _generated[key]


# ---- resolve: random answers and every tmax code ----------------------------------------------------------------------------------
TMAX_CODES = secondary_cases.TMAX_CODES
RESOLVE_SHAPES = [(1, "point"), (3, "mixed")]  # (B, table)
_resolve = {}


def resolve_inputs(w, h, batch, table_name):
    """{"tmax", "weight", "occluded", "sums"}: tmax codes, finite weights (zeros and a subnormal among them) and occluded bytes (0, 1,
    and other non-zero values) drawn independently, and a sums plane of earlier sums with integer counts"""
    key = (w, h, batch, table_name)
    if key not in _resolve:
        rng = np.random.default_rng(11 * w + 5 * h + batch + 100 * len(TABLES[table_name]))
        n = w * h * batch * len(TABLES[table_name])
        sums = np.concatenate([rng.uniform(0.0, 50.0, (h, w, 3)), rng.integers(0, 9, (h, w, 1))], -1).astype(F)
        weight = rng.uniform(0.0, 4.0, n).astype(F)
        weight[rng.random(n) < 0.1] = 0
        weight[rng.random(n) < 0.05] = F(1e-39)
        _resolve[key] = {"tmax": rng.choice(np.array(TMAX_CODES, F), n), "weight": weight,
                         "occluded": rng.choice(np.array([0, 0, 1, 1, 255, 2], np.uint8), n), "sums": sums}
    return _resolve[key]


# ---- end to end -------------------------------------------------------------------------------------------------------------------
# The teapot at 24 x 16 from the camera of the secondary rays' cases, the planes rendered at one sample per pixel (a pixel's position
# is then a point of the surface itself: DESIGN.md 4.11, "a limit worth knowing").  Both lights stand on the handle's side, in front:
# a point light low down, so that the lid and the flank towards the spout face away from it and the handle and the rim throw hard
# shadows, and a sphere light of radius 1 a little higher, whose disc the handle, the knob and the rim cut (penumbrae).  Found with
# the oracle among 64 placements: 62 pixels fully visible, 33 fully shadowed, 35 partly, 46 facing away from both, 206 misses.
E2E = dict(res=(24, 16), spp=1, tile=8, seed=81, camera=secondary_cases.E2E_CAMERA, instances=None, samples=8, batch=3, light_seed=1900,
           bias=1e-4, margin=0.05,
           lights=[((-6.0, 1.0, 3.0), 0.0, (30.0, 28.0, 24.0)), ((-4.0, 3.0, 2.0), 1.0, (4.0, 6.0, 10.0))])
E2E_MIN_PER_CLASS = 8
E2E_CLASSES = ("miss", "visible", "shadowed", "partly", "away")


def classes(sums, rays):
    """the pixel classes of a result, boolean maps, from the sums plane and the [samples, L, H, W] tmax and occluded of its rays:
    miss (nothing counted); lit and fully visible (some ray traced, none of them occluded); lit and fully shadowed (some ray traced,
    all of them occluded); partly shadowed by the sphere light (light 1: of its traced rays some occluded, some not); facing away
    from both lights (counted, and no ray traced)"""
    traced = rays["tmax"] > 0
    hidden = traced & (rays["occluded"] != 0)
    nt, nh = traced.sum((0, 1)), hidden.sum((0, 1))
    nt1, nh1 = traced[:, 1].sum(0), hidden[:, 1].sum(0)
    counted = sums[..., 3] > 0
    return {"miss": ~counted, "visible": counted & (nt > 0) & (nh == 0), "shadowed": counted & (nt > 0) & (nh == nt),
            "partly": counted & (nh1 > 0) & (nh1 < nt1), "away": counted & (nt == 0)}


_e2e = {}


def e2e(po, teapot_obj):
    """{"planes", "eye", "bvh", "out", "sums", "rays"}: the model's irradiance over the oracle, in batches of 3 + 3 + 2; made once"""
    if "e2e" not in _e2e:
        c = E2E
        b, planes, eye = secondary_cases._oracle_frame(po, teapot_obj, c)
        out, sums, rays = lm.run(po, b.occluded, planes["position"], planes["normal"], c["lights"], c["light_seed"], c["samples"], c["batch"],
                                 eye, want_rays=True, bias=c["bias"], margin=c["margin"])
        _e2e["e2e"] = dict(planes=planes, eye=eye, bvh=b, out=out, sums=sums, rays=rays)
    return _e2e["e2e"]
