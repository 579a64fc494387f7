"""The inputs the CPU and the GPU tests of the secondary rays share: seeded synthetic plane sets on which every special value of
include/minipath_secondary.h is planted, and the two end-to-end cases on the teapot.  Everything here is made once and never
changed; the CPU tests show that the inputs reach every rule (tests/test_secondary_cpu.py), the GPU tests compare bits."""
import numpy as np

from tests import secondary_model as sm
from tests import temporal_cases
from tests.secondary_model import F

# one pixel, ragged against the 256-pixel block and the 64-pixel wave (851 pixels), and whole blocks (1024 pixels)
SIZES = [(1, 1), (37, 23), (64, 16)]
BATCHES = [(1, 0), (3, 0), (1, 5), (3, 5)]  # (B, sample_begin) of SAMPLE_COUNT samples
SAMPLE_COUNT = 8
SEED = 0xA0C1
EYE = (0.3, -0.2, 0.1)  # inside the cloud of points, so that normals of every direction are flipped and kept
# name -> the settings of mps_generate beside the sizes.  The hard sun has an axis for a light (so planted normals are exactly
# grazing), no spread and no bound; the soft sun a light in general position with a negative z (the other half of basis()).
MODES = {
    "ao": dict(mode=sm.MODE_AO, radius=0.75, bias=1e-4),
    "sun_hard": dict(mode=sm.MODE_SUN, light=(0.0, 0.0, 1.0), spread=0.0, radius=float("inf"), bias=1e-4),
    "sun_soft": dict(mode=sm.MODE_SUN, light=tuple((np.array([0.3, 0.5, -0.8]) / np.linalg.norm([0.3, 0.5, -0.8])).tolist()), spread=0.05,
                     radius=2.5, bias=0.0),
}
KINDS = 16
MIN_PER_RULE = 16  # pixels over the three sizes that reach each rule (tests/test_secondary_cpu.py)

_synthetic = {}


def synthetic(w, h):
    """{"position", "normal", "kind"} for a size.  Points uniform in [-2, 2]^3 around EYE, unit normals of every direction, both
    planes weighted by an alpha of 1, 0.5 or 0.375 as the renderer's means are.  Planted, cycling over the pixels (kind = index % 16,
    so that the single pixel of 1 x 1 is a plain hit):
      1 a miss (alpha 0, the planes' zeros)   2 a NaN alpha   3 a negative alpha   4 a zero normal   5 a NaN in the normal
      6 the normal (1, 0, +0)   7 (0, 1, -0)   8 (0, 0, 1)   9 (0, 0, -1), with power-of-two alphas so that they stay exact: n.z of the
      turned normal is +0 or -0 and 1 or -1 depending on the side of EYE the point lies on, and with the light (0, 0, 1) kinds 6 and
      7 graze it exactly (dot == +-0), 8 and 9 face it or turn their back to it."""
    key = (w, h)
    if key in _synthetic:
        return _synthetic[key]
    rng = np.random.default_rng(104729 * w + 13 * h)
    kind = (np.arange(h * w).reshape(h, w) % KINDS)
    alpha = rng.choice([1.0, 1.0, 0.5, 0.375], (h, w))
    pts = rng.uniform(-2.0, 2.0, (h, w, 3))
    nrm = rng.normal(0, 1, (h, w, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    planted = {6: (1.0, 0.0, 0.0), 7: (0.0, 1.0, -0.0), 8: (0.0, 0.0, 1.0), 9: (0.0, 0.0, -1.0)}
    for k, v in planted.items():
        nrm[kind == k] = v
        alpha[kind == k] = rng.choice([1.0, 0.5, 0.25], int((kind == k).sum()))
    position = np.concatenate([pts * alpha[..., None], alpha[..., None]], -1).astype(F)
    normal = np.concatenate([nrm * alpha[..., None], (rng.uniform(1.0, 4.0, (h, w)) * alpha)[..., None]], -1).astype(F)
    normal[kind == 7, 2] = F(-0.0)  # (-0.0 * alpha is -0.0 already; said once more)
    position[kind == 1] = 0
    normal[kind == 1] = 0
    position[kind == 2, 3] = np.nan
    position[kind == 3, 3] *= F(-1)
    normal[kind == 4, :3] = 0
    normal[kind == 5, rng.integers(0, 3)] = np.nan
    _synthetic[key] = {"position": position, "normal": normal, "kind": kind}
    return _synthetic[key]


_generated = {}


def generated(po, w, h, mode_name, batch, sample_begin):
    """(the model's ray arrays, info) of a synthetic case: made once"""
    key = (w, h, mode_name, batch, sample_begin)
    if key not in _generated:
        c = synthetic(w, h)
        _generated[key] = sm.generate(po, c["position"], c["normal"], seed=SEED, sample_count=SAMPLE_COUNT, sample_begin=sample_begin,
                                      batch=batch, eye=EYE, want_info=True, **MODES[mode_name])
    return _generated[key]


# ---- resolve: random answers and every tmax code ----------------------------------------------------------------------------------
TMAX_CODES = [0.0, -1.0, -0.0, 0.5, float("inf"), float("nan"), -2.0]
_resolve = {}


def resolve_inputs(w, h, batch):
    """{"tmax", "occluded", "counts"}: tmax codes and occluded bytes (0, 1, and other non-zero values) drawn independently, and a
    counts plane of earlier integer sums whose .z and .w hold NaN (never read)"""
    key = (w, h, batch)
    if key not in _resolve:
        rng = np.random.default_rng(7 * w + 3 * h + batch)
        n = w * h * batch
        counts = np.zeros((h, w, 4), F)
        counts[..., 1] = rng.integers(0, 9, (h, w))
        counts[..., 0] = np.floor(counts[..., 1] * rng.random((h, w)))
        counts[..., 2:] = np.nan
        _resolve[key] = {"tmax": rng.choice(np.array(TMAX_CODES, F), n), "occluded": rng.choice(np.array([0, 0, 1, 1, 255, 2], np.uint8), n),
                         "counts": counts}
    return _resolve[key]


# ---- end to end -------------------------------------------------------------------------------------------------------------------
# One camera for both: above the teapot and a little to the side, looking down, so that the inside of the body shows through the gap
# under the lid and past the spout (shading normals that face away: flipped) beside the lid, the flanks, the handle and the spout.
# The planes are rendered at one sample per pixel, so a pixel's position is a point of the surface itself; the mean of several
# samples lies a little inside a convex surface, which the bias of 1e-4 does not make up for.
# AO: the radius is about the teapot's height: the lid and the rims are free, the joints of the handle and of the spout and the
# body under the rim are partly occluded, the inside is dark.
# SUN: the two teapot instances of tests/temporal_cases.py; the light comes from the left and low: the flanks on the right face away
# (unlit), and the lid's knob, the handle, the spout and the near teapot throw shadows on lit surfaces.
E2E_CAMERA = ((1.0, 9.0, 2.0), (1.0, 1.5, -1.0))
E2E_AO = dict(res=(48, 32), spp=1, tile=16, seed=77, camera=E2E_CAMERA, instances=None,
              samples=8, batch=3, ao_seed=900, radius=3.0, bias=1e-4)
E2E_SUN = dict(res=(48, 32), spp=1, tile=16, seed=78, camera=E2E_CAMERA, instances=temporal_cases.E2E["instances"],
               samples=4, batch=4, sun_seed=901, light=(-0.70, 0.35, 0.62), spreads=(0.0, 0.05), bias=1e-4)
E2E_MIN_PER_CLASS = 32


def e2e_light():
    l = np.array(E2E_SUN["light"], np.float64)
    return tuple((l / np.linalg.norm(l)).astype(F).tolist())


def e2e_camera(mp, case):
    """the case's camera: a pinhole (f_number = inf)"""
    eye, at = case["camera"]
    return mp.Camera.default().look_at(eye, at, (0.0, 1.0, 0.0)).f_number(float("inf"))


def classes(counts, info=None):
    """the pixel classes of a counts plane: boolean maps"""
    V, Cn = counts[..., 0], counts[..., 1]
    out = {"partly": (Cn > 0) & (V > 0) & (V < Cn), "free": (Cn > 0) & (V == Cn), "dark": (Cn > 0) & ((V == 0) | (V <= Cn / 4))}
    if info is not None:
        out["flipped"] = info["flipped"]
        out["unlit"] = info["pixel"] == sm.P_UNLIT
        out["shadowed"] = (info["pixel"] == sm.P_LIVE) & (V < Cn)
    return out


_e2e = {}


def _oracle_frame(po, teapot_obj, case):
    """the oracle's BVH, the planes of the case's frame by the feature-plane model, and the eye"""
    from tests import aov_pass_model

    w, h = case["res"]
    b = po.Bvh.from_obj(teapot_obj)
    if case["instances"] is not None:
        b.set_instances(np.array(case["instances"], F))
    view, smp = temporal_cases.oracle_view(po, temporal_cases.oracle_camera(po, *case["camera"]), case["res"])
    planes = aov_pass_model.planes(po, b.intersect, smp, w, case["spp"], case["seed"], (0, 0, w, h))
    return b, planes, view.center


def e2e_ao(po, teapot_obj):
    """{"planes", "eye", "out", "counts", "info"}: the model's ambient occlusion over the oracle, in batches of 3 + 3 + 2; made once"""
    if "ao" not in _e2e:
        c = E2E_AO
        b, planes, eye = _oracle_frame(po, teapot_obj, c)
        kw = dict(radius=c["radius"], bias=c["bias"])
        out, counts = sm.run(po, b.occluded, planes["position"], planes["normal"], sm.MODE_AO, c["ao_seed"], c["samples"], c["batch"], eye, **kw)
        _, info = sm.generate(po, planes["position"], planes["normal"], sm.MODE_AO, c["ao_seed"], c["samples"], 0, 1, eye, want_info=True, **kw)
        _e2e["ao"] = dict(planes=planes, eye=eye, out=out, counts=counts, info=info, keep=b)
    return _e2e["ao"]


def sun_model(po, occluded_fn, position, normal, eye, spread):
    """the model's sun visibility of the case for given planes: (out, counts, info)"""
    c = E2E_SUN
    kw = dict(light=e2e_light(), spread=spread, radius=float("inf"), bias=c["bias"])
    out, counts = sm.run(po, occluded_fn, position, normal, sm.MODE_SUN, c["sun_seed"], c["samples"], c["batch"], eye, **kw)
    _, info = sm.generate(po, position, normal, sm.MODE_SUN, c["sun_seed"], c["samples"], 0, 1, eye, want_info=True, **kw)
    return out, counts, info


def e2e_sun(po, teapot_obj):
    """{"planes", "eye", "bvh", spread: (out, counts, info)} over the oracle's own planes; made once"""
    if "sun" not in _e2e:
        b, planes, eye = _oracle_frame(po, teapot_obj, E2E_SUN)
        e = dict(planes=planes, eye=eye, bvh=b)
        for spread in E2E_SUN["spreads"]:
            e[spread] = sun_model(po, b.occluded, planes["position"], planes["normal"], eye, spread)
        _e2e["sun"] = e
    return _e2e["sun"]
