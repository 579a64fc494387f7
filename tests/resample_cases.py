"""The inputs the CPU and the GPU tests of the guided resampling share: seeded synthetic plane sets on which every special value of
include/minipath_resample.h is planted, and the end-to-end case on the teapot.  Everything here is made once and never changed; the
CPU tests show that the inputs reach every rule (tests/test_resample_cpu.py), the GPU tests compare bits."""
import numpy as np

from tests import resample_model as rm
from tests import secondary_cases
from tests import secondary_model as sm
from tests.resample_model import F

# one pixel, a single row, ragged against f = 2, 3, 4 and the 16 x 16 tile at once (3 x 2 tiles), and whole tiles
SIZES = [(1, 1), (5, 1), (37, 23), (64, 16)]
FACTORS = [2, 3, 4]
MIN_PER_RULE = 16
KINDS = 16
# per factor: the weights of the synthetic upsample cases -- k = 0 and no plane weight, both in the middle, k = 8 and a tight plane
UP_WEIGHTS = {2: (0, float("inf")), 3: (3, 0.05), 4: (8, 0.004)}


def phases(f):
    """the first, one in between and the last"""
    return [0, f * f // 2, f * f - 1]


def down_cases():
    """(size, f, pick_mode, phase) of every synthetic downsample case"""
    return [(s, f, rm.PICK_PHASE, ph) for s in SIZES for f in FACTORS for ph in phases(f)] + \
           [(s, f, rm.PICK_NEAREST, 0) for s in SIZES for f in FACTORS]


_synthetic = {}


def synthetic(W, H):
    """{"position", "normal", "ids", "kind"} for a size.  A smooth surface seen from (0, 0, 6): two sheets, the right one (x >= 0.6 W)
    1.5 further away, so that picks across the step lie far off the tangent plane; analytic normals times a random length, both
    planes weighted by an alpha of 1, 0.5 or 0.375 as the renderer's means are; t = the distance from the eye.  Planted, cycling
    over the pixels (kind = index % 16, so that the single pixel of 1 x 1 is a plain hit):
      1 a miss (the planes' zeros)   2 a NaN alpha   3 a negative alpha   4 a zero normal   5 a NaN in the normal
      6 the normal turned round (every tap of another pick has wn == 0: the nearest-tap fallback)
    and by place, on sizes that hold them:
      a rectangle of misses x in [8, 20), y in [4, 12): whole blocks without a valid pixel for every f
      equal depths (t = 2 exactly) on x in [24, 37), y in [12, 16): NEAREST's first-wins
      a NaN depth (normal.w) at every (12 i, 12 j) with a plain hit: the first pixel of its block for every f
    "ids" is an int32 plane of words no float compare would keep apart (negative, NaN patterns)."""
    key = (W, H)
    if key in _synthetic:
        return _synthetic[key]
    rng = np.random.default_rng(7919 * W + 31 * H)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    kind = (np.arange(H * W).reshape(H, W) % KINDS)
    if W >= 12:
        kind[::12, ::12] = 0
    z = 0.3 * np.sin(0.35 * xs) + 0.2 * np.cos(0.5 * ys) - 1.5 * (xs >= 0.6 * W)
    pts = np.stack([0.1 * xs - 0.05 * W, 0.1 * ys - 0.05 * H, z], -1)
    nrm = np.stack([-0.3 * 0.35 * np.cos(0.35 * xs) / 0.1, 0.2 * 0.5 * np.sin(0.5 * ys) / 0.1, np.ones_like(xs)], -1)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    nrm[kind == 6] *= -1
    nrm *= rng.uniform(0.5, 2.0, (H, W))[..., None]
    alpha = rng.choice([1.0, 1.0, 0.5, 0.375], (H, W))
    t = np.linalg.norm(pts - np.array([0.0, 0.0, 6.0]), axis=-1)
    t[12:16, 24:37] = 2.0
    position = np.concatenate([pts * alpha[..., None], alpha[..., None]], -1).astype(F)
    normal = np.concatenate([nrm * alpha[..., None], (t * alpha)[..., None]], -1).astype(F)
    if W >= 12:
        normal[::12, ::12, 3] = np.nan
    position[kind == 1] = 0
    normal[kind == 1] = 0
    position[kind == 2, 3] = np.nan
    position[kind == 3, 3] *= F(-1)
    normal[kind == 4, :3] = 0
    normal[kind == 5, rng.integers(0, 3)] = np.nan
    position[4:12, 8:20] = 0
    normal[4:12, 8:20] = 0
    ids = rng.integers(-2 ** 31, 2 ** 31, (H, W, 4), dtype=np.int64).astype(np.int32)
    ids[..., 3] = np.where(position[..., 3] > 0, 1, 0)
    ids[::3, ::2, 2] = 0x7FC00001  # a NaN pattern with a payload
    _synthetic[key] = {"position": position, "normal": normal, "ids": ids, "kind": kind}
    return _synthetic[key]


_down = {}


def downsampled(W, H, f, pick_mode, phase):
    """the model's (picks, [position_lo, normal_lo, ids_lo], info) of a synthetic case: made once"""
    key = (W, H, f, pick_mode, phase)
    if key not in _down:
        c = synthetic(W, H)
        _down[key] = rm.downsample(c["position"], c["normal"], [c["position"], c["normal"], c["ids"]], f, pick_mode, phase, want_info=True)
    return _down[key]


_up = {}


def upsample_inputs(W, H, f):
    """{"position_lo", "normal_lo", "picks", "color_lo", "k", "sigma_plane", "out", "info"}: the low planes of the PHASE case in
    between, as caller data -- with, cycling over the low pixels, a colour alpha of 0 (index % 7 == 3), a pick >= W * H
    (index % 11 == 5), a NaN in position_lo (index % 13 == 7) --, a rectangle of colour alphas 0 on X in [1, 6), Y in [0, 4), whose
    inner pixels have no usable tap (holes), random colours, and the model's result with the factor's weights; made once"""
    key = (W, H, f)
    if key not in _up:
        picks, (position_lo, normal_lo, _), _ = downsampled(W, H, f, rm.PICK_PHASE, phases(f)[1])
        h, w = picks.shape
        rng = np.random.default_rng(17 * W + 5 * H + f)
        index = np.arange(h * w).reshape(h, w)
        color_lo = np.concatenate([rng.uniform(0.0, 1.0, (h, w, 3)), np.ones((h, w, 1))], -1).astype(F)
        picks, position_lo = picks.copy(), position_lo.copy()
        if w * h > 1:
            color_lo[index % 7 == 3, 3] = 0
            picks[index % 11 == 5] = (W * H + rng.integers(0, 1000, int((index % 11 == 5).sum()))).astype(np.uint32)
            position_lo[index % 13 == 7, 1] = np.nan
            color_lo[0:4, 1:6, 3] = 0
        c = synthetic(W, H)
        k, sigma_plane = UP_WEIGHTS[f]
        out, info = rm.upsample(c["position"], c["normal"], position_lo, normal_lo, picks, color_lo, f, k, sigma_plane, want_info=True)
        _up[key] = dict(position_lo=position_lo, normal_lo=normal_lo, picks=picks, color_lo=color_lo, k=k, sigma_plane=sigma_plane,
                        out=out, info=info)
    return _up[key]


# ---- end to end -------------------------------------------------------------------------------------------------------------------
# The teapot at 48 x 32 and one sample per pixel with the camera and the ambient-occlusion settings of secondary_cases.E2E_AO, traced
# at 24 x 16 (f = 2) and brought back.  The second phase of the GPU test picks other pixels.
E2E = dict(secondary_cases.E2E_AO, factor=2, phase=0, second_phase=3, reference_samples=64, reference_seed=901)
E2E_MIN_PER_CLASS = 32
_e2e = {}


def e2e_frame(po, teapot_obj):
    """{"planes", "eye", "bvh"}: the oracle's frame of secondary_cases.E2E_AO; made once"""
    if "frame" not in _e2e:
        b, planes, eye = secondary_cases._oracle_frame(po, teapot_obj, E2E)
        _e2e["frame"] = dict(planes=planes, eye=eye, bvh=b)
    return _e2e["frame"]


def e2e_low(po, teapot_obj, phase, pick_mode=rm.PICK_PHASE):
    """{"picks", "position_lo", "normal_lo", "ids_lo", "ao_lo", "counts_lo"}: the model's downsample of the frame and the secondary
    model's 8-sample ambient occlusion over the oracle at the low resolution; made once per phase"""
    key = ("low", phase, pick_mode)
    if key not in _e2e:
        c, fr = E2E, e2e_frame(po, teapot_obj)
        p = fr["planes"]
        picks, (position_lo, normal_lo, ids_lo) = rm.downsample(p["position"], p["normal"], [p["position"], p["normal"], p["ids"]], c["factor"],
                                                                pick_mode, phase)
        ao_lo, counts_lo = sm.run(po, fr["bvh"].occluded, position_lo, normal_lo, sm.MODE_AO, c["ao_seed"], c["samples"], c["batch"], fr["eye"],
                                  radius=c["radius"], bias=c["bias"])
        _e2e[key] = dict(picks=picks, position_lo=position_lo, normal_lo=normal_lo, ids_lo=ids_lo, ao_lo=ao_lo, counts_lo=counts_lo)
    return _e2e[key]


def e2e_up(po, teapot_obj, phase, k, sigma_plane):
    """(out, info): the model's upsample of e2e_low(phase) with the given weights; made once per argument set"""
    key = ("up", phase, float(k), float(sigma_plane))
    if key not in _e2e:
        fr, lo = e2e_frame(po, teapot_obj), e2e_low(po, teapot_obj, phase)
        _e2e[key] = rm.upsample(fr["planes"]["position"], fr["planes"]["normal"], lo["position_lo"], lo["normal_lo"], lo["picks"], lo["ao_lo"],
                                E2E["factor"], k, sigma_plane, want_info=True)
    return _e2e[key]


def e2e_reference(po, teapot_obj):
    """the oracle's 64-sample ambient occlusion at full resolution (another seed): what the resampled 8 samples approximate"""
    if "ref" not in _e2e:
        c, fr = E2E, e2e_frame(po, teapot_obj)
        out, _ = sm.run(po, fr["bvh"].occluded, fr["planes"]["position"], fr["planes"]["normal"], sm.MODE_AO, c["reference_seed"],
                        c["reference_samples"], 16, fr["eye"], radius=c["radius"], bias=c["bias"])
        _e2e["ref"] = out
    return _e2e["ref"]
