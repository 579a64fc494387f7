"""GPU tests (-m gpu) of what the cached packet kernels do once per work unit instead of once per pass (kernels_tiles.hip, kernels_aov.hip): the sample key
from the lane's key at sample 0, the scene pre-test decided per unit (mask_cache.h, mask_cache_unit_reaches), and the shading normal's
short normalisation (ray_math.h, unit_normal).  Frames against the oracle's bits, with the kernels named, at 96 x 64 in tiles of 32:
64 samples on render_tiles_packet_kernel<16, ..., true> (four passes per unit, sixteen samples in flight) and 32 samples on
render_aov_packet_kernel<4, ..., true>:

  teapot   units that miss the scene, units on the silhouette and units inside it
  atrium   the stand-in scene at a small detail: an interior view, every ray reaches the scene's box; walls along the axes
  away     the teapot's camera turned round: every unit misses, and every unit keeps the per-ray pre-test, which skips the walk
  wide     the atrium through a lens 2.5 m across: corner rays of mixed sign patterns decline to set bounds in many units, which then
           take their bounds from the first pass and keep the per-ray test
  sphere, group   a Sphere scene and an object group, on kernels this change leaves as they were

The teapot, away and wide frames once more in the counted build libminipath_hip_noskip.so (-DMP_PROF_MISSES; the build's own switch,
-DMP_NO_EMPTY_SKIP, concerns the walk, not the pass entry), in a process of its own (tests/walk_frames.py, run_in_variant): `units_skip_pretest`
and `units_keep_pretest` are the units whose passes skip the per-ray pre-test and the units that keep it.  The teapot's frame and the wide
lens's must show both, the frame that looks away only the second."""
import functools

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib
from tests import aov_model
from tests import walk_frames as wf
from tests.conftest import TEAPOT
from tests.walk_frames import Counters, assert_same_bits, differing, frame, planes, run_in_variant

pytestmark = pytest.mark.gpu

RES, TS, SPP, AOV_SPP = (96, 64), 32, 64, 32
SEED = 33
WHICH = ("shade", "normal", "ids")
PACKET = "render_tiles_packet_kernel<16, false, 8, false, true>"
AOV = "render_aov_packet_kernel<4, false, 8, false, true>"
BALL = ((0.4, 0.0, 0.0), 1.0)
GROUP_AT = [[0.0, 0.0, 0.0], [0.0, 3.5, -1.0]]
CACHED = ("teapot", "atrium", "away", "wide")


def cameras():
    return {**wf.cameras(),
            "sphere": mp.Camera.default().look_at((0.4, 5.0, 4.5), (0.0, 0.0, 0.0), (0, 1, 0)),
            "group": mp.Camera.default().look_at((1.0, 5.0, 12.0), (0.0, 2.0, 0.0), (0, 1, 0))}


def counted_frames():
    """{name: f32 frame, name + "_units": (units that skip the per-ray pre-test, units that keep it)} in the library that is loaded"""
    prof = Counters(_lib.lib())
    ctx = mp.Context(0)
    cams, out = cameras(), {}
    objs = wf.make_objects(ctx, ("teapot", "away", "wide"))
    for name in ("teapot", "away", "wide"):
        prof.reset()
        f, _, names, _ = frame(ctx, objs[name], cams[name], mp.RenderSettings(TS, SPP, RES, seed=SEED))
        assert names == [PACKET], names
        c = prof.read()
        out[name], out[name + "_units"] = f, np.array([c["units_skip_pretest"], c["units_keep_pretest"]], np.uint64)
    return out


@functools.lru_cache(maxsize=None)
def oracle_scene(oracle, name):
    """the oracle's twin of a scene: a Bvh, or the sphere as (center, radius)"""
    if name in CACHED:
        return wf.oracle_scene(oracle, name)
    if name == "sphere":
        return BALL
    box = oracle.Bvh.from_obj(TEAPOT)
    box.set_group([oracle.Bvh.from_obj(TEAPOT), BALL], np.array(GROUP_AT, np.float32))
    return box


@functools.lru_cache(maxsize=None)
def wanted(oracle, name):
    """the oracle's frame of a case, once: (f32, u8)"""
    if name in CACHED:
        return wf.oracle_frame(oracle, name, RES, SPP, SEED, TS)
    if name == "sphere":
        smp = oracle.sampler_from_array(cameras()[name].build_sampler(RES).as_array())
        return oracle.render_tile_sphere(*BALL, smp, RES[0], SPP, SEED, 0, 0, *RES)
    return wf.oracle_image(oracle, oracle_scene(oracle, name), cameras()[name], RES, SPP, SEED, TS)


@pytest.fixture(scope="module")
def world():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    ctx = mp.Context(0)
    objs = wf.make_objects(ctx, CACHED)
    objs["sphere"] = mp.Sphere(*BALL, ctx)
    objs["group"] = mp.ObjectGroup([objs["teapot"], mp.Sphere(*BALL, ctx)], np.array(GROUP_AT, np.float32))
    return ctx, objs


def check_view(name, f):
    """the case shows what it is there for"""
    alpha = f[..., 3]
    if name == "teapot":
        blocks = alpha.reshape(RES[1] // 2, 2, RES[0] // 2, 2).transpose(0, 2, 1, 3).reshape(-1, 4)
        assert (blocks.max(1) == 0).any() and (blocks.min(1) == 1).any() and ((blocks.min(1) < 1) & (blocks.max(1) > 0)).any(), \
            "units that miss, interior units and silhouette units"
    elif name == "away":
        assert not alpha.any(), "every ray misses"
    elif name in ("atrium", "wide"):
        assert np.count_nonzero(alpha) > alpha.size // 2
    else:
        assert 0.0 < alpha.mean() < 1.0


@pytest.mark.parametrize("name", CACHED + ("sphere", "group"))
def test_frame_matches_the_oracle(oracle, world, name):
    ctx, objs = world
    of, ou8 = wanted(oracle, name)
    check_view(name, of)
    f, u8, names, _ = frame(ctx, objs[name], cameras()[name], mp.RenderSettings(TS, SPP, RES, seed=SEED))
    if name in CACHED:
        assert names == [PACKET], names
    else:
        assert len(names) == 1 and names[0].count(",") < 4, names  # (the cached instantiations are the ones with five arguments)
    print(f"{name}: {names}, {differing(f, of)} of {of.size} values differ from the oracle")
    assert_same_bits(f, of, name)
    assert np.array_equal(u8, ou8), name


@pytest.mark.parametrize("name", ["teapot", "atrium"])
def test_planes_match_the_model(oracle, world, name):
    ctx, objs = world
    img, names = planes(ctx, objs[name], cameras()[name], mp.RenderSettings(TS, AOV_SPP, RES, seed=SEED), WHICH)
    assert names == [AOV], names
    smp = oracle.sampler_from_array(cameras()[name].build_sampler(RES).as_array())
    want = aov_model.planes(oracle, oracle_scene(oracle, name).intersect, smp, RES[0], AOV_SPP, SEED, (0, 0, *RES))
    for k in WHICH:
        print(f"{name} {k}: {differing(img[k], want[k])} of {want[k].size} values differ from the model")
        assert_same_bits(img[k], want[k], (name, k))


def test_both_outcomes_of_the_unit_pretest_occur(oracle, tmp_path):
    got = run_in_variant("noskip", "tests.test_pass_hoist_gpu:counted_frames", tmp_path, timeout=600)
    units = (RES[0] // 2) * (RES[1] // 2)
    for name in ("teapot", "away", "wide"):
        assert_same_bits(got[name], wanted(oracle, name)[0], name)
        skip, keep = (int(v) for v in got[name + "_units"])
        print(f"{name}: {skip} units skip the per-ray pre-test, {keep} keep it")
        assert skip + keep == units, name
    skip, keep = (int(v) for v in got["teapot_units"])
    assert skip > 0 and keep > 0, "both outcomes in the teapot's frame"
    assert int(got["away_units"][0]) == 0, "a unit that looks away from the scene skipped the pre-test"
    skip, keep = (int(v) for v in got["wide_units"])
    assert keep > 0, "no unit of the wide lens fell back to the per-ray test"
    assert skip > 0, "no unit of the wide lens set its bounds from the corner rays"
