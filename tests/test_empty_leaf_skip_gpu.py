"""GPU tests (-m gpu) of the cached packet walk's skip of list entries whose leaf has an empty unit triangle mask (packet_walk.h,
trace_packet_cached: the visit that finds the mask empty marks the arena entry, later pops of the entry stop at the mark).

Frames against the oracle's bits, with the kernels named, in units of four passes -- the fewest the plans give a cached kernel
(launch_plan.cpp), so a mark set in pass 1 is met in passes 2 to 4: the teapot and the stand-in at a small detail (tests/graft_model.py's
eviction scene) at 64 x 48 and 64 spp on render_tiles_packet_kernel<16, ..., true> and on render_aov_packet_kernel<16, ..., true>,
and the teapot at depth 2 and 32 spp on render_paths_kernel<8, ..., true>, whose camera pass runs the cached walk.

The same frames in three other builds of the library (minipath_amd/csrc/Makefile), each in a process of its own
(tests/walk_frames.py, run_in_variant):
  lists_tiny  four table slots, 32 arena entries: lists that do not fit reset the arena in mid-unit, and marks must die with them
  shrunk      a negative margin of the corner bounds: passes leave the bounds, which widens them and clears the lists
  noskip      -DMP_NO_EMPTY_SKIP: the walk without marks
All three count (MP_PROF_MISSES); `pops_skipped` is the number of pops that stopped at a mark: non-zero in the first two, zero in
the third.  Every build gives the oracle's bits, so the frames with the skip on and off are the same."""
import functools

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib
from tests import aov_model
from tests import graft_model as gm
from tests.walk_frames import (Counters, assert_same_bits, cameras, counted, frame, make_objects, named, oracle_frame, oracle_scene, planes, run_in_variant,
                               teapot_oracle)

pytestmark = pytest.mark.gpu

RES, TS, SPP = (64, 48), 32, 64
TEAPOT_SEED, PATH_SPP, PATH_DEPTH = 21, 32, 2
SEEDS = {"teapot": TEAPOT_SEED, "atrium": gm.EVICT_SEED}
WHICH = ("ids", "albedo", "normal")
PACKET, AOV, PATHS = ("render_tiles_packet_kernel<16, false, 8, false, true>", "render_aov_packet_kernel<16, false, 8, false, true>",
                      "render_paths_kernel<8, false, false, true>")


def render_frames():
    """{name: array} of every frame, in the library that is loaded; "counters" where it counts"""
    lib = _lib.lib()
    prof = Counters(lib) if counted(lib) else None
    if prof:
        prof.reset()
    ctx = mp.Context(0)
    cams, objs, out = cameras(), make_objects(ctx, SEEDS), {}
    for name, seed in SEEDS.items():
        st = mp.RenderSettings(TS, SPP, RES, seed=seed)
        f, u8, names, _ = frame(ctx, objs[name], cams[name], st)
        assert names == [PACKET], names
        out[name], out[name + "_u8"] = f, u8
        img, names = planes(ctx, objs[name], cams[name], st, WHICH)
        assert names == [AOV], names
        for k in WHICH:
            out[f"{name}_{k}"] = img[k]
        if name == "teapot":
            f, u8, names, seg = frame(ctx, objs[name], cams[name], mp.RenderSettings(TS, PATH_SPP, RES, seed=seed, max_depth=PATH_DEPTH))
            assert names == [PATHS], names
            out["paths"], out["paths_u8"], out["paths_segments"] = f, u8, np.array([seg], np.int64)
    if prof:
        out["counters"] = np.array(list(prof.read().values()), np.uint64)
    return out


@functools.lru_cache(maxsize=None)
def wanted(oracle):
    """the oracle's frames, once: {name: array} as render_frames names them"""
    out = {}
    out["paths"], out["paths_u8"], seg = teapot_oracle(oracle, RES, PATH_SPP, TEAPOT_SEED, TS, PATH_DEPTH)
    out["paths_segments"] = np.array([seg], np.int64)
    for name, seed in SEEDS.items():
        out[name], out[name + "_u8"] = oracle_frame(oracle, name, RES, SPP, seed, TS)
        smp = oracle.sampler_from_array(cameras()[name].build_sampler(RES).as_array())
        pl = aov_model.planes(oracle, oracle_scene(oracle, name).intersect, smp, RES[0], SPP, seed, (0, 0, *RES))
        for k in WHICH:
            out[f"{name}_{k}"] = pl[k]
    assert 0.0 < out["teapot"][..., 3].mean() < 1.0 and np.count_nonzero(out["atrium"][..., 3]) > RES[0] * RES[1] // 2, "hits in view"
    return out


def compare(got, want):
    for k, w in want.items():
        g = got[k]
        if w.dtype.itemsize == 4 and g.dtype.itemsize == 4:  # f32 images and planes, the ids plane (u32 in the model, i32 from the device)
            assert_same_bits(g, w, k)
        else:
            assert np.array_equal(g, w), k


def test_frames_match_the_oracle(oracle):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    compare(render_frames(), wanted(oracle))


@pytest.mark.parametrize("variant", ["lists_tiny", "shrunk", "noskip"])
def test_frames_in_counted_builds(oracle, tmp_path, variant):
    got = run_in_variant(variant, "tests.test_empty_leaf_skip_gpu:render_frames", tmp_path, timeout=600)
    compare(got, wanted(oracle))
    c = named(got["counters"])
    builds, leaf_builds, bound_sets, resets, left, skipped = (c[k] for k in ("list_builds", "leaf_mask_builds", "bound_sets", "arena_resets",
                                                                              "passes_left_uncached", "pops_skipped"))
    print(f"{variant}: list builds {builds}, leaf-mask builds {leaf_builds}, inner links {c['inner_links']}, bound sets {bound_sets}, evictions {c['evictions']}, "
          f"arena resets {resets}, passes left to the uncached walk {left}, pops skipped at a mark {skipped}")
    assert builds > 0 and leaf_builds > 0, "the cached walk ran"
    if variant == "noskip":
        assert skipped == 0
    else:
        assert skipped > 0, "no pop met a mark"
    if variant == "lists_tiny":
        assert resets > 0 and left > 0, "no arena reset in mid-unit"
    if variant == "shrunk":
        assert bound_sets > RES[0] * RES[1] // 4, "the bounds were not widened in mid-unit"
