"""Support for the tests that render frames through the cached packet walk (packet_walk.h, trace_packet_cached): one context per
tree format, a frame or its feature planes with the kernels that ran, the views and scenes those tests share with the oracle's
images of them (computed once per case), the bit compare, and -- for the Makefile's `test-variants`, the library rebuilt with
other tunables or with counters -- a runner that calls a function in a process of its own which loads that build, and a reader
of the build's counters by name.

Run as a program, `python -m tests.walk_frames tests.test_x:function dst.npz [args]`, this module is that process: it calls the
function with the arguments and saves the {name: array} it returns.  (MINIPATH_HIP_SO is read when the package first loads the
library, so it is set by the parent.)"""
import ctypes as C
import functools
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import scenes
from tests import dispatch_cases as dc
from tests import graft_model as gm
from tests.conftest import ROOT, TEAPOT

SLOTS = (16, 8)
CSRC = os.path.join(ROOT, "minipath_amd", "csrc")


# ---- the bit compare -------------------------------------------------------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def differing(got, want):
    """the number of 32-bit words in which two arrays of one shape differ"""
    return int(np.sum(bits(got) != bits(want)))


def assert_same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = differing(got, want)
    assert diff == 0, f"{what}: {diff} of {want.size} words differ"


# ---- frames ----------------------------------------------------------------------------------------------------------------------

def make_contexts():
    """{slots: context}: the scenes made on each take its tree format at upload"""
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    out = {}
    for s in SLOTS:
        c = mp.Context(0)
        c.set_option("packet_tree_slots", s)
        out[s] = c
    return out


# "blocks_per_cu" (a diagnostic knob, 0 = as many as fit): 1 lets the launchers see an eighth of the CUs, so that the waves of a
# persistent kernel run many work units each on a small frame (tests/long_waves.py)
LEVERS = {"blocks_per_cu": 0}


def set_options(ctx, **opts):
    for k, v in {**dc.DEFAULTS, **LEVERS, **opts}.items():
        ctx.set_option(k, v)


def frame(ctx, obj, cam, st, **opts):
    """one frame through FrameRenderer: (f32 image, u8 image, kernels reported, ray segments)"""
    import torch

    set_options(ctx, **opts)
    try:
        fr = mp.FrameRenderer(mp.Scene(obj), cam, st)
        fr.render()
        names = dc.launched(ctx)
        img, img8 = fr.untile()
        torch.cuda.synchronize()
        return img.cpu().numpy(), img8.cpu().numpy(), names, int(fr.segments.item())
    finally:
        set_options(ctx)


def planes(ctx, obj, cam, st, which, **opts):
    """the feature planes `which` of one frame: ({name: image}, kernels reported)"""
    import torch

    set_options(ctx, **opts)
    try:
        fr = mp.FrameRenderer(mp.Scene(obj), cam, st)
        out = fr.render_aov(**{k: k in which for k in ("shade", "normal", "albedo", "ids")})
        names = dc.launched(ctx)
        img = {k: fr.untile_plane(out[k]).cpu().numpy() for k in which}
        torch.cuda.synchronize()
        return img, names
    finally:
        set_options(ctx)


def check_formats(ctxs, make_obj, cam, st, want, name_re, **opts):
    """the frame under both formats: the scene holds its context's format, the one kernel matches name_re, the image is the
    oracle's bit for bit -- and so the two formats agree"""
    of, ou8 = want
    got = {}
    for slots, ctx in ctxs.items():
        obj = make_obj(ctx)
        assert obj.device_tree(packet=True)[0].shape[1] == slots
        f, u8, names, _ = frame(ctx, obj, cam, st, **opts)
        assert len(names) == 1 and re.fullmatch(name_re, names[0]), (slots, names)
        assert_same_bits(f, of, (slots, names))
        assert np.array_equal(u8, ou8), slots
        got[slots] = f
    assert np.array_equal(bits(got[16]), bits(got[8]))


# ---- the views the tests share: cameras, device objects, the oracle's twins and frames -------------------------------------------

def cameras():
    """teapot: units that miss the scene, units on the silhouette and units inside it.  atrium: the stand-in scene of
    tests/graft_model.py (evict_mesh), an interior view.  away: the teapot's camera turned round, every ray misses.  wide: the
    atrium through a lens 2.5 m across."""
    eye = (0.0, 2.0, 10.0)  # Camera.teapot_view's
    return {"teapot": mp.Camera.teapot_view(),
            "atrium": scenes.atrium_camera(),
            "away": mp.Camera.default().look_at(eye, (0.0, 2.5, 20.0), (0.0, 1.0, 0.0)).f_number(4.8),
            "wide": scenes.atrium_camera().f_number(0.01)}


def make_objects(ctx, names):
    """{name: device object} of the views named: the teapot for `teapot` and `away`, the stand-in for `atrium` and `wide`"""
    out = {}
    if {"teapot", "away"} & set(names):
        out["teapot"] = out["away"] = mp.TriangleBvh.with_obj(TEAPOT, ctx)
    if {"atrium", "wide"} & set(names):
        out["atrium"] = out["wide"] = mp.TriangleBvh.build(*gm.evict_mesh(), ctx)
    return out


@functools.lru_cache(maxsize=None)
def oracle_scene(oracle, name):
    """the oracle's twin of a shared view's scene, once"""
    return oracle.Bvh.from_obj(TEAPOT) if name in ("teapot", "away") else gm.evict_oracle(oracle)


def oracle_image(oracle, twin, cam, res, spp, seed, ts):
    """the oracle's frame of a Bvh through a camera of this package: (f32, u8)"""
    smp = oracle.sampler_from_array(cam.build_sampler(res).as_array())
    f, u8, *_ = twin.render_image_mt(smp, *res, spp, seed, ts, 16)
    return f, u8


@functools.lru_cache(maxsize=None)
def oracle_frame(oracle, name, res, spp, seed, ts):
    """the oracle's frame of a shared view, once: (f32, u8)"""
    return oracle_image(oracle, oracle_scene(oracle, name), cameras()[name], res, spp, seed, ts)


@functools.lru_cache(maxsize=None)
def teapot_oracle(oracle, res, spp, seed, ts, depth=0):
    if depth:
        smp = oracle.sampler_from_array(mp.Camera.teapot_view().build_sampler(res).as_array())
        f, u8, _, seg = oracle.Bvh.from_obj(TEAPOT).render_image_paths_mt(smp, *res, spp, seed, depth, ts, 16)
        return f, u8, seg
    return (*oracle_frame(oracle, "teapot", res, spp, seed, ts), None)


def evict_oracle_image(oracle, spp):
    return oracle_frame(oracle, "atrium", gm.EVICT_RES, spp, gm.EVICT_SEED, gm.EVICT_TS)


# ---- the counters of a counted build (-DMP_PROF_MISSES), by name ------------------------------------------------------------------

# g_prof's slots in order (prof_counters.h; family_launch.h, kProfSlots)
PROF_SLOTS = (
    "list_builds",
    "leaf_mask_builds",
    "inner_links",  # under -DMP_PROF_MASK_TRIS (the maskfar and nomaskfar builds) instead: triangles the built leaf masks keep
    "bound_sets",
    "evictions",
    "arena_resets",
    "passes_left_uncached",  # passes left to the uncached walk
    "pops_skipped",  # pops that stopped at the mark of an empty-mask leaf
    "units_skip_pretest",  # units whose passes skip the per-ray scene pre-test
    "units_keep_pretest",
    "passes_bounds_entry",  # passes that enter the cached walk on the one bounds test
    "passes_full_entry",  # ... through the full guards
)


def counted(lib):
    """does the loaded library count (only a -DMP_PROF_MISSES build exports the reader)"""
    return hasattr(lib, "mp_prof_read_n")


def named(values):
    """{name: int} of all the counters in slot order, as an array of them travels through a child's .npz"""
    assert len(values) == len(PROF_SLOTS), len(values)
    return dict(zip(PROF_SLOTS, (int(v) for v in values)))


class Counters:
    """all the counters of the loaded (counted) library, summed over the units that run the cached walk"""

    def __init__(self, lib):
        self._read = lib.mp_prof_read_n
        self._read.argtypes = [C.POINTER(C.c_ulonglong), C.c_int, C.c_int]

    def read(self, reset=False):
        """{name: int} once the device is idle; with reset, the counters are zero afterwards"""
        import torch

        torch.cuda.synchronize()
        cnt = (C.c_ulonglong * len(PROF_SLOTS))()
        assert self._read(cnt, len(PROF_SLOTS), int(reset)) == 0
        return named(cnt)

    def reset(self):
        self.read(reset=True)


# ---- a function in a process of its own, with a variant of the library -----------------------------------------------------------

def run_in_variant(variant, target, tmp_path, *args, timeout, csrc=CSRC):
    """target ("tests.test_x:function") called with the strings args in one child process that loads libminipath_hip_<variant>.so
    from csrc: the {name: array} it returned.  One child, waited for; nothing is retried."""
    so = os.path.join(csrc, f"libminipath_hip_{variant}.so")
    if not os.path.exists(so):
        pytest.fail(f"{so} missing: run build() first")
    dst = str(tmp_path / f"{variant}.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-m", "tests.walk_frames", target, dst, *args], env=dict(os.environ, MINIPATH_HIP_SO=so), cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    with np.load(dst) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    module, _, function = sys.argv[1].partition(":")
    np.savez(sys.argv[2], **getattr(importlib.import_module(module), function)(*sys.argv[3:]))
