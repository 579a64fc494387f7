"""GPU tests (-m gpu) of the far-side terms of the unit triangle masks (mask_cache.h, tri_may_hit: u.lo > 1 or v.lo > 1 rejects).

(a) The probe (mask_probe.hip, far_kernel through mp_mask_probe_far): tri_may_hit against the per-ray sequence of 192 rays inside each
    box, on boxes that lie beyond a triangle's far edges and on exact-boundary cases (a corner ray of the box aimed at v1, at v2 or at
    a point of the edge v1 v2 with exact arithmetic, one ulp inside, one ulp outside).  No violation; cases that only the new terms
    reject and boundary cases that are accepted and kept must both occur.
(b) Frames against the oracle's bits at 96 x 64 in tiles of 32: 64 samples on render_tiles_packet_kernel<16, ..., true> (four passes per
    unit, the fewest that get the cached kernel) and the feature planes at 32 samples on render_aov_packet_kernel<4, ..., true>:
      teapot   units that miss, silhouette units and interior units
      atrium   the stand-in at detail 0.5, an interior view
      wide     the stand-in through a lens 2.5 m across
      vertex   the stand-in with the eye exactly on a vertex of the mesh (u, v, t = +-0 at the triangles that share it)
(c) The same frames in two counted builds of the library (minipath_amd/csrc/Makefile: maskfar, the shipped rule, and nomaskfar,
    -DMP_NO_MASK_FAR; both -DMP_PROF_MISSES -DMP_PROF_MASK_TRIS, so `leaf_mask_builds` is the number of leaf-mask builds and the slot
    after it, `inner_links` in other builds, the number of triangles those masks keep), each in a process of its own
    (tests/walk_frames.py, run_in_variant): both give the oracle's bits, and the masks of the shipped rule keep strictly fewer
    triangles per build."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib
from tests import aov_model
from tests import graft_model as gm
from tests import walk_frames as wf
from tests.walk_frames import CSRC, Counters, assert_same_bits, differing, frame, planes, run_in_variant

pytestmark = pytest.mark.gpu
PROBE = os.path.join(CSRC, "libmp_mask_probe.so")

RES, TS, SPP, AOV_SPP = (96, 64), 32, 64, 32
SEED = 41
WHICH = ("shade", "normal", "ids")
PACKET = "render_tiles_packet_kernel<16, false, 8, false, true>"
AOV = "render_aov_packet_kernel<4, false, 8, false, true>"
SCENES = ("teapot", "atrium", "wide", "vertex")
NCASES = 1 << 18


def vertex_eye():
    """a vertex of the stand-in's mesh all of whose coordinates are of magnitude >= 1 (the pinhole's lens offset rounds away, so every
    ray starts on it), and a point to look at"""
    p = gm.evict_mesh()[0].reshape(-1, 3)
    ok = np.nonzero(np.all(np.abs(p) >= 1.0, axis=1))[0]
    v = p[ok[len(ok) // 2]]
    return tuple(float(x) for x in v), (float(v[0]) + 3.0, float(v[1]) + 0.25, float(v[2]) - 1.0)


def cameras():
    eye, at = vertex_eye()
    return {**wf.cameras(), "vertex": mp.Camera.default().look_at(eye, at, (0.0, 1.0, 0.0)).f_number(1e30)}


def make_objects(ctx):
    out = wf.make_objects(ctx, SCENES)
    out["vertex"] = out["atrium"]
    return out


def counted_frames():
    """{name: f32 frame, name + "_masks": (leaf-mask builds, triangles the built masks keep)} in the library that is loaded"""
    prof = Counters(_lib.lib())
    ctx = mp.Context(0)
    cams, objs, out = cameras(), make_objects(ctx), {}
    for name in SCENES:
        prof.reset()
        f, _, names, _ = frame(ctx, objs[name], cams[name], mp.RenderSettings(TS, SPP, RES, seed=SEED))
        assert names == [PACKET], names
        c = prof.read()
        out[name], out[name + "_masks"] = f, np.array([c["leaf_mask_builds"], c["inner_links"]], np.uint64)  # (-DMP_PROF_MASK_TRIS: triangles kept)
    return out


def test_probe_beyond_the_far_edges():
    if not os.path.exists(PROBE):
        pytest.fail(f"{PROBE} missing: run build() first")
    import torch

    # (the renderer's HIP runtime is initialised before the probe's copy loads, the order the whole suite has)
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    torch.zeros(1, device="cuda")
    L = C.CDLL(PROBE)
    L.mp_mask_probe_far.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    o = (C.c_ulonglong * 8)()
    rc = L.mp_mask_probe_far(0xFA5, NCASES, o)
    assert rc == 0, f"HIP error {rc}"
    print(f"tri_may_hit, far side: violations {o[0]} cases {o[1]} first {o[2]:#x} hit {o[3]} rejected {o[4]} by the new terms only {o[5]} "
          f"boundary cases kept {o[6]}")
    assert o[1] == NCASES
    assert o[0] == 0, f"{o[0]} cases rejected although a ray inside B hits; first case {o[2]}"
    # (the numpy twin of the generator, tests/test_mask_far_side_cpu.py: a quarter of the far family's cases are rejected by the new
    # terms only, three quarters of the exact family's are boundary cases kept; the bounds ask for a tenth of each)
    assert o[5] >= NCASES * 5 // 8 // 40, "too few cases that only the far-side terms reject"
    assert o[6] >= NCASES * 3 // 8 // 10, "too few exact-boundary cases that are accepted and kept"
    assert o[3] > 0 and o[4] > o[5]


def oracle_scene(oracle, name):
    return wf.oracle_scene(oracle, "atrium" if name == "vertex" else name)


@functools.lru_cache(maxsize=None)
def wanted(oracle, name):
    """the oracle's frame of a scene, once: (f32, u8)"""
    if name != "vertex":
        return wf.oracle_frame(oracle, name, RES, SPP, SEED, TS)
    return wf.oracle_image(oracle, oracle_scene(oracle, name), cameras()[name], RES, SPP, SEED, TS)


@pytest.fixture(scope="module")
def world():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    ctx = mp.Context(0)
    return ctx, make_objects(ctx)


def check_view(name, f):
    """the scene shows what it is there for"""
    alpha = f[..., 3]
    if name == "teapot":
        assert 0.0 < alpha.mean() < 1.0
    else:
        assert np.count_nonzero(alpha) > alpha.size // 2


@pytest.mark.parametrize("name", SCENES)
def test_frame_matches_the_oracle(oracle, world, name):
    ctx, objs = world
    of, ou8 = wanted(oracle, name)
    check_view(name, of)
    f, u8, names, _ = frame(ctx, objs[name], cameras()[name], mp.RenderSettings(TS, SPP, RES, seed=SEED))
    assert names == [PACKET], names
    print(f"{name}: {names}, {differing(f, of)} of {of.size} values differ from the oracle")
    assert_same_bits(f, of, name)
    assert np.array_equal(u8, ou8), name


@pytest.mark.parametrize("name", SCENES)
def test_planes_match_the_model(oracle, world, name):
    ctx, objs = world
    img, names = planes(ctx, objs[name], cameras()[name], mp.RenderSettings(TS, AOV_SPP, RES, seed=SEED), WHICH)
    assert names == [AOV], names
    smp = oracle.sampler_from_array(cameras()[name].build_sampler(RES).as_array())
    want = aov_model.planes(oracle, oracle_scene(oracle, name).intersect, smp, RES[0], AOV_SPP, SEED, (0, 0, *RES))
    for k in WHICH:
        print(f"{name} {k}: {differing(img[k], want[k])} of {want[k].size} values differ from the model")
        assert_same_bits(img[k], want[k], (name, k))


def test_masks_keep_fewer_triangles_than_without_the_far_side(oracle, tmp_path):
    on, off = (run_in_variant(v, "tests.test_mask_far_side_gpu:counted_frames", tmp_path, timeout=600) for v in ("maskfar", "nomaskfar"))
    for name in SCENES:
        of = wanted(oracle, name)[0]
        assert_same_bits(on[name], of, ("maskfar", name))
        assert_same_bits(off[name], of, ("nomaskfar", name))
        (b1, k1), (b0, k0) = (int(v) for v in on[name + "_masks"]), (int(v) for v in off[name + "_masks"])
        print(f"{name}: leaf-mask builds {b1} / {b0}, triangles kept {k1} / {k0}: per build {k1 / max(b1, 1):.2f} with the far side, "
              f"{k0 / max(b0, 1):.2f} without")
        assert b1 > 0 and b0 > 0, "the cached walk built masks"
        assert k1 * b0 < k0 * b1, f"{name}: the far-side terms dropped no triangle"
