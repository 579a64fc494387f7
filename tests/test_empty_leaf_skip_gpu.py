"""GPU tests (-m gpu) of the cached packet walk's skip of list entries whose leaf has an empty unit triangle mask (packet_walk.h,
trace_packet_cached: the visit that finds the mask empty marks the arena entry, later pops of the entry stop at the mark).

Frames against the oracle's bits, with the kernels named, in units of four passes -- the fewest the plans give a cached kernel
(launch_plan.cpp), so a mark set in pass 1 is met in passes 2 to 4: the teapot and the stand-in at a small detail (tests/graft_model.py's
eviction scene) at 64 x 48 and 64 spp on render_tiles_packet_kernel<16, ..., true> and on render_aov_packet_kernel<16, ..., true>,
and the teapot at depth 2 and 32 spp on render_paths_kernel<8, ..., true>, whose camera pass runs the cached walk.

The same frames in three other builds of the library (minipath_amd/csrc/Makefile), each in a process of its own:
  lists_tiny  four table slots, 32 arena entries: lists that do not fit reset the arena in mid-unit, and marks must die with them
  shrunk      a negative margin of the corner bounds: passes leave the bounds, which widens them and clears the lists
  noskip      -DMP_NO_EMPTY_SKIP: the walk without marks
All three count (MP_PROF_MISSES); slot 7 of mp_prof_read8 is the number of pops that stopped at a mark: non-zero in the first two,
zero in the third.  Every build gives the oracle's bits, so the frames with the skip on and off are the same.

Run as a program (MINIPATH_HIP_SO is read when the package loads) this file renders the frames and writes them to the .npz named."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RES, TS, SPP = (64, 48), 32, 64
TEAPOT_SEED, PATH_SPP, PATH_DEPTH = 21, 32, 2
WHICH = ("ids", "albedo", "normal")
PACKET, AOV, PATHS = ("render_tiles_packet_kernel<16, false, 8, false, true>", "render_aov_packet_kernel<16, false, 8, false, true>",
                      "render_paths_kernel<8, false, false, true>")


def render_frames():
    """{name: array} of every frame, in the library that is loaded; "counters" where it counts"""
    import torch

    import minipath_amd as mp
    from minipath_amd import _lib, scenes
    from tests import graft_model as gm
    from tests.conftest import TEAPOT
    from tests.unit_list_frames import frame, planes

    lib = _lib.lib()
    counted = hasattr(lib, "mp_prof_read8")
    cnt = (C.c_ulonglong * 8)()
    if counted:
        lib.mp_prof_read8.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
        assert lib.mp_prof_read8(cnt, 1) == 0
    ctx = mp.Context(0)
    out = {}
    for name, make, cam, seed in (("teapot", lambda: mp.TriangleBvh.with_obj(TEAPOT, ctx), mp.Camera.teapot_view(), TEAPOT_SEED),
                                  ("atrium", lambda: mp.TriangleBvh.build(*gm.evict_mesh(), ctx), scenes.atrium_camera(), gm.EVICT_SEED)):
        obj = make()
        st = mp.RenderSettings(TS, SPP, RES, seed=seed)
        f, u8, names, _ = frame(ctx, obj, cam, st)
        assert names == [PACKET], names
        out[name], out[name + "_u8"] = f, u8
        img, names = planes(ctx, obj, cam, st, WHICH)
        assert names == [AOV], names
        for k in WHICH:
            out[f"{name}_{k}"] = img[k]
        if name == "teapot":
            f, u8, names, seg = frame(ctx, obj, cam, mp.RenderSettings(TS, PATH_SPP, RES, seed=seed, max_depth=PATH_DEPTH))
            assert names == [PATHS], names
            out["paths"], out["paths_u8"], out["paths_segments"] = f, u8, np.array([seg], np.int64)
    torch.cuda.synchronize()
    if counted:
        assert lib.mp_prof_read8(cnt, 0) == 0
        out["counters"] = np.array(list(cnt), np.uint64)
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **render_frames())
    sys.exit(0)

import functools  # noqa: E402

import pytest  # noqa: E402

import minipath_amd as mp  # noqa: E402
from minipath_amd import scenes  # noqa: E402
from tests import aov_model  # noqa: E402
from tests import graft_model as gm  # noqa: E402
from tests.conftest import TEAPOT  # noqa: E402
from tests.unit_list_frames import bits, teapot_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
CSRC = os.path.join(ROOT, "minipath_amd", "csrc")


@functools.lru_cache(maxsize=None)
def wanted(oracle):
    """the oracle's frames, once: {name: array} as render_frames names them"""
    out = {}
    out["teapot"], out["teapot_u8"], _ = teapot_oracle(oracle, RES, SPP, TEAPOT_SEED, TS)
    out["paths"], out["paths_u8"], seg = teapot_oracle(oracle, RES, PATH_SPP, TEAPOT_SEED, TS, PATH_DEPTH)
    out["paths_segments"] = np.array([seg], np.int64)
    asmp = oracle.sampler_from_array(scenes.atrium_camera().build_sampler(RES).as_array())
    out["atrium"], out["atrium_u8"], *_ = gm.evict_oracle(oracle).render_image_mt(asmp, *RES, SPP, gm.EVICT_SEED, TS, 16)
    tsmp = oracle.sampler_from_array(mp.Camera.teapot_view().build_sampler(RES).as_array())
    for name, intersect, smp, seed in (("teapot", oracle.Bvh.from_obj(TEAPOT).intersect, tsmp, TEAPOT_SEED),
                                       ("atrium", gm.evict_oracle(oracle).intersect, asmp, gm.EVICT_SEED)):
        pl = aov_model.planes(oracle, intersect, smp, RES[0], SPP, seed, (0, 0, *RES))
        for k in WHICH:
            out[f"{name}_{k}"] = pl[k]
    assert 0.0 < out["teapot"][..., 3].mean() < 1.0 and np.count_nonzero(out["atrium"][..., 3]) > RES[0] * RES[1] // 2, "hits in view"
    return out


def compare(got, want):
    for k, w in want.items():
        g = got[k]
        if w.dtype.itemsize == 4 and g.dtype.itemsize == 4:  # f32 images and planes, the ids plane (u32 in the model, i32 from the device)
            diff = int(np.sum(bits(g) != bits(w)))
            assert g.shape == w.shape and diff == 0, (k, diff)
        else:
            assert np.array_equal(g, w), k


def test_frames_match_the_oracle(oracle):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    compare(render_frames(), wanted(oracle))


@pytest.mark.parametrize("variant", ["lists_tiny", "shrunk", "noskip"])
def test_frames_in_counted_builds(oracle, tmp_path, variant):
    so = os.path.join(CSRC, f"libminipath_hip_{variant}.so")
    if not os.path.exists(so):
        pytest.fail(f"{so} missing: run build() first")
    dst = str(tmp_path / "frames.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), dst], env=dict(os.environ, MINIPATH_HIP_SO=so), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    with np.load(dst) as z:
        got = {k: z[k] for k in z.files}
    compare(got, wanted(oracle))
    builds, leaf_builds, links, bound_sets, evictions, resets, left, skipped = (int(v) for v in got["counters"])
    print(f"{variant}: list builds {builds}, leaf-mask builds {leaf_builds}, inner links {links}, bound sets {bound_sets}, evictions {evictions}, "
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
