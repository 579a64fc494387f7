#!/usr/bin/env python3
"""Slow-path calls of the packet walk's mask cache per work unit and pass (a build with -DMP_PROF_MISSES: tools/build_variant.sh prof
"-DMP_PROF_MISSES", run with MINIPATH_HIP_SO=variants/libmp_prof.so), read through mp_prof_read_n by the reader the tests use
(tests/walk_frames.py, Counters: the counters by name).  usage: cache_miss_count.py [atrium|teapot] [spp]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import minipath_amd as mp
from minipath_amd import scenes, _lib
from tests.walk_frames import Counters

which = sys.argv[1] if len(sys.argv) > 1 else "atrium"
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 256
ctx = mp.Context(0)
if which == "atrium":
    scene, cam = mp.Scene(mp.TriangleBvh.build(*scenes.atrium(1, 1.0), ctx)), scenes.atrium_camera()
else:
    scene, cam = mp.Scene(mp.TriangleBvh.with_obj(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "teapot.obj"), ctx)), mp.Camera.teapot_view()
fr = mp.FrameRenderer(scene, cam, mp.RenderSettings(64, spp, (1920, 1080), seed=0x5EED))
fr.render(); torch.cuda.synchronize()
prof = Counters(_lib.lib())
prof.reset()
fr.render()
c = prof.read()
S = 16 if spp >= 64 else 8 if spp >= 32 else 4
units = 1920 * 1080 // (64 // S)
passes = units * (spp // S)
print(f"{which} x{spp}: per unit: node-list slow paths {c['list_builds'] / units:.1f}, leaf-mask slow paths {c['leaf_mask_builds'] / units:.1f}, bounds (re)set {c['bound_sets'] / units:.2f};"
      f" per pass: node visits (inner links followed) {c['inner_links'] / passes:.2f}")
print(f"{which} x{spp}: per unit: node-table evictions {c['evictions'] / units:.3f}, arena resets {c['arena_resets'] / units:.4f}; passes left to the uncached walk: {c['passes_left_uncached']} of {passes}")
print(f"{which} x{spp}: per pass: pops skipped on an empty-mask leaf {c['pops_skipped'] / passes:.3f}")
if len(sys.argv) > 3 and sys.argv[3] == "mask-tris":
    # a build with -DMP_PROF_MASK_TRIS as well: the slot named inner_links is not the inner links followed (the "node visits" above)
    # but the triangles the built leaf masks keep, so it over leaf_mask_builds is the mean popcount of a stored mask (the model:
    # tools/tri_exit_count.py)
    kept, built = c["inner_links"], c["leaf_mask_builds"]
    print(f"{which} x{spp}: per leaf-mask build: surviving triangles {kept / max(built, 1):.2f} ({kept} in {built} builds); the node visits above are not counted in this build")
