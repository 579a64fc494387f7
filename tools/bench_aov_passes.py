#!/usr/bin/env python3
"""Time of the feature planes through mp_render_aov_pass_device on the two frames of tools/bench_aov.py (atrium stand-in,
1920x1080, 256 spp; teapot, 1920x1080, 16 spp): the four old planes and all six in one launch, and all six with the frame split
into 4 and into 16 equal passes -- beside the plain render in one launch and in the same passes (render_pass), which is the
render's own cost of splitting.  The planes are allocated once per mode (render_aov() of bench_aov.py allocates and zero-fills its
planes per launch; "aov all (old entry)" here is that call, for the bridge between the two tools).  Device time between two events
around REPS frames, median / min / max over ROUNDS rounds.  Prints one line per (scene, mode).  Diagnostics only.
usage: bench_aov_passes.py [ATRIUM_DETAIL]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import minipath_amd as mp
from minipath_amd import scenes
from tools.bench_aov import TEAPOT, timed


def in_passes(step, total, passes):
    """one frame as `passes` equal passes of step(begin, count)"""
    per = total // passes

    def frame():
        nxt = 0
        for p in range(passes):
            nxt = step(nxt, per if p < passes - 1 else 0)
        assert nxt == total
    return frame


def main():
    detail = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    ctx = mp.Context(0)
    cases = [("atrium", mp.TriangleBvh.build(*scenes.atrium(1, detail), ctx=ctx), scenes.atrium_camera(), 256),
             ("teapot", mp.TriangleBvh.with_obj(TEAPOT, ctx), mp.Camera.teapot_view(), 16)]
    print("library:", os.environ.get("MINIPATH_HIP_SO") or "default")
    for name, bvh, cam, spp in cases:
        fr = mp.FrameRenderer(mp.Scene(bvh), cam, mp.RenderSettings(64, spp, (1920, 1080), seed=1))
        rays = fr.samples_per_frame
        four = fr.new_aov_planes()
        six = fr.new_aov_planes(position=True, shade_sq=True)
        two = fr.new_aov_planes(shade=False, normal=False, albedo=False, ids=False, position=True, shade_sq=True)
        modes = {"render": fr.render,
                 "aov all (old entry)": lambda: fr.render_aov(),
                 "pass entry, four": lambda: fr.render_aov_pass(four),
                 "pass entry, P + sq": lambda: fr.render_aov_pass(two),
                 "pass entry, six": lambda: fr.render_aov_pass(six)}
        for passes in (4, 16):
            modes[f"six, {passes} passes"] = in_passes(lambda b, c: fr.render_aov_pass(six, b, c), spp, passes)
            modes[f"render, {passes} passes"] = in_passes(fr.render_pass, spp, passes)
        modes["render (again)"] = fr.render
        for mode, fn in modes.items():
            med, lo, hi = timed(fn)
            print(f"{name:7s} {spp:4d} spp  {mode:20s} {med:9.3f} ms  (min {lo:.3f} max {hi:.3f})  {rays / med / 1e6:8.2f} Grays/s")
            sys.stdout.flush()
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
