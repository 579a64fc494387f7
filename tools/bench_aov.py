#!/usr/bin/env python3
"""Time of one feature-plane launch (mp_render_aov_device: all planes; shade only; normal + albedo only) against the plain render
(mp_render_tiles_device) of the same settings, on the metric's frame (atrium stand-in, 1920x1080, 256 spp) and on the teapot
(1920x1080, 16 spp); on the teapot also the same planes by the ray API (mp_generate_rays + mp_trace_rays with full records per
sample + torch sums).  Device time between two events around REPS back-to-back launches, median / min / max over ROUNDS rounds:
the spread of the plain render's rounds is the session's noise.  Prints one line per (scene, mode).  Diagnostics only.
usage: bench_aov.py [--plain-only] [ATRIUM_DETAIL]
--plain-only: only the plain render -- for a library that predates the feature (MINIPATH_HIP_SO=older/libminipath_hip.so)."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import minipath_amd as mp
from minipath_amd import _lib, scenes

TEAPOT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "teapot.obj")
REPS, ROUNDS = 5, 7


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / REPS)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def ray_api_planes(ctx, bvh, cam, st):
    """shade / normal / albedo-free planes through the ray API: spp x (generate, trace with full records, torch adds in order)"""
    w, h = st.resolution
    n = w * h
    rays = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(6)]
    smp, sts = cam.build_sampler((w, h)).as_struct(), st.as_struct()
    acc = torch.zeros((n, 5), dtype=torch.float32, device="cuda")  # shade, n.xyz, t
    cnt = torch.zeros(n, dtype=torch.float32, device="cuda")
    for s in range(st.sample_count):
        _lib.check(_lib.lib().mp_generate_rays(ctx.handle, C.byref(smp), C.byref(sts), _lib.Block(0, 0, w, h), s,
                                               *[r.data_ptr() for r in rays], None))
        d = torch.stack(rays[3:], 1)
        hit = bvh.intersect(torch.stack(rays[:3], 1), d, full=True)
        m = (hit["prim"] != -1).float()
        nn = hit["normal"]
        acc[:, 0] += (d * nn).sum(1).abs() * m
        acc[:, 1:4] += nn * m[:, None]
        acc[:, 4] += hit["t"] * m
        cnt += m
    inv = 1.0 / st.sample_count
    return acc * inv, cnt * inv


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    plain_only = "--plain-only" in sys.argv
    if plain_only:
        _lib.SIGNATURES.pop("mp_render_aov_device", None)
    detail = float(args[0]) if args else 1.0
    ctx = mp.Context(0)
    cases = [("atrium", mp.TriangleBvh.build(*scenes.atrium(1, detail), ctx=ctx), scenes.atrium_camera(), 256),
             ("teapot", mp.TriangleBvh.with_obj(TEAPOT, ctx), mp.Camera.teapot_view(), 16)]
    print("library:", os.environ.get("MINIPATH_HIP_SO") or "default")
    for name, bvh, cam, spp in cases:
        st = mp.RenderSettings(64, spp, (1920, 1080), seed=1)
        fr = mp.FrameRenderer(mp.Scene(bvh), cam, st)
        rays = fr.samples_per_frame
        modes = {"render": fr.render}
        if not plain_only:
            modes["aov all"] = lambda: fr.render_aov()
            modes["aov shade"] = lambda: fr.render_aov(normal=False, albedo=False, ids=False)
            modes["aov normal+albedo"] = lambda: fr.render_aov(shade=False, ids=False)
            modes["render (again)"] = fr.render
        for mode, fn in modes.items():
            med, lo, hi = timed(fn)
            print(f"{name:7s} {spp:4d} spp  {mode:18s} {med:9.3f} ms  (min {lo:.3f} max {hi:.3f})  {rays / med / 1e6:8.2f} Grays/s")
            sys.stdout.flush()
        if name == "teapot" and not plain_only:
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ray_api_planes(ctx, bvh, cam, st)
            a.record()
            ray_api_planes(ctx, bvh, cam, st)
            b.record()
            torch.cuda.synchronize()
            print(f"{name:7s} {spp:4d} spp  {'ray API + torch':18s} {a.elapsed_time(b):9.3f} ms  (one run; shade, normal, t and alpha only)")


if __name__ == "__main__":
    main()
