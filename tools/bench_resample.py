#!/usr/bin/env python3
"""Device time of the guided resampling (mpr_downsample, mpr_upsample, include/minipath_resample.h) at 1920x1080 for f = 2 and 4
against their traffic floors, and the whole 8-sample ambient-occlusion frame traced at the low resolution and brought back against
SecondaryVisibility.ambient_occlusion at full resolution.

Planes: the renderer's own untiled "position", "normal" and "ids" planes at one sample per pixel of the atrium stand-in and of the
teapot.  T = device time between two events around REPS back-to-back calls; the runs of one table alternate inside every round,
median / min / max over ROUNDS rounds (the protocol of tools/bench_secondary.py).  Floor = the bytes the definition must touch / the
rate a copy reaches on this machine (COPY_GBS):
  downsample phase    per low pixel: 16 B of each of position, normal and ids at the candidate (the guides are two of the three
                      sources) and 3 x 16 + 4 B written: 100 B
  downsample nearest  32 B per full pixel (every pixel's depth is looked at), 16 B of ids and 52 B written per low pixel
  upsample            48 B per full pixel (two guides read, out written) and 52 B per low pixel (three planes and the pick)
  frame low           GuidedResampler.downsample(position, normal, ids) -> SecondaryVisibility at the low resolution, 8 samples in
                      batches of 4 -> GuidedResampler.upsample
  frame full          SecondaryVisibility.ambient_occlusion at 1920x1080, the same samples and batches
Prints one line per run.  Diagnostics only.
usage: bench_resample.py [ATRIUM_DETAIL]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import minipath_amd as mp
from minipath_amd import resample as rs
from minipath_amd import scenes

W, H = 1920, 1080
REPS, ROUNDS = 20, 9
COPY_GBS = 6290.0
SAMPLES = 8
FACTORS = (2, 4)
TEAPOT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "teapot.obj")


def frame_planes(scene, cam):
    fr = mp.FrameRenderer(scene, cam, mp.RenderSettings(64, 1, (W, H), seed=1))
    pl = fr.new_aov_planes(position=True)
    fr.render_aov_pass(pl)
    img = {k: fr.untile_plane(pl[k]) for k in ("position", "normal", "ids")}
    torch.cuda.synchronize()
    return img


def timed(runs):
    """runs: name -> callable; ms[name] = per-call device times over ROUNDS rounds, the runs alternating inside a round"""
    for f in runs.values():  # warm-up
        f()
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, f in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPS):
                f()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / REPS)
    return {k: np.array(v) for k, v in ms.items()}


def line(name, t, floor_ms=None, extra=""):
    med = float(np.median(t))
    s = f"{name:34s} {med * 1e3:9.1f} us  (min {t.min() * 1e3:.1f} max {t.max() * 1e3:.1f})"
    if floor_ms is not None:
        s += f"  floor {floor_ms * 1e3:6.1f} us  ratio {med / floor_ms:5.2f}"
    print(s + ("  " + extra if extra else ""))
    return med


def bench_scene(name, bvh, cam, radius):
    scene = mp.Scene(bvh)
    img = frame_planes(scene, cam)
    position, normal, ids = img["position"], img["normal"], img["ids"]
    pixels = W * H
    hits = float((position[..., 3] > 0).float().mean())
    print(f"---- {name}: {W}x{H}, hit pixels {hits:.3f}, radius {radius}")
    full = mp.SecondaryVisibility(scene, (W, H), batch=4)
    runs, floors, frames = {}, {}, {}
    keep = []
    for f in FACTORS:
        r = mp.GuidedResampler((W, H), f)
        lw, lh = r.low_resolution
        low = lw * lh
        vis = mp.SecondaryVisibility(scene, r.low_resolution, batch=4)
        keep.append((r, vis))
        runs[f"downsample phase f={f}"] = lambda r=r: r.downsample(position, normal, ids, phase=1)
        floors[f"downsample phase f={f}"] = low * 100 / (COPY_GBS * 1e9) * 1e3
        runs[f"downsample nearest f={f}"] = lambda r=r: r.downsample(position, normal, ids, pick="nearest")
        floors[f"downsample nearest f={f}"] = (pixels * 32 + low * 68) / (COPY_GBS * 1e9) * 1e3
        # upsample on the planes of a phase downsample and that frame's low ambient occlusion
        p_lo, n_lo, _ = r.downsample(position, normal, ids, phase=1)
        ao_lo = vis.ambient_occlusion(p_lo, n_lo, cam, SAMPLES, radius, seed=7)[0].clone()
        # a resampler of its own, so that the timed downsamples above leave these picks alone
        up = mp.GuidedResampler((W, H), f)
        up.downsample(position, normal, phase=1)
        keep.append(up)
        runs[f"upsample f={f}"] = lambda up=up, ao_lo=ao_lo: up.upsample(ao_lo, position, normal)
        floors[f"upsample f={f}"] = (pixels * 48 + low * 52) / (COPY_GBS * 1e9) * 1e3

        def frame_low(r=r, vis=vis):
            p, n, _ = r.downsample(position, normal, ids, phase=1)
            ao, _ = vis.ambient_occlusion(p, n, cam, SAMPLES, radius, seed=7)
            return r.upsample(ao, position, normal)
        frames[f"frame low f={f} 8 (4+4)"] = frame_low
    ms = timed(runs)
    for k in runs:
        line(k, ms[k], floors[k])
    frames["frame full 8 (4+4)"] = lambda: full.ambient_occlusion(position, normal, cam, SAMPLES, radius, seed=7)
    ms = timed(frames)
    med = {k: line(k, ms[k]) for k in frames}
    print("frame full / frame low: " + "  ".join(f"f={f}: {med['frame full 8 (4+4)'] / med[f'frame low f={f} 8 (4+4)']:.2f}" for f in FACTORS))
    # what the resampled frame shows against the full-resolution one (the same 8 samples per traced pixel, 1 / f^2 of the rays)
    ref = full.ambient_occlusion(position, normal, cam, 64, radius, seed=11)[0].clone()
    same = full.ambient_occlusion(position, normal, cam, SAMPLES, radius, seed=7)[0].clone()
    hit = position[..., 3] > 0
    err = {"full 8": float((same[..., 0] - ref[..., 0]).abs()[hit].mean())}
    for f in FACTORS:
        out = frames[f"frame low f={f} 8 (4+4)"]()
        err[f"low f={f}"] = float((out[..., 0] - ref[..., 0]).abs()[hit].mean())
        holes = int(((out[..., 3] == 0) & hit).sum())
        err[f"holes f={f}"] = holes
    torch.cuda.synchronize()
    print("mean |v - v64| at hits against 64 samples at full resolution: " + "  ".join(f"{k}: {v:.4f}" if isinstance(v, float) else f"{k}: {v}"
                                                                                         for k, v in err.items()))
    sys.stdout.flush()


def main():
    detail = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    ctx = mp.Context(0)
    bench_scene("atrium", mp.TriangleBvh.build(*scenes.atrium(1, detail), ctx=ctx), scenes.atrium_camera(), 2.0)
    bench_scene("teapot", mp.TriangleBvh.with_obj(TEAPOT, ctx), mp.Camera.teapot_view(), 1.0)
    print("kernels: " + ", ".join(rs.last_kernels()))


if __name__ == "__main__":
    main()
