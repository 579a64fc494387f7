#!/usr/bin/env python3
"""Device time of the temporal reprojection (mpt_reproject, include/minipath_temporal.h) at 1920x1080, with and without
variance_in, against its traffic floor and against the frame it accompanies.

Planes: "atrium" -- two frames of the atrium stand-in at 16 spp from a camera that moves a little (0.05 to the side and a small
turn), the renderer's own untiled planes, the first frame's mpt_reset as history: what a user's second frame does; "kept" -- the
atrium's first frame reprojected onto itself through its own view with an unbounded position radius, so that every tap of every
hit pixel is kept and all eight history loads of every pixel are made: the most the kernel can be given.
T = device time between two events around REPS back-to-back calls; the four (planes, variance) runs alternate inside every round,
median / min / max over ROUNDS rounds.  Floor = the bytes the definition must move / the rate a copy reaches on this machine
(COPY_GBS): the pixel's own planes read (four, five with variance_in), the five history planes read once, two
planes written and variance_out, 16 B per pixel each.
Also times the 1-spp and the 16-spp render of the frame (FrameRenderer.render, the same events) and prints the reprojection as a
fraction of each.  Prints one line per run.  Diagnostics only.
usage: bench_temporal.py [ATRIUM_DETAIL]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import minipath_amd as mp
from minipath_amd import scenes
from minipath_amd import temporal as tp

W, H = 1920, 1080
REPS, ROUNDS = 20, 9
COPY_GBS = 6290.0
PLANES = {False: 4 + 5 + 3, True: 5 + 5 + 3}  # read own + read history + written, by variance_in


def frame_planes(scene, cam, seed):
    fr = mp.FrameRenderer(scene, cam, mp.RenderSettings(64, 16, (W, H), seed=seed))
    pl = fr.new_aov_planes(albedo=False, position=True, shade_sq=True)
    fr.render_aov_pass(pl)
    img = {k: fr.untile_plane(v) for k, v in pl.items()}
    img["variance"] = mp.AtrousDenoiser((W, H), 0).variance_from_moments(img["shade"], img["shade_sq"], 16)
    torch.cuda.synchronize()
    return img


def settings(sigma_position):
    d = mp.TemporalAccumulator((W, H), 0).settings
    return tp.TemporalSettings(C.sizeof(tp.TemporalSettings), W, H, 0, sigma_position, d.normal_min, d.max_history, d.alpha_color,
                               d.alpha_moments, d.min_variance_history)


def render_ms(scene, cam, spp):
    fr = mp.FrameRenderer(scene, cam, mp.RenderSettings(64, spp, (W, H), seed=1))
    for _ in range(3):
        fr.render()
    torch.cuda.synchronize()
    ms = []
    for _ in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fr.render()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def main():
    detail = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    ctx = mp.Context(0)
    scene = mp.Scene(mp.TriangleBvh.build(*scenes.atrium(1, detail), ctx=ctx))
    eye, at, fnum = scenes.ATRIUM_VIEW
    cams = [scenes.atrium_camera(),
            mp.Camera.default().look_at((eye[0], eye[1], eye[2] + 0.05), (at[0], at[1], at[2] + 0.3), (0.0, 1.0, 0.0)).f_number(fnum)]
    f0, f1 = frame_planes(scene, cams[0], 1), frame_planes(scene, cams[1], 2)
    view0 = mp.TemporalAccumulator.view_of(cams[0], (W, H))
    hist, mom = torch.empty_like(f0["shade"]), torch.empty_like(f0["shade"])
    tp.check(tp.lib().mpt_reset(0, W, H, f0["shade"].data_ptr(), f0["position"].data_ptr(), hist.data_ptr(), mom.data_ptr(), None))
    out, mout, vout = (torch.empty_like(hist) for _ in range(3))
    cases = {"atrium": (f1, settings(mp.TemporalAccumulator((W, H), 0).settings.sigma_position)), "kept": (f0, settings(float("inf")))}
    st_kept = cases["kept"][1]
    st_kept.normal_min = -1e30  # nothing is turned away either

    def call(name, variance):
        cur, st = cases[name]
        tp.check(tp.lib().mpt_reproject(0, C.byref(st), C.byref(view0), cur["shade"].data_ptr(), cur["position"].data_ptr(),
                                        cur["normal"].data_ptr(), cur["ids"].data_ptr(), cur["variance"].data_ptr() if variance else None,
                                        f0["position"].data_ptr(), f0["normal"].data_ptr(), f0["ids"].data_ptr(), hist.data_ptr(),
                                        mom.data_ptr(), out.data_ptr(), mout.data_ptr(), vout.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    runs = [(n, v) for n in cases for v in (False, True)]
    stats = {}
    for r in runs:  # warm-up, and what each run does
        call(*r)
        call(*r)
        torch.cuda.synchronize()
        N = mout[..., 2]
        stats[r] = (float((N > 0).float().mean()), float((N > 1).float().mean()), tp.last_kernels())
    ms = np.zeros((ROUNDS, len(runs)))
    for rnd in range(ROUNDS):
        for i, r in enumerate(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPS):
                call(*r)
            b.record()
            torch.cuda.synchronize()
            ms[rnd, i] = a.elapsed_time(b) / REPS
    frames = {spp: render_ms(scene, cams[1], spp) for spp in (1, 16)}
    for spp, (med, lo, hi) in frames.items():
        print(f"frame {spp:2d} spp  {med:8.3f} ms  (min {lo:.3f} max {hi:.3f})")
    for i, (name, variance) in enumerate(runs):
        t = ms[:, i]
        med = float(np.median(t))
        floor = W * H * 16 * PLANES[variance] / (COPY_GBS * 1e9) * 1e3
        hits, with_history, kernels = stats[(name, variance)]
        print(f"{name:6s} {'variance_in' if variance else 'plain      '}  {med * 1e3:7.1f} us  (min {t.min() * 1e3:.1f} max {t.max() * 1e3:.1f})  "
              f"floor {floor * 1e3:5.1f} us  ratio {med / floor:5.2f}  of the 1-spp frame {med / frames[1][0]:.4f}  of the 16-spp frame "
              f"{med / frames[16][0]:.4f}  hit pixels {hits:.3f}  with history {with_history:.3f}  kernels {kernels}")
    sys.stdout.flush()


if __name__ == "__main__":
    main()
