#!/usr/bin/env python3
"""Time of the a-trous denoiser (mpd_atrous, minipath_amd.AtrousDenoiser) at 1920x1080, 5 iterations, with and without a variance
plane, pass by pass against each pass's traffic floor.

Planes: "atrium" -- the atrium stand-in's own feature planes (render_aov_pass at 16 spp: shade as the colour, normal + depth,
variance from the moments), the frame a user would filter; "flat" -- one normal, one depth, every pixel a hit and a constant colour,
so that no tap is skipped or cut short: the most arithmetic the kernel can be given.
A pass cannot be launched alone through the ABI (its step is its index), so the time of pass i is T(i + 1 iterations) - T(i
iterations): the calls differ by exactly that launch (the last pass of either writes the output plane).  T = device time between two
events around REPS back-to-back calls; the runs with 1..5 iterations alternate inside every round, median / min / max over ROUNDS
rounds.  The spread of the 5-iteration total is the session's noise, and a difference of two medians carries about twice it.
Floor of a pass = the bytes it must read once and write once / the HBM rate of bench.py's roofline (HBM_PEAK_GBS): colour and
normal + depth in, colour out = 48 B per pixel; with variance 4 B more in (.x) and 16 B more out = 68 B per pixel.
Prints one line per (planes, variance, pass) and one per total.  Diagnostics only.
usage: bench_denoise.py [ATRIUM_DETAIL]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import minipath_amd as mp
from bench import HBM_PEAK_GBS
from minipath_amd import scenes

W, H, ITERATIONS = 1920, 1080, 5
REPS, ROUNDS = 20, 9
BYTES = {False: 16 + 16 + 16, True: 16 + 16 + 4 + 16 + 16}


def atrium_planes(detail):
    ctx = mp.Context(0)
    bvh = mp.TriangleBvh.build(*scenes.atrium(1, detail), ctx=ctx)
    st = mp.RenderSettings(64, 16, (W, H), seed=1)
    fr = mp.FrameRenderer(mp.Scene(bvh), scenes.atrium_camera(), st)
    pl = fr.new_aov_planes(albedo=False, ids=False, shade_sq=True)
    fr.render_aov_pass(pl)
    img = {k: fr.untile_plane(v) for k, v in pl.items()}
    var = mp.AtrousDenoiser((W, H), 0).variance_from_moments(img["shade"], img["shade_sq"], st.sample_count)
    torch.cuda.synchronize()
    return img["shade"], img["normal"], var


def flat_planes():
    color = torch.full((H, W, 4), 0.5, dtype=torch.float32, device="cuda")
    color[..., :3] += 0.1 * torch.rand((H, W, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    color[..., 3] = 1
    nd = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    nd[..., 2], nd[..., 3] = 1, 2
    var = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    var[..., 0] = 0.01
    return color, nd, var


def main():
    detail = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    floor_ms = {v: W * H * b / (HBM_PEAK_GBS * 1e9) * 1e3 for v, b in BYTES.items()}
    for name, (color, nd, var) in (("atrium", atrium_planes(detail)), ("flat", flat_planes())):
        hits = float((color[..., 3] != 0).float().mean())
        for variance in (False, True):
            dns = [mp.AtrousDenoiser((W, H), 0, iterations=n) for n in range(1, ITERATIONS + 1)]
            out, vout = torch.empty_like(color), torch.empty_like(color)

            def call(dn):
                if variance:
                    dn.denoise(color, nd, variance=var, out=out, variance_out=vout)
                else:
                    dn.denoise(color, nd, out=out)
            for dn in dns:  # warm-up: code object, scratch
                call(dn)
                call(dn)
            torch.cuda.synchronize()
            ms = np.zeros((ROUNDS, ITERATIONS))
            for r in range(ROUNDS):
                for i, dn in enumerate(dns):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(REPS):
                        call(dn)
                    b.record()
                    torch.cuda.synchronize()
                    ms[r, i] = a.elapsed_time(b) / REPS
            med = np.median(ms, 0)
            tag = f"{name:6s} {'variance' if variance else 'plain   '}"
            for i in range(ITERATIONS):
                t = med[i] - (med[i - 1] if i else 0.0)
                print(f"{tag} pass {i} step {1 << i:2d}  {t * 1e3:8.1f} us  floor {floor_ms[variance] * 1e3:6.1f} us  ratio {t / floor_ms[variance]:6.2f}")
            tot = ms[:, -1]
            print(f"{tag} total {ITERATIONS} passes {np.median(tot):7.3f} ms  (min {tot.min():.3f} max {tot.max():.3f})  hit pixels {hits:.2f}  "
                  f"kernels {dns[-1].last_kernels()}")
            sys.stdout.flush()


if __name__ == "__main__":
    main()
