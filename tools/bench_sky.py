#!/usr/bin/env python3
"""Device time of the sky lighting's reduction (mpe_resolve, include/minipath_sky.h) at 1920x1080 against its traffic floor, against
the visibility reduction it sits beside (mps_resolve on the same buffers), and its share of a whole SkyLight frame.

Planes: the renderer's own untiled "position" and "normal" planes at one sample per pixel of the atrium stand-in and of the teapot;
the rays are those mps_generate (MPS_MODE_AO) makes from them and the answers those of mp_occluded_rays, so the directions that reach
the map are a frame's own.  T = device time between two events around REPS back-to-back calls; the runs alternate inside every round,
median / min / max over ROUNDS rounds (the protocol of tools/bench_secondary.py).  Floor = the bytes the definition must move / the
rate a copy reaches on this machine (COPY_GBS): per pixel B = 8 samples of 17 B read (dx dy dz tmax and the answer)
and 32 B written (sums and out), and the map read once (N * N * 16 B).  Maps: gradient skies of N = 64 and N = 1024.
  kernels  sky_resolve_kernel<true> at each N; resolve_kernel<true> of libminipath_secondary.so on the same tmax and answers, for
           scale (it reads 5 B per ray and writes the same 32 B)
  frame    SkyLight.light at 8 samples in one batch of 8 at each N, and its stages timed one by one: the share of the new kernel
Prints one line per run.  Diagnostics only.
usage: bench_sky.py [ATRIUM_DETAIL]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import minipath_amd as mp
from minipath_amd import _lib as hip
from minipath_amd import scenes
from minipath_amd import secondary as sv
from minipath_amd import sky

W, H = 1920, 1080
REPS, ROUNDS = 10, 7
COPY_GBS = 6290.0
SAMPLES = BATCH = 8
MAPS = (64, 1024)
SKY = dict(zenith=(0.2, 0.4, 1.0), horizon=(1.0, 0.9, 0.8), ground=(0.05, 0.04, 0.03))
TEAPOT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "teapot.obj")


def frame_planes(scene, cam):
    fr = mp.FrameRenderer(scene, cam, mp.RenderSettings(64, 1, (W, H), seed=1))
    pl = fr.new_aov_planes(position=True)
    fr.render_aov_pass(pl)
    img = {k: fr.untile_plane(pl[k]) for k in ("position", "normal")}
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
    s = f"{name:36s} {med * 1e3:9.1f} us  (min {t.min() * 1e3:.1f} max {t.max() * 1e3:.1f})"
    if floor_ms is not None:
        s += f"  floor {floor_ms * 1e3:6.1f} us  ratio {med / floor_ms:5.2f}"
    print(s + ("  " + extra if extra else ""))
    return med


def bench_scene(name, bvh, cam, radius):
    scene = mp.Scene(bvh)
    img = frame_planes(scene, cam)
    position, normal = img["position"], img["normal"]
    pixels = W * H
    eye = mp.SkyLight.eye_of(cam)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    light = mp.SkyLight(scene, (W, H), batch=BATCH)
    b = light.buffers()
    rays = [b[k].data_ptr() for k in sky.RAY_ARRAYS]
    read = [b[k].data_ptr() for k in sky.READ_ARRAYS]
    ctx = bvh.ctx
    ao_st = sv.batch_settings(W, H, sv.MPS_MODE_AO, SAMPLES, 0, BATCH, 7, eye, radius=radius, bias=1e-4)

    def generate():
        sv.check(sv.lib().mps_generate(0, C.byref(ao_st), position.data_ptr(), normal.data_ptr(), *rays, stream))

    def query():
        hip.check(hip.lib().mp_occluded_rays(ctx.handle, bvh.handle, *rays, pixels * BATCH, b["occluded"].data_ptr(), stream))

    def visibility():
        sv.check(sv.lib().mps_resolve(0, C.byref(ao_st), b["tmax"].data_ptr(), b["occluded"].data_ptr(), b["counts"].data_ptr(), b["ao"].data_ptr(), stream))

    generate()
    query()  # the rays and the answers every reduction below is timed on
    torch.cuda.synchronize()
    traced = b["tmax"] > 0
    opened = float((traced & (b["occluded"] == 0)).float().mean())
    print(f"---- {name}: {W}x{H}, B = {BATCH}, radius {radius}: rays traced {float(traced.float().mean()):.3f}, open (looked up) {opened:.3f}")
    envs = {n: mp.gradient_sky(n, device=0, **SKY) for n in MAPS}
    runs, floors = {}, {}
    for n, env in envs.items():
        st = light.batch_settings(SAMPLES, 0, BATCH, n, 1)

        def res(st=st, env=env):
            sky.check(sky.lib().mpe_resolve(0, C.byref(st), env.data_ptr(), *read, b["occluded"].data_ptr(), b["sums"].data_ptr(), b["out"].data_ptr(), stream))
        runs[f"sky_resolve_kernel<true> N={n}"] = res
        floors[f"sky_resolve_kernel<true> N={n}"] = (pixels * (17 * BATCH + 32) + n * n * 16) / (COPY_GBS * 1e9) * 1e3
    runs["resolve_kernel<true> (visibility)"] = visibility
    floors["resolve_kernel<true> (visibility)"] = pixels * (5 * BATCH + 32) / (COPY_GBS * 1e9) * 1e3
    ms = timed(runs)
    med = {k: line(k, ms[k], floors[k]) for k in runs}
    for n in MAPS:
        print(f"N={n}: sky_resolve_kernel<true> / resolve_kernel<true> = {med[f'sky_resolve_kernel<true> N={n}'] / med['resolve_kernel<true> (visibility)']:.2f}")
    # ---- the frame and its stages
    for n, env in envs.items():
        frame_runs = {
            f"frame SkyLight.light N={n} {SAMPLES} (one batch)": lambda env=env: light.light(position, normal, eye, env, SAMPLES, seed=7, radius=radius),
            "stage mps_generate": generate,
            "stage mp_occluded_rays": query,
            f"stage mpe_resolve N={n}": runs[f"sky_resolve_kernel<true> N={n}"],
        }
        ms = timed(frame_runs)
        m4 = [line(k, ms[k]) for k in frame_runs]
        out, sums = light.light(position, normal, eye, env, SAMPLES, seed=7, radius=radius)
        torch.cuda.synchronize()
        hit = sums[..., 3] > 0
        print(f"N={n}: share of the frame: mpe_resolve {m4[3] / m4[0]:.3f}  (generate {m4[1] / m4[0]:.3f}  query {m4[2] / m4[0]:.3f});  "
              f"mean sky radiance at hits {[round(float(out[..., c][hit].mean()), 4) for c in range(3)]}")
        sys.stdout.flush()


def main():
    detail = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    ctx = mp.Context(0)
    bench_scene("atrium", mp.TriangleBvh.build(*scenes.atrium(1, detail), ctx=ctx), scenes.atrium_camera(), 6.0)
    bench_scene("teapot", mp.TriangleBvh.with_obj(TEAPOT, ctx), mp.Camera.teapot_view(), float("inf"))


if __name__ == "__main__":
    main()
