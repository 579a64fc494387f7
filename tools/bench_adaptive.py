#!/usr/bin/env python3
"""Cost of adaptive sampling (minipath_amd.AdaptiveSampler, include/minipath_adaptive.h) at 1920x1080, tile 64 (510 slots).

1. kernels -- mpa_tile_error, mpa_move_tiles (all 510 slots) and mpa_finish_tiles (every slot scaled) on synthetic planes: device
   time between two events around REPS back-to-back calls, the three alternating inside every round, median / min / max over
   ROUNDS rounds.  Every call of a run works on another of SETS plane sets (SETS * 67 MB, more than the 256 MB Infinity Cache), so
   the bytes come from HBM.  Bytes = what the operation must read once and write once: tile_error 2 x 16 B per owned pixel (it
   loads the whole pixel, .x is used), move 16 B in + 16 B out per slot pixel, finish 16 B in + 16 B out per owned pixel; against
   bench.py's HBM_PEAK_GBS (8 TB/s spec; a float4 copy reaches 79 % of it).
2. bookkeeping -- on SCENE at BUDGET spp, host clock around work that ends in a device synchronise, the three alternating inside every
   round: "adaptive" = AdaptiveSampler at threshold -1 (nothing stops: every round renders all tiles in place, checks them and reads
   the result back), "split" = the same rounds as plain render_aov_pass calls and one synchronise, "single" = one launch.
   adaptive - split is the price of the checks and the per-round synchronisations.
3. adaptive against fixed -- render() at THRESHOLDS under each of SCHEDULES: time (as in 2) and mean samples per pixel, on the teapot
   and on SCENE.
`trace` as the first argument: only three adaptive frames at threshold -1 on SCENE, for a kernel trace of the bookkeeping
(rocprofv3 --kernel-trace --stats -- python tools/bench_adaptive.py trace).

Diagnostics only.  usage: bench_adaptive.py [ATRIUM_DETAIL]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import minipath_amd as mp
from bench import HBM_PEAK_GBS
from minipath_amd import adaptive as ad
from minipath_amd import scenes

W, H, TS, BUDGET = 1920, 1080, 64, 256
REPS, ROUNDS, SETS = 8, 9, 8
FRAME_ROUNDS = 5
THRESHOLDS = (0.1, 0.05, 0.02)
MIN_SAMPLES = ROUND_SAMPLES = 16
SCHEDULES = ((16, 16), (32, 64))  # (min_samples, round_samples) of part 3: 16 rounds, and 5 (a pass has a fixed cost of its own)
TEAPOT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "teapot.obj")


def stats(v):
    return f"{np.median(v):9.3f}  (min {np.min(v):.3f} max {np.max(v):.3f})"


def kernels():
    tiles = mp.tile_ordering(mp.ScreenBlock(0, 0, W, H), TS)
    n = len(tiles)
    wh = torch.tensor([[t.width(), t.height()] for t in tiles], dtype=torch.int32, device="cuda")
    owned = sum(t.area() for t in tiles)
    gen = torch.Generator("cuda").manual_seed(1)
    sets = []
    for _ in range(SETS):
        shade = torch.rand((n, TS, TS, 4), device="cuda", generator=gen) * 16
        sq = shade * torch.rand((n, TS, TS, 4), device="cuda", generator=gen)
        sets.append((shade, sq))
    d_open = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_err = torch.zeros(n, dtype=torch.float32, device="cuda")
    k_mid = torch.full((n,), 16, dtype=torch.int32, device="cuda")
    L, stream = ad.lib(), torch.cuda.current_stream().cuda_stream

    def tile_error(i):
        s, q = sets[i % SETS]
        ad.check(L.mpa_tile_error(0, TS, n, 16, 0.05, 0.05, s.data_ptr(), q.data_ptr(), wh.data_ptr(), d_open.data_ptr(), d_err.data_ptr(), stream))

    def move(i):
        s, q = sets[i % SETS]
        ad.check(L.mpa_move_tiles(0, TS, n, s.data_ptr(), n, None, q.data_ptr(), n, None, stream))

    def finish(i):
        s, _ = sets[i % SETS]
        ad.check(L.mpa_finish_tiles(0, TS, n, BUDGET, s.data_ptr(), k_mid.data_ptr(), wh.data_ptr(), stream))

    # tile_error first in every round: move and finish change the planes (which costs tile_error nothing: it has no data-dependent path)
    ops = (("mpa_tile_error", tile_error, owned * 32), ("mpa_move_tiles", move, n * TS * TS * 32), ("mpa_finish_tiles", finish, owned * 32))
    for _, fn, _ in ops:
        fn(0)
    torch.cuda.synchronize()
    us = {name: [] for name, _, _ in ops}
    for _ in range(ROUNDS):
        for name, fn, _ in ops:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(REPS):
                fn(i)
            b.record()
            torch.cuda.synchronize()
            us[name].append(a.elapsed_time(b) / REPS * 1e3)
    print(f"kernels  {W}x{H} tile {TS}: {n} slots, {owned} owned pixels; us per call, median of {ROUNDS} rounds of {REPS} calls")
    for name, _, nbytes in ops:
        med = float(np.median(us[name]))
        gbs = nbytes / (med * 1e-6) / 1e9
        print(f"kernels  {name:17s} {stats(us[name])} us  {nbytes / 1e6:6.1f} MB  {gbs:7.0f} GB/s  {gbs / HBM_PEAK_GBS:5.2f} of the {HBM_PEAK_GBS:.0f} GB/s peak")
    sys.stdout.flush()


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def frames(name, scene, cam):
    st = mp.RenderSettings(TS, BUDGET, (W, H), seed=1)
    fr = mp.FrameRenderer(scene, cam, st)
    bounds = ad.round_bounds(BUDGET, MIN_SAMPLES, ROUND_SAMPLES)
    pixels = W * H

    def planes():
        return fr.new_aov_planes(shade=True, normal=False, albedo=False, ids=False, shade_sq=True)

    def single():
        pl = planes()
        return timed(lambda: fr.render_aov_pass(pl))[0]

    def split():
        pl = planes()

        def run():
            for b0, b1 in zip(bounds, bounds[1:]):
                fr.render_aov_pass(pl, b0, b1 - b0)
        return timed(run)[0]

    def adaptive(threshold, schedule=(MIN_SAMPLES, ROUND_SAMPLES)):
        s = mp.AdaptiveSampler(scene, cam, st, threshold, min_samples=schedule[0], round_samples=schedule[1])
        ms = timed(s.render)[0]
        return ms, s.samples_drawn / pixels, s.round

    runs = [("single", single), ("split", split), ("adaptive -1", lambda: adaptive(-1.0)[0])]
    for _, fn in runs:  # warm-up: code objects, tile lists, allocator
        fn()
    ms = {k: [] for k, _ in runs}
    for _ in range(FRAME_ROUNDS):
        for k, fn in runs:
            ms[k].append(fn())
    print(f"frames   {name}: {W}x{H} tile {TS}, budget {BUDGET} spp, {len(bounds) - 1} rounds of {ROUND_SAMPLES}; ms, median of {FRAME_ROUNDS} alternating rounds")
    for k, _ in runs:
        print(f"frames   {name} {k:12s} {stats(ms[k])} ms")
    over = np.array(ms["adaptive -1"]) - np.array(ms["split"])
    print(f"frames   {name} bookkeeping = adaptive -1 - split: {stats(over)} ms = {100 * np.median(over) / np.median(ms['split']):.2f} % of split; "
          f"split - single: {np.median(ms['split']) - np.median(ms['single']):.3f} ms")
    for schedule in SCHEDULES:
        for thr in THRESHOLDS:
            adaptive(thr, schedule)
            res = [adaptive(thr, schedule) for _ in range(3)]
            t = [r[0] for r in res]
            print(f"frames   {name} min/round {schedule[0]:3d}/{schedule[1]:3d} threshold {thr:5.2f}  {stats(t)} ms  mean spp {res[0][1]:7.2f} of "
                  f"{BUDGET}  rounds {res[0][2]:2d}  time / single {np.median(t) / np.median(ms['single']):.3f}")
    sys.stdout.flush()


def main():
    args = sys.argv[1:]
    ctx = mp.Context(0)
    if args and args[0] == "trace":
        scene, cam = mp.Scene(mp.TriangleBvh.build(*scenes.atrium(1, 1.0), ctx=ctx)), scenes.atrium_camera()
        for _ in range(3):
            s = mp.AdaptiveSampler(scene, cam, mp.RenderSettings(TS, BUDGET, (W, H), seed=1), -1.0, min_samples=MIN_SAMPLES,
                                   round_samples=ROUND_SAMPLES)
            print("adaptive -1: %.3f ms" % timed(s.render)[0])
        return
    detail = float(args[0]) if args else 1.0
    kernels()
    frames("teapot", mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, ctx)), mp.Camera.teapot_view())
    frames("atrium", mp.Scene(mp.TriangleBvh.build(*scenes.atrium(1, detail), ctx=ctx)), scenes.atrium_camera())


if __name__ == "__main__":
    main()
