#!/usr/bin/env python3
"""The CPU sweep behind GuidedResampler's default weights: on the end-to-end case of tests/resample_cases.py (the teapot at 48 x 32,
8-sample ambient occlusion traced at 24 x 16 over the oracle) the numpy model's upsampled plane (tests/resample_model.py) is compared
with the oracle's 64-sample ambient occlusion at full resolution, for every k = sigma_normal_pow2 in 0..8 and a ladder of
sigma_plane, over all four phases of the picks.  Prints the mean absolute error at the hit pixels per setting, the error of
replicating each block's pick over the block, and the error of the 8-sample plane at full resolution (four times the rays).
No GPU is used.  usage: sweep_resample.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from oracle import pyoracle as po
from tests import resample_cases as tc, resample_model as rm, secondary_model as sm

TEAPOT = os.path.join(ROOT, "tests", "golden", "teapot.obj")
SIGMAS = [0.001, 0.002, 0.005, 0.01, 0.02, 0.05, 0.1, float("inf")]


def main():
    c, fr = tc.E2E, tc.e2e_frame(po, TEAPOT)
    ref = tc.e2e_reference(po, TEAPOT)
    hit = fr["planes"]["position"][..., 3] > 0

    def mae(a):
        return float(np.abs(a[..., 0][hit].astype(np.float64) - ref[..., 0][hit]).mean())

    full, _ = sm.run(po, fr["bvh"].occluded, fr["planes"]["position"], fr["planes"]["normal"], sm.MODE_AO, c["ao_seed"], c["samples"], c["batch"],
                     fr["eye"], radius=c["radius"], bias=c["bias"])
    print(f"hit pixels {int(hit.sum())};  8 samples at full resolution: {mae(full):.5f}")
    phases = range(c["factor"] ** 2)
    lows = [tc.e2e_low(po, TEAPOT, ph) for ph in phases]
    rep = [mae(rm.replicate(lo["picks"], lo["ao_lo"], fr["planes"]["position"], c["factor"])) for lo in lows]
    print("replicated picks, per phase: " + " ".join(f"{e:.5f}" for e in rep) + f"  mean {np.mean(rep):.5f}")
    print("mean absolute error of the upsampled plane, mean over the phases (rows k, columns sigma_plane)")
    print("k \\ sp " + " ".join(f"{s:8g}" for s in SIGMAS))
    best = None
    for k in range(9):
        row = []
        for s in SIGMAS:
            e = float(np.mean([mae(tc.e2e_up(po, TEAPOT, ph, k, s)[0]) for ph in phases]))
            row.append(e)
            if best is None or e < best[0]:
                best = (e, k, s)
        print(f"{k:6d} " + " ".join(f"{e:8.5f}" for e in row))
    print(f"best: k = {best[1]}, sigma_plane = {best[2]}: {best[0]:.5f}")


if __name__ == "__main__":
    main()
