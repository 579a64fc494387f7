#!/usr/bin/env python3
"""How many shaded waves of the packet kernel hold a lane whose shading normal has a zero component?  Counted on the CPU: randomly
picked work units of the metric's frame (1920 x 1080, 256 spp, units of 2 x 2 pixels x 16 samples per pass; unit-pick seed 11), the
first pass of each, rays and hits from the oracle.  A component of the unit normal is +-0 exactly when that component of the
unnormalised normal is (a zero over a positive length keeps its sign; a non-zero quotient this small does not occur in these
scenes), so the oracle's normalised normal answers for the numerators of ray_math.h's unit_normal.  Per wave with a hit: a lane with
a zero component, a lane with a -0 component -- the waves that would fall back if the short normalisation did not admit zeros.

usage: normal_zero_count.py [atrium|teapot] [units]
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import minipath_amd as mp
    from minipath_amd import scenes
    from oracle import pyoracle as po

    scene = sys.argv[1] if len(sys.argv) > 1 else "atrium"
    units = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    res, spp, seed = (1920, 1080), 256, 0x5EED
    if scene == "teapot":
        orc, cam = po.Bvh.from_obj(os.path.join(ROOT, "tests", "golden", "teapot.obj")), mp.Camera.teapot_view()
    else:
        orc, cam = po.Bvh.build(*scenes.atrium(1, 1.0)), scenes.atrium_camera()
    smp = po.sampler_from_array(cam.build_sampler(res).as_array())
    L = po.lib()
    rng = np.random.default_rng(11)
    shaded = with_zero = with_neg_zero = all_lanes_zero = 0
    lanes = lanes_zero = lanes_neg_zero = 0
    for _ in range(units):
        ux, uy = 2 * int(rng.integers(0, res[0] // 2)), 2 * int(rng.integers(0, res[1] // 2))
        zero, neg = [], []
        for px, py in ((ux, uy), (ux + 1, uy), (ux, uy + 1), (ux + 1, uy + 1)):
            for s in range(16):
                hr = orc.intersect(po.sample_ray(smp, px, py, L.mpo_sample_key(C.c_uint64(seed), res[0], spp, px, py, s)))
                if hr.hit:
                    n = np.array([hr.normal[0], hr.normal[1], hr.normal[2]], np.float32)
                    zero.append(bool((n == 0).any()))
                    neg.append(bool(((n == 0) & np.signbit(n)).any()))
        if zero:
            shaded += 1
            with_zero += any(zero)
            with_neg_zero += any(neg)
            all_lanes_zero += all(zero)
            lanes += len(zero); lanes_zero += sum(zero); lanes_neg_zero += sum(neg)
    print(f"{scene}: {units} units, {shaded} first passes with a hit ({lanes} shaded lanes)")
    print(f"  waves with a lane that has a zero component : {with_zero} ({100.0 * with_zero / max(shaded, 1):.1f} %), every shaded lane: {all_lanes_zero}")
    print(f"  waves with a lane that has a -0 component   : {with_neg_zero} ({100.0 * with_neg_zero / max(shaded, 1):.1f} %)")
    print(f"  lanes with a zero component {lanes_zero} ({100.0 * lanes_zero / max(lanes, 1):.1f} %), with a -0 component {lanes_neg_zero} "
          f"({100.0 * lanes_neg_zero / max(lanes, 1):.1f} %)")


if __name__ == "__main__":
    main()
