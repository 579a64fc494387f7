#!/usr/bin/env python3
"""Throughput of the three ray queries -- closest hit (mp_trace_rays), bounded closest hit (mp_trace_rays_bounded) and occlusion
(mp_occluded_rays) -- on two ray sets, on the atrium stand-in and on the teapot:
  shadow:  pinhole camera rays' first hits, offset 1e-4 along the normal (to the ray's side), aimed at a point light inside the
           scene, tmax = distance * (1 - 1e-4);  closest = the same rays unbounded;
  bounce:  incoherent bounce-like rays as in tools/bench_trace.py (surface points of random interior rays, uniformly random
           directions), with tmax = 2.0 for the bounded and occlusion queries.
Prints one line per (scene, ray set, query): Mrays/s and ms per call (median of the timed calls).  Diagnostics only.
usage: bench_query.py [N_RAYS] [ATRIUM_DETAIL]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from minipath_amd import scenes
from minipath_amd.camera import Camera
from minipath_amd.scene import Context, TriangleBvh

TEAPOT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "teapot.obj")


def camera_rays(cam, w, h, dev):
    c, f, u, r = [torch.from_numpy(x).to(dev) for x in cam.center_forward_up_right()]
    ys, xs = torch.meshgrid(torch.linspace(0.6, -0.6, h, device=dev), torch.linspace(-1.0, 1.0, w, device=dev), indexing="ij")
    d = f[None] + xs.reshape(-1, 1) * r[None] * 0.9 + ys.reshape(-1, 1) * u[None] * 0.9
    d = torch.nn.functional.normalize(d, dim=1)
    return c.expand_as(d).contiguous(), d.contiguous()


def shadow_rays(bvh, cam, light, n, dev):
    w = int(np.sqrt(n * 16 / 9))
    o, d = camera_rays(cam, w, max(1, n // w), dev)
    h = bvh.intersect(o, d, full=True)
    hit = h["prim"] != -1
    p, nrm = h["point"][hit], h["normal"][hit]
    nrm = torch.where(((nrm * d[hit]).sum(1, keepdim=True) > 0), -nrm, nrm)  # towards the camera side
    p = p + 1e-4 * nrm
    to_l = light[None] - p
    dist = to_l.norm(dim=1)
    return p.contiguous(), (to_l / dist[:, None]).contiguous(), (dist * (1 - 1e-4)).contiguous()


def bounce_rays(bvh, lo, hi, n, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    lo, hi = torch.tensor(lo, device=dev), torch.tensor(hi, device=dev)
    o = lo + (hi - lo) * torch.rand((n, 3), device=dev, generator=g)
    d = torch.nn.functional.normalize(torch.randn((n, 3), device=dev, generator=g), dim=1)
    h = bvh.intersect(o, d)
    hit = h["prim"] != -1
    o2 = (o + d * h["t"][:, None])[hit]
    d2 = torch.nn.functional.normalize(torch.randn((o2.shape[0], 3), device=dev, generator=g), dim=1)
    o2 = o2 + 1e-3 * d2
    return o2.contiguous(), d2.contiguous(), torch.full((o2.shape[0],), 2.0, device=dev)


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
    detail = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    dev = torch.device("cuda:0")
    ctx = Context(0)
    cases = [
        ("atrium", TriangleBvh.build(*scenes.atrium(1, detail), ctx=ctx), scenes.atrium_camera(),
         torch.tensor([0.0, 9.0, 0.0], device=dev), ([-17.0, 0.5, -10.0], [17.0, 13.0, 10.0])),
        ("teapot", TriangleBvh.with_obj(TEAPOT, ctx), Camera.teapot_view(), torch.tensor([2.0, 5.0, 4.0], device=dev),
         ([-3.0, 0.0, -2.0], [3.0, 3.0, 2.0])),
    ]
    for name, bvh, cam, light, (lo, hi) in cases:
        sets = {"shadow": shadow_rays(bvh, cam, light, n, dev), "bounce": bounce_rays(bvh, lo, hi, n, dev)}
        for sname, (o, d, tm) in sets.items():
            m = o.shape[0]
            occ = bvh.occluded(o, d, tmax=tm)
            frac = float(occ.float().mean())
            res = {
                "closest": timed(lambda: bvh.intersect(o, d)),
                "bounded": timed(lambda: bvh.intersect(o, d, tmax=tm)),
                "occluded": timed(lambda: bvh.occluded(o, d, tmax=tm)),
            }
            for q, dt in res.items():
                print(f"{name:7s} {sname:7s} {q:9s} {m / dt / 1e6:8.0f} Mrays/s {dt * 1e3:8.2f} ms  ({m} rays, {frac:.3f} occluded)")
            sys.stdout.flush()


if __name__ == "__main__":
    main()
