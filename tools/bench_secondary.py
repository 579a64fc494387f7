#!/usr/bin/env python3
"""Device time of the secondary rays (mps_generate, mps_resolve, include/minipath_secondary.h) at 1920x1080 against their traffic
floors, the whole ambient-occlusion frame with its shares, the same frame done with torch ops and TriangleBvh.occluded, and the
occlusion query's rate on sample-major against pixel-major rays.

Planes: the renderer's own untiled "position" and "normal" planes at one sample per pixel of the atrium stand-in and of the teapot.
T = device time between two events around REPS back-to-back calls; the runs of one table alternate inside every round, median / min
/ max over ROUNDS rounds.  Floor = the bytes the definition must move / the rate a copy reaches on this machine (COPY_GBS, DESIGN.md
4.9): generate reads 32 B per pixel and writes 28 B per ray, resolve reads 5 B per ray and writes 16 B per pixel for the counts and
16 B for out.
  kernels  secondary_rays_kernel<0>, <1> (the hard sun of the frame's key light) and resolve_kernel<true> at B = 4 and 8
  frame    SecondaryVisibility.ambient_occlusion at 8 samples in batches of 4, and its three stages timed one by one on the rays of
           the first batch: the share of the query against the two new kernels
  torch    the same 8 samples per hit pixel generated with torch ops (cosine directions about the turned normal, torch's own RNG),
           traced with TriangleBvh.occluded ([n, 3] tensors, which it transposes) and summed with torch: the route a user had
  order    mp_occluded_rays on the first batch's rays as they are (sample-major) and permuted with torch to pixel-major
Prints one line per run.  Diagnostics only.
usage: bench_secondary.py [ATRIUM_DETAIL]"""
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

W, H = 1920, 1080
REPS, ROUNDS = 20, 9
COPY_GBS = 6290.0
SAMPLES = 8
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
    s = f"{name:34s} {med * 1e3:9.1f} us  (min {t.min() * 1e3:.1f} max {t.max() * 1e3:.1f})"
    if floor_ms is not None:
        s += f"  floor {floor_ms * 1e3:6.1f} us  ratio {med / floor_ms:5.2f}"
    print(s + ("  " + extra if extra else ""))
    return med


def torch_ao(bvh, position, normal, eye, samples, batch, radius, bias, gen):
    """the frame's work with torch ops: {visible, counted} per pixel"""
    A = position[..., 3].reshape(-1)
    hit = A > 0
    P = position[..., :3].reshape(-1, 3) / A[:, None]
    N = normal[..., :3].reshape(-1, 3)
    n = N / torch.linalg.norm(N, dim=-1, keepdim=True)
    hit = hit & torch.isfinite(n).all(-1)
    n = torch.where(((P - eye) * n).sum(-1, keepdim=True) > 0, -n, n)
    sg = torch.copysign(torch.ones_like(n[:, 2]), n[:, 2])
    a = -1.0 / (sg + n[:, 2])
    bb = n[:, 0] * n[:, 1] * a
    t = torch.stack([1.0 + sg * n[:, 0] * n[:, 0] * a, sg * bb, -sg * n[:, 0]], -1)
    bt = torch.stack([bb, sg + n[:, 1] * n[:, 1] * a, -n[:, 1]], -1)
    o = torch.where(hit[:, None], P + n * bias, torch.zeros_like(P))
    tmax = torch.where(hit, torch.full_like(A, radius), torch.zeros_like(A))
    visible = torch.zeros_like(A)
    for begin in range(0, samples, batch):
        b = min(batch, samples - begin)
        r = torch.sqrt(torch.rand((b, A.numel()), device=A.device, generator=gen))
        phi = torch.rand((b, A.numel()), device=A.device, generator=gen) * (2 * np.pi)
        u, v = r * torch.cos(phi), r * torch.sin(phi)
        z = torch.sqrt(torch.clamp(1.0 - r * r, min=0.0))
        d = t[None] * u[..., None] + bt[None] * v[..., None] + n[None] * z[..., None]
        d = torch.where(hit[None, :, None], d, torch.zeros_like(d))
        occ = bvh.occluded(o[None].expand(b, -1, -1).reshape(-1, 3), d.reshape(-1, 3), tmax=tmax.repeat(b))
        visible += ((~occ).reshape(b, -1) & hit[None]).sum(0)
    return visible, hit.to(A.dtype) * samples


def bench_scene(name, bvh, cam, radius):
    scene = mp.Scene(bvh)
    img = frame_planes(scene, cam)
    position, normal = img["position"], img["normal"]
    pixels = W * H
    hits = float((position[..., 3] > 0).float().mean())
    eye = mp.SecondaryVisibility.eye_of(cam)
    light = (-0.5, 0.7, 0.5)
    light = tuple((np.array(light) / np.linalg.norm(light)).tolist())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print(f"---- {name}: {W}x{H}, hit pixels {hits:.3f}, radius {radius}")
    # ---- the kernels against their floors
    bufs, runs, floors = {}, {}, {}
    for B in (4, 8):
        vis = mp.SecondaryVisibility(scene, (W, H), batch=B)
        b = vis.buffers()
        bufs[B] = (vis, b)
        rays = [b[k].data_ptr() for k in sv.RAY_ARRAYS]
        for mode, tag in ((sv.MPS_MODE_AO, "ao"), (sv.MPS_MODE_SUN, "sun")):
            st = sv.batch_settings(W, H, mode, SAMPLES, 0, B, 7, eye, light, radius if mode == sv.MPS_MODE_AO else float("inf"), 1e-4, 0.0)

            def gen(st=st, rays=rays):
                sv.check(sv.lib().mps_generate(0, C.byref(st), position.data_ptr(), normal.data_ptr(), *rays, stream))
            runs[f"generate {tag} B={B}"] = gen
            floors[f"generate {tag} B={B}"] = pixels * (32 + 28 * B) / (COPY_GBS * 1e9) * 1e3
        st_ao = sv.batch_settings(W, H, sv.MPS_MODE_AO, SAMPLES, 0, B, 7, eye, light, radius, 1e-4, 0.0)

        def res(st=st_ao, b=b):
            sv.check(sv.lib().mps_resolve(0, C.byref(st), b["tmax"].data_ptr(), b["occluded"].data_ptr(), b["counts"].data_ptr(), b["out"].data_ptr(),
                                          stream))
        runs[f"resolve B={B}"] = res
        floors[f"resolve B={B}"] = pixels * (5 * B + 32) / (COPY_GBS * 1e9) * 1e3
        b["occluded"].random_(0, 2)  # resolve's time does not depend on the answers; something defined
    ms = timed(runs)
    for k in runs:
        line(k, ms[k], floors[k])
    # ---- the frame and its stages (B = 4: two batches)
    vis, b = bufs[4]
    rays = [b[k].data_ptr() for k in sv.RAY_ARRAYS]
    st = sv.batch_settings(W, H, sv.MPS_MODE_AO, SAMPLES, 0, 4, 7, eye, light, radius, 1e-4, 0.0)
    sv.check(sv.lib().mps_generate(0, C.byref(st), position.data_ptr(), normal.data_ptr(), *rays, stream))
    ctx = bvh.ctx

    def query(rays=rays, occ=b["occluded"]):
        hip.check(hip.lib().mp_occluded_rays(ctx.handle, bvh.handle, *rays, pixels * 4, occ.data_ptr(), stream))
    perm = {k: b[k].reshape(4, pixels).t().contiguous().reshape(-1) for k in sv.RAY_ARRAYS}  # pixel-major: ray = p * B + b
    occ2 = torch.empty_like(b["occluded"])
    prays = [perm[k].data_ptr() for k in sv.RAY_ARRAYS]
    gen_t = torch.Generator(device="cuda")
    gen_t.manual_seed(7)
    eye_t = torch.tensor(eye, device="cuda")
    frame_runs = {
        "frame ambient_occlusion 8 (4+4)": lambda: vis.ambient_occlusion(position, normal, eye, SAMPLES, radius, seed=7),
        "stage generate B=4": runs["generate ao B=4"],
        "stage mp_occluded_rays B=4": query,
        "stage resolve B=4": runs["resolve B=4"],
        "query pixel-major B=4": lambda: query(prays, occ2),
        "torch route 8 (4+4)": lambda: torch_ao(bvh, position, normal, eye_t, SAMPLES, 4, radius, 1e-4, gen_t),
    }
    ms = timed(frame_runs)
    med = {k: line(k, ms[k]) for k in frame_runs}
    g, q, r = med["stage generate B=4"], med["stage mp_occluded_rays B=4"], med["stage resolve B=4"]
    print(f"shares of a batch: generate {g / (g + q + r):.3f}  query {q / (g + q + r):.3f}  resolve {r / (g + q + r):.3f};  "
          f"torch route / frame {med['torch route 8 (4+4)'] / med['frame ambient_occlusion 8 (4+4)']:.2f};  "
          f"query pixel-major / sample-major {med['query pixel-major B=4'] / q:.3f}")
    # the permuted rays are the same rays: the answers agree
    query()
    query(prays, occ2)
    torch.cuda.synchronize()
    same = bool(torch.equal(b["occluded"].reshape(4, pixels).t().reshape(-1), occ2))
    out, counts = vis.ambient_occlusion(position, normal, eye, SAMPLES, radius, seed=7)
    tv, tc_ = torch_ao(bvh, position, normal, eye_t, SAMPLES, 4, radius, 1e-4, gen_t)
    torch.cuda.synchronize()
    hit = counts[..., 1] > 0
    print(f"answers of the two orders agree: {same};  mean visibility at hits: library {float(out[..., 0][hit].mean()):.4f}  "
          f"torch route {float((tv.reshape(H, W)[hit] / SAMPLES).mean()):.4f}")
    sys.stdout.flush()


def main():
    detail = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    ctx = mp.Context(0)
    bench_scene("atrium", mp.TriangleBvh.build(*scenes.atrium(1, detail), ctx=ctx), scenes.atrium_camera(), 2.0)
    bench_scene("teapot", mp.TriangleBvh.with_obj(TEAPOT, ctx), mp.Camera.teapot_view(), 1.0)


if __name__ == "__main__":
    main()
