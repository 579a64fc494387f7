#!/usr/bin/env python3
"""Device time of the lights (mpl_generate, mpl_resolve, include/minipath_lights.h) at 1920x1080 against their traffic floors, the
whole irradiance frame with its shares, and the same frame done with torch ops and TriangleBvh.occluded.

Planes: the renderer's own untiled "position" and "normal" planes at one sample per pixel of the atrium stand-in and of the teapot.
T = device time between two events around REPS back-to-back calls; the runs of one table alternate inside every round, median / min
/ max over ROUNDS rounds (the protocol of tools/bench_secondary.py).  Floor = the bytes the definition must move / the rate a copy
reaches on this machine (COPY_GBS): generate reads 32 B per pixel and writes 32 B per ray, resolve reads 9 B per ray
and writes 16 B per pixel for the sums and 16 B for out.  L = 1, 4 and 8 lights, B = 2 samples per batch.
  kernels  light_rays_kernel<true> (sphere lights) at each L, light_rays_kernel<false> (the same lights as points) at L = 4, and
           irradiance_kernel<true> at each L
  frame    LocalLights.irradiance at 4 samples in batches of 2 at each L, and its three stages timed one by one on the rays of the
           first batch: the share of the query against the two new kernels
  torch    the same samples per hit pixel and light generated with torch ops (uniform points of the light's disc across the line to
           the surface, torch's own RNG), traced with TriangleBvh.occluded ([n, 3] tensors and a tmax per ray) and summed with
           torch: the route a user had
Prints one line per run.  Diagnostics only.
usage: bench_lights.py [ATRIUM_DETAIL]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import minipath_amd as mp
from minipath_amd import _lib as hip
from minipath_amd import lights as ll
from minipath_amd import scenes

W, H = 1920, 1080
REPS, ROUNDS = 10, 7
COPY_GBS = 6290.0
SAMPLES, BATCH = 4, 2
COUNTS = (1, 4, 8)
TEAPOT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "teapot.obj")
# eight lamps each: hung along the nave of the hall; around and above the teapot
ATRIUM_LAMPS = [((x, y, z), 0.3, (60.0, 54.0, 45.0)) for x, y, z in ((-10, 8, 0), (0, 9, 2), (10, 8, -2), (-5, 6, -6), (5, 6, 6), (-14, 5, 3), (14, 7, 0),
                                                                     (0, 12, 0))]
TEAPOT_LAMPS = [((x, y, z), 0.5, (30.0, 28.0, 24.0)) for x, y, z in ((-6, 1, 3), (-4, 3, 2), (6, 2, 3), (0, 7, 2), (3, 4, -5), (-3, 5, 5), (0, 1, 7),
                                                                     (7, 6, 0))]


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


def torch_irradiance(bvh, position, normal, eye, lamps, samples, batch, bias, margin, gen):
    """the frame's work with torch ops: {E.r, E.g, E.b} summed per pixel, and the count"""
    A = position[..., 3].reshape(-1)
    hit = A > 0
    P = position[..., :3].reshape(-1, 3) / A[:, None]
    N = normal[..., :3].reshape(-1, 3)
    n = N / torch.linalg.norm(N, dim=-1, keepdim=True)
    hit = hit & torch.isfinite(n).all(-1)
    n = torch.where(((P - eye) * n).sum(-1, keepdim=True) > 0, -n, n)
    o = torch.where(hit[:, None], P + n * bias, torch.zeros_like(P))
    E = torch.zeros_like(P)
    for begin in range(0, samples, batch):
        b = min(batch, samples - begin)
        os_, ds, tms, wts = [], [], [], []
        for c, R, _ in lamps:
            c = torch.tensor(c, device=A.device)
            w = c - o
            q = torch.linalg.norm(w, dim=-1, keepdim=True)
            m = w / q
            sg = torch.copysign(torch.ones_like(m[:, 2]), m[:, 2])
            a = -1.0 / (sg + m[:, 2])
            bb = m[:, 0] * m[:, 1] * a
            t = torch.stack([1.0 + sg * m[:, 0] * m[:, 0] * a, sg * bb, -sg * m[:, 0]], -1)
            bt = torch.stack([bb, sg + m[:, 1] * m[:, 1] * a, -m[:, 1]], -1)
            r = torch.sqrt(torch.rand((b, A.numel()), device=A.device, generator=gen)) * R
            phi = torch.rand((b, A.numel()), device=A.device, generator=gen) * (2 * np.pi)
            g = c + t[None] * (r * torch.cos(phi))[..., None] + bt[None] * (r * torch.sin(phi))[..., None]
            d = g - o[None]
            dist = torch.linalg.norm(d, dim=-1)
            nd = (d * n[None]).sum(-1)
            lit = hit[None] & (q[None, :, 0] > R) & (nd > 0) & (dist - margin > 0)
            os_.append(torch.where(lit[..., None], o[None].expand(b, -1, -1), torch.zeros_like(d)))
            ds.append(torch.where(lit[..., None], d, torch.zeros_like(d)))
            tms.append(torch.where(lit, dist - margin, torch.full_like(dist, -1.0)))
            wts.append(torch.where(lit, nd / (dist * dist * dist), torch.zeros_like(dist)))
        tm = torch.stack(tms, 1)  # [b, L, pixels], as the library's buffers
        occ = bvh.occluded(torch.stack(os_, 1).reshape(-1, 3), torch.stack(ds, 1).reshape(-1, 3), tmax=tm.reshape(-1)).reshape(tm.shape)
        seen = ((tm > 0) & ~occ).to(A.dtype) * torch.stack(wts, 1)
        inten = torch.tensor([it for _, _, it in lamps], device=A.device)  # [L, 3]
        E += torch.einsum("blp,lc->pc", seen, inten)
    return E, hit.to(A.dtype) * samples


def bench_scene(name, bvh, cam, lamps8, margin):
    scene = mp.Scene(bvh)
    img = frame_planes(scene, cam)
    position, normal = img["position"], img["normal"]
    pixels = W * H
    hits = float((position[..., 3] > 0).float().mean())
    eye = mp.LocalLights.eye_of(cam)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print(f"---- {name}: {W}x{H}, hit pixels {hits:.3f}, B = {BATCH}, margin {margin}")
    lights = mp.LocalLights(scene, (W, H), batch=BATCH)
    b = lights.buffers(max(COUNTS))
    rays = [b[k].data_ptr() for k in ll.RAY_ARRAYS]
    b["occluded"].random_(0, 2)  # resolve's time does not depend on the answers; something defined
    ctx = bvh.ctx
    # ---- the kernels against their floors
    runs, floors, stage = {}, {}, {}
    for L in COUNTS:
        tables = {"spheres": ll.light_table(lamps8[:L])}
        if L == 4:
            tables["points"] = ll.light_table([(c, 0.0, it) for c, _, it in lamps8[:L]])
        st = lights.batch_settings(SAMPLES, 0, BATCH, L, 7, eye, 1e-4, margin)
        for tag, table in tables.items():
            def gen(st=st, table=table):
                ll.check(ll.lib().mpl_generate(0, C.byref(st), table, position.data_ptr(), normal.data_ptr(), *rays, stream))
            runs[f"generate {tag} L={L}"] = gen
            floors[f"generate {tag} L={L}"] = pixels * (32 + 32 * BATCH * L) / (COPY_GBS * 1e9) * 1e3

        def res(st=st, table=tables["spheres"]):
            ll.check(ll.lib().mpl_resolve(0, C.byref(st), table, b["tmax"].data_ptr(), b["weight"].data_ptr(), b["occluded"].data_ptr(),
                                          b["sums"].data_ptr(), b["out"].data_ptr(), stream))
        runs[f"resolve L={L}"] = res
        floors[f"resolve L={L}"] = pixels * (9 * BATCH * L + 32) / (COPY_GBS * 1e9) * 1e3

        def query(L=L):
            hip.check(hip.lib().mp_occluded_rays(ctx.handle, bvh.handle, *rays[:7], pixels * BATCH * L, b["occluded"].data_ptr(), stream))
        stage[L] = (runs[f"generate spheres L={L}"], query, res)
    ms = timed(runs)
    for k in runs:
        line(k, ms[k], floors[k])
    # ---- the frame, its stages (on the rays of the first batch) and the torch route, one table of runs per L
    gen_t = torch.Generator(device="cuda")
    gen_t.manual_seed(7)
    eye_t = torch.tensor(eye, device="cuda")
    for L in COUNTS:
        lamps = lamps8[:L]
        g, q, r = stage[L]
        g()  # the rays the query is timed on
        frame_runs = {
            f"frame irradiance L={L} {SAMPLES} ({BATCH}+{BATCH})": lambda: lights.irradiance(position, normal, eye, lamps, SAMPLES, seed=7, margin=margin),
            f"stage generate L={L}": g,
            f"stage mp_occluded_rays L={L}": q,
            f"stage resolve L={L}": r,
            f"torch route L={L} {SAMPLES} ({BATCH}+{BATCH})": lambda: torch_irradiance(bvh, position, normal, eye_t, lamps, SAMPLES, BATCH, 1e-4, margin, gen_t),
        }
        ms = timed(frame_runs)
        med = [line(k, ms[k]) for k in frame_runs]
        tg, tq, tr = med[1:4]
        out, sums = lights.irradiance(position, normal, eye, lamps, SAMPLES, seed=7, margin=margin)
        lib_mean = float(out[..., :3][sums[..., 3] > 0].mean())
        E, cnt = torch_irradiance(bvh, position, normal, eye_t, lamps, SAMPLES, BATCH, 1e-4, margin, gen_t)
        torch.cuda.synchronize()
        print(f"L={L}: shares of a batch: generate {tg / (tg + tq + tr):.3f}  query {tq / (tg + tq + tr):.3f}  resolve {tr / (tg + tq + tr):.3f};  "
              f"torch route / frame {med[4] / med[0]:.2f};  mean irradiance at hits: library {lib_mean:.5f}  torch route "
              f"{float((E[cnt > 0] / SAMPLES).mean()):.5f}")
        sys.stdout.flush()


def main():
    detail = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    ctx = mp.Context(0)
    bench_scene("atrium", mp.TriangleBvh.build(*scenes.atrium(1, detail), ctx=ctx), scenes.atrium_camera(), ATRIUM_LAMPS, 0.35)
    bench_scene("teapot", mp.TriangleBvh.with_obj(TEAPOT, ctx), mp.Camera.teapot_view(), TEAPOT_LAMPS, 0.0)


if __name__ == "__main__":
    main()
