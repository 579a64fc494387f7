#!/usr/bin/env python3
"""What the cached packet walk (packet_walk.h, trace_packet_cached) costs per pass on trees of several widths, counted on the CPU
before any kernel work: the reference tree collapsed to at most LIMIT slots per node (sim_collapse.build_device, policy "area":
the device trees' rule -- 8 = the wide tree, 16 = the packet tree), walked by a numpy model of the cached walk with the unit
bounds of mask_cache_begin_unit (corner rays + 1/64; analytic_bounds.Cache), the per-unit node masks (box_reject) and triangle
masks (sim_tri_reject.interval_reject).  A child is tested when it is popped, with t1 <= min(hi, best.t), for the rays that were
live at its parent's visit; work units are 2 x 2 pixels x 16 samples per pass, rays from the oracle, on the metric's frame
(1920 x 1080).

Per limit: nodes and absorbed reference nodes, the histogram of children per node; per pass: pops, pops culled for every ray,
node visits, leaf visits, surviving triangle tests; per unit: distinct nodes and leaves looked up (= mask slow paths, a bounds
reset counts them again).  Asserts that no rejected child is passed and no rejected triangle is hit by any ray, and that every
ray's best.t is bit-equal across the limits in every pass.

usage: packet_tree_count.py [atrium|teapot] [units] [limits, e.g. 8,16,32] [passes per unit]
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

from analytic_bounds import FLT_MAX, Cache, box_reject, jitter_scale, ray_ok  # noqa: E402
from sim_collapse import RefTree, build_device, load, slab  # noqa: E402
from sim_tri_reject import interval_reject, mt_valid  # noqa: E402

F = np.float32
MARGIN = 1 / 64  # MP_MCACHE_MARGIN


class Counts:
    def __init__(self):
        self.pops = self.culled = self.nodes = self.leaves = self.tris = self.node_fills = self.leaf_fills = 0


def walk_pass(nodes, root, ref, o, d, inv, cache, node_masks, leaf_masks, cnt):
    """one pass of 64 rays through the cached walk's model; returns best.t [64]"""
    neg = inv[0] < 0
    best = np.full(o.shape[0], FLT_MAX, F)
    everyone = np.ones(o.shape[0], bool)
    # a frame: [node, children still to pop (ascending), rays live at the visit]; the root is child 0 of a pseudo-node whose box
    # every ray passes
    frames = [[None, [0], everyone]]
    while frames:
        node, todo, pm = frames[-1]
        if not todo:
            frames.pop()
            continue
        c = todo.pop()  # highest child first
        cnt.pops += 1
        if node is None:
            link, ok = root, pm
        else:
            boxes, links = nodes[node]
            t1, t2 = slab(boxes[c][None, :], o, inv, best)
            ok = (t1[:, 0] <= t2[:, 0]) & pm
            link = int(links[c])
        if not ok.any():
            cnt.culled += 1
            continue
        if link >= 0:
            cnt.nodes += 1
            boxes, links = nodes[link]
            if link not in node_masks:
                cnt.node_fills += 1
                node_masks[link] = ~box_reject(boxes, cache.lo, cache.hi, neg)
            keep = node_masks[link]
            t1, t2 = slab(boxes, o, inv, best)
            passed = ((t1 <= t2) & ok[:, None]).any(0)
            assert not (passed & ~keep).any(), "a rejected child is passed by a ray"
            kids = [int(k) for k in np.nonzero(keep)[0]]
            if kids:
                if not frames[-1][1]:
                    frames.pop()  # the frame it replaces is kept only if it still has children
                frames.append([link, kids, ok])
        else:
            cnt.leaves += 1
            first = -1 - link
            v0, e1, e2 = ref.leaf[first]
            if first not in leaf_masks:
                cnt.leaf_fills += 1
                leaf_masks[first] = ~interval_reject(v0, e1, e2, cache.lo[0], cache.hi[0], cache.lo[2], cache.hi[2])
            keep = leaf_masks[first]
            valid, t = mt_valid(v0, e1, e2, o, d)
            valid &= ok[:, None]
            assert not (valid.any(0) & ~keep).any(), "a rejected triangle is hit by a ray"
            cnt.tris += int(keep.sum())
            best = np.minimum(best, np.where(valid & keep[None, :], t, np.inf).min(axis=1).astype(F))
    return best


def main():
    from minipath_amd import scenes
    from oracle import pyoracle as po

    scene = sys.argv[1] if len(sys.argv) > 1 else "atrium"
    units = int(sys.argv[2]) if len(sys.argv) > 2 else 80
    limits = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "8,16,32").split(",")]
    passes = int(sys.argv[4]) if len(sys.argv) > 4 else 16
    w, h, spp = 1920, 1080, 16 * passes
    if scene == "teapot":
        cam = po.teapot_camera()
    else:
        cam = po.Camera()
        po.lib().mpo_camera_default(C.byref(cam))
        eye, at, fnum = scenes.ATRIUM_VIEW
        po.lib().mpo_camera_look_at(C.byref(cam), po.vec3(*eye), po.vec3(*at), po.vec3(0, 1, 0))
        cam.f_number = fnum
    smp = po.build_sampler(cam, w, h)
    s, js = smp.as_array(), jitter_scale()
    ref = RefTree(*load(scene, 1.0))
    trees = {lim: build_device(ref, "area", lim) for lim in limits}
    cnt = {lim: Counts() for lim in limits}
    rng = np.random.default_rng(11)
    n_pass = generic = 0
    for _ in range(units):
        x0, y0 = 2 * int(rng.integers(0, w // 2)), 2 * int(rng.integers(0, h // 2))
        caches = {lim: Cache(MARGIN, s, js, (x0, x0 + 1, y0, y0 + 1)) for lim in limits}
        masks = {lim: ({}, {}) for lim in limits}
        for p in range(passes):
            o = np.zeros((64, 3), F)
            d = np.zeros((64, 3), F)
            inv = np.zeros((64, 3), F)
            for l in range(64):
                px, py = x0 + (l // 16) % 2, y0 + (l // 16) // 2
                r = po.sample_ray(smp, px, py, po.lib().mpo_sample_key(0x5EED, w, spp, px, py, p * 16 + l % 16))
                o[l] = list(r.o)
                d[l] = list(r.d)
                inv[l] = list(r.inv)
            neg = inv < 0
            if not ray_ok(o, d, inv).all() or not (neg.all(0) | ~neg.any(0)).all():
                generic += 1  # a generic walk: no cache
                continue
            n_pass += 1
            bests = []
            for lim in limits:
                c = caches[lim]
                sets = c.sets
                c.begin_pass(o, d, inv)
                if c.sets != sets:  # the bounds were (re)set: every mask goes
                    masks[lim] = ({}, {})
                nodes, root, _ = trees[lim]
                bests.append(walk_pass(nodes, root, ref, o, d, inv, c, masks[lim][0], masks[lim][1], cnt[lim]))
            for b in bests[1:]:
                assert np.array_equal(b.view(np.uint32), bests[0].view(np.uint32)), "best.t differs between the trees"
    print(f"{scene}: {units} units x {passes} passes of 2x2 pixels x 16 samples; {n_pass} cached passes, {generic} generic")
    print("every ray's best.t bit-equal on all trees in every pass; no rejected child passed, no rejected triangle hit")
    print(f"{'limit':>5s} {'nodes':>6s} {'absorbed':>8s} {'pops/pass':>10s} {'culled/pass':>12s} {'node visits/pass':>17s} {'leaf visits/pass':>17s} "
          f"{'tri tests/pass':>15s} {'nodes/unit':>11s} {'leaves/unit':>12s}")
    for lim in limits:
        nodes, _, absorbed = trees[lim]
        c = cnt[lim]
        print(f"{lim:5d} {len(nodes):6d} {absorbed:8d} {c.pops / n_pass:10.2f} {c.culled / n_pass:12.2f} {c.nodes / n_pass:17.2f} "
              f"{c.leaves / n_pass:17.2f} {c.tris / n_pass:15.2f} {c.node_fills / units:11.1f} {c.leaf_fills / units:12.1f}")
    for lim in limits:
        hist = np.bincount([len(links) for _, links in trees[lim][0]], minlength=lim + 1)
        print(f"children per node, limit {lim}: " + " ".join(f"{k}:{int(v)}" for k, v in enumerate(hist) if v))


if __name__ == "__main__":
    main()
