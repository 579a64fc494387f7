#!/usr/bin/env python3
"""What building a unit's leaf masks in batches, on demand, would save -- counted on the CPU before anything is built.  A sibling of
tools/tri_exit_count.py: the same numpy restatement of trace_packet_cached (packet_walk.h) over child lists
(tests/unit_list_model.py), the same frame (1920 x 1080, units of 2 x 2 pixels x 16 samples per pass, rays from the oracle, unit
bounds from the corner rays at the shipped margin, unit-pick seed 11), with the walk's marks on empty-mask leaves and a model of the
leaf table (MP_LEAF_ENTRIES tags, slot = first packet & (entries - 1)) kept under two rules at once -- the walk itself, its visits and
its hits do not depend on when a mask is built:

  single  leaf_mask_slow as it is: a visit that misses in the leaf table builds that leaf's mask (triangle j on lane j).
  batch   the rule proposed for it: the call also builds the masks of leaves the SAME list pops next -- the entries below the popped
          one, in pop order -- while their triangles fit the 64 lanes.  A candidate joins when it is not marked, its record's link is
          a leaf, that leaf's tag is not in the table and its n_real fits the lanes left; the scan stops at the first inner entry or
          the first leaf that does not fit; the popped leaf is stored last.  The root's one-entry list has no neighbours.

Counted per unit: leaf-mask calls under both rules, lanes used per call, masks built ahead that no later visit of the unit uses,
and leaf-table evictions (a store over another valid tag) with those that only the masks built ahead cause.

usage: leaf_batch_count.py [atrium|teapot] [units] [passes]     (passes: 16 = 256 samples, 4 = 64, 1 = 16)
"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

F = np.float32


def leaf_entries():
    src = open(os.path.join(ROOT, "minipath_amd", "csrc", "mask_cache.h")).read()
    return int(re.search(r"^#define\s+MP_LEAF_ENTRIES\s+(\d+)\b", src, re.M).group(1))


def batch_members(entries_below, is_marked, link_of, tagged, n_popped, lanes=64):
    """the batch rule: which of `entries_below` (arena positions in pop order) join the popped leaf of n_popped triangles;
    returns [(position, link)]"""
    left, out = lanes - n_popped, []
    for pos in entries_below:
        if is_marked(pos):
            continue
        link = link_of(pos)
        if link & 63 == 0:  # an inner entry (or a null link: none in a list): the scan stops
            break
        if tagged(link >> 6):
            continue
        if (link & 63) > left:  # the first leaf that does not fit: the scan stops
            break
        left -= link & 63
        out.append((pos, link))
    return out


def main():
    import minipath_amd as mp
    from minipath_amd import scenes
    from oracle import pyoracle as po
    from sim_collapse import fma32
    from sim_tri_reject import interval_reject
    from tests import graft_model as gm
    from tests import unit_list_model as ul

    scene = sys.argv[1] if len(sys.argv) > 1 else "atrium"
    units = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    passes = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    res, spp, seed = (1920, 1080), 16 * passes, 0x5EED
    if scene == "teapot":
        host, cam = mp.TriangleBvh.with_obj(os.path.join(ROOT, "tests", "golden", "teapot.obj")), mp.Camera.teapot_view()
    else:
        host, cam = mp.TriangleBvh.build(*scenes.atrium(1, 1.0)), scenes.atrium_camera()
    sarr = cam.build_sampler(res).as_array()
    tris = gm.LeafTriangles(host)
    entries, arena_entries = ul.header_sizes()
    nleaf = leaf_entries()
    nodes, root = host.device_tree(packet=True)[:2]
    root_rec = nodes.shape[0] * nodes.shape[1]

    def dot(a, b):
        return fma32(a[2], b[2], fma32(a[1], b[1], F(a[0]) * F(b[0])))

    def fms(a, b, c):
        return fma32(a, b, -c)

    def leaf_visit(link, header, o, d, live):
        """(closest accepted t per ray among the triangles the unit mask keeps, whether it keeps any)"""
        if link not in tris.cache:
            tris.nearest(link, o[:1], d[:1])
        v0, e1, e2 = tris.cache[link]
        lo, hi, _ = header
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            keep = ~interval_reject(v0, e1, e2, lo[0], hi[0], lo[2], hi[2], far=True)
            dd, oo = [d[:, None, k] for k in range(3)], [o[:, None, k] for k in range(3)]
            E1, E2, V0 = ([a[None, :, k] for k in range(3)] for a in (e1, e2, v0))
            h = [fms(dd[1], E2[2], dd[2] * E2[1]), fms(dd[2], E2[0], dd[0] * E2[2]), fms(dd[0], E2[1], dd[1] * E2[0])]
            det = np.broadcast_to(dot(E1, h), (o.shape[0], v0.shape[0])).astype(F)
            s = [(oo[k] - V0[k]).astype(F) for k in range(3)]
            un = dot(s, h)
            q = [fms(s[1], E1[2], s[2] * E1[1]), fms(s[2], E1[0], s[0] * E1[2]), fms(s[0], E1[1], s[1] * E1[0])]
            vn, tn = dot(dd, q), dot(E2, q)
            inv = (F(1) / det).astype(F)
            u, v, t = (inv * un).astype(F), (inv * vn).astype(F), (inv * tn).astype(F)
            acc = (u >= 0) & (v >= 0) & ((u + v).astype(F) <= 1) & (t >= 0) & live[:, None]
        assert not (acc.any(0) & ~keep).any(), "a triangle the unit mask drops is accepted by a live ray"
        tt = np.where(acc & keep[None, :], t, F(np.inf))
        return (tt.min(1).astype(F) if tt.shape[1] else np.full(o.shape[0], np.inf, F)), bool(keep.any())

    keys = ("calls_single", "calls_batch", "lanes_single", "lanes_batch", "ahead", "ahead_used", "evict_single", "evict_batch", "evict_ahead",
            "root_calls", "stop_inner", "stop_fit", "stop_end")
    cnt = {k: 0 for k in keys}

    def walk_unit(header, rays):
        table, arena, marked, out = {}, [], set(), []
        leaf = {"single": {}, "batch": {}}  # slot -> first packet
        ahead = set()  # first packets whose mask the batch rule built ahead and no visit has used yet
        for o, d, inv in rays:
            best = np.full(o.shape[0], np.finfo(F).max, F)
            frames = []
            cur = [None, 1, np.ones(o.shape[0], bool)]
            while True:
                if cur[1] == 0:
                    if not frames:
                        break
                    cur = frames.pop()
                    continue
                cur[1] -= 1
                pos = None if cur[0] is None else cur[0] + cur[1]
                if pos in marked:
                    continue
                idx = root_rec if pos is None else arena[pos]
                box, link = ul._record(nodes, root, idx)
                ok = gm._slab(box, o, inv, np.where(cur[2], best, F(-1)))
                if not ok.any():
                    continue
                if link & 63:
                    first, n_real = link >> 6, link & 63
                    slot = first & (nleaf - 1)
                    # -- the leaf table under the rule as it is
                    if leaf["single"].get(slot) != first:
                        cnt["calls_single"] += 1
                        cnt["lanes_single"] += n_real
                        cnt["evict_single"] += slot in leaf["single"]
                        leaf["single"][slot] = first
                    # -- and under the batch rule
                    tb = leaf["batch"]
                    if tb.get(slot) != first:
                        cnt["calls_batch"] += 1
                        cnt["root_calls"] += pos is None
                        below = [] if pos is None else [cur[0] + i for i in range(cur[1] - 1, -1, -1)]
                        members = batch_members(below, lambda p: p in marked, lambda p: ul._record(nodes, root, arena[p])[1],
                                                lambda f: tb.get(f & (nleaf - 1)) == f, n_real)
                        # (why the scan ended, for the record)
                        taken = {p for p, _ in members}
                        ended = "stop_end"
                        for p in below:
                            if p in marked or p in taken:
                                continue
                            l = ul._record(nodes, root, arena[p])[1]
                            if l & 63 == 0:
                                ended = "stop_inner"; break
                            if tb.get((l >> 6) & (nleaf - 1)) == (l >> 6):
                                continue
                            ended = "stop_fit"; break
                        cnt[ended] += 1
                        cnt["lanes_batch"] += n_real + sum(l & 63 for _, l in members)
                        for _, l in members:
                            f2 = l >> 6
                            s2 = f2 & (nleaf - 1)
                            if s2 in tb and tb[s2] != f2:
                                cnt["evict_batch"] += 1
                                cnt["evict_ahead"] += 1
                                ahead.discard(tb[s2])
                            tb[s2] = f2
                            ahead.add(f2)
                            cnt["ahead"] += 1
                        if slot in tb and tb[slot] != first:  # the popped leaf is stored last
                            cnt["evict_batch"] += 1
                            ahead.discard(tb[slot])
                        tb[slot] = first
                    elif first in ahead:
                        ahead.discard(first)
                        cnt["ahead_used"] += 1
                    t, any_kept = leaf_visit(link, header, o, d, ok)
                    if not any_kept and pos is not None:
                        marked.add(pos)
                    best = np.where(ok & (t < best), t, best).astype(F)
                    continue
                node = link >> 6
                slot = ul.node_slot(node, entries)
                e = table.get(slot)
                if e is None or e[0] != node:
                    lst = ul.build_list(nodes, node, header, arena_entries - len(arena))
                    if lst is None:
                        return None  # (a unit whose lists overflow the arena: not what this tool counts)
                    e = table[slot] = (node, len(arena), len(lst))
                    arena.extend(lst)
                if e[2]:
                    if cur[1]:
                        frames.append(cur)
                    cur = [e[1], e[2], ok]
            out.append(best)
        return np.array(out)

    class MaskedTriangles:
        def __init__(self, header):
            self.header = header

        def nearest(self, link, o, d):
            return leaf_visit(link, self.header, o, d, np.ones(o.shape[0], bool))[0]

    rng = np.random.default_rng(11)
    n_units = declined = 0
    for _ in range(units):
        x0, y0 = int(rng.integers(0, res[0] // 2)), int(rng.integers(0, res[1] // 2))
        up = ul.unit_passes(po, sarr, res, spp, seed, y0 * (res[0] // 2) + x0, ul.shipped_margin())
        if up is None:
            declined += 1
            continue
        header, rays = up
        saved = dict(cnt)
        got = walk_unit(header, rays)
        if got is None:
            cnt.update(saved)
            declined += 1
            continue
        model, _, _ = ul.list_unit_walk(nodes, root, MaskedTriangles(header), header, rays, entries, arena_entries)
        assert np.array_equal(got.view(np.uint32), model.view(np.uint32)), "best.t differs from the model's list walk"
        n_units += 1

    u = lambda k: cnt[k] / max(n_units, 1)
    print(f"{scene}: {n_units} units x {passes} passes of 2x2 pixels x 16 samples ({declined} units skipped); packet tree, leaf table {nleaf}")
    print("asserted: no triangle the unit mask drops is accepted by a live ray; best.t equal to tests/unit_list_model.py's list walk")
    print("per unit:                                              single     batch")
    print(f"  leaf-mask calls                                     {u('calls_single'):7.2f}   {u('calls_batch'):7.2f}")
    print(f"  lanes used per call                                 {cnt['lanes_single'] / max(cnt['calls_single'], 1):7.2f}   {cnt['lanes_batch'] / max(cnt['calls_batch'], 1):7.2f}")
    print(f"  leaf-table evictions                                {u('evict_single'):7.3f}   {u('evict_batch'):7.3f}   (by masks built ahead: {u('evict_ahead'):.3f})")
    print(f"  masks built ahead / of these, used by a later visit            {u('ahead'):7.2f} / {u('ahead_used'):.2f}")
    print(f"  batch calls from the root's list (no neighbours)               {u('root_calls'):7.2f}")
    print(f"  batch calls whose scan ends at: the list's end / an inner entry / a leaf that does not fit   "
          f"{u('stop_end'):.2f} / {u('stop_inner'):.2f} / {u('stop_fit'):.2f}")


if __name__ == "__main__":
    main()
