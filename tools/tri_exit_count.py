#!/usr/bin/env python3
"""Where the triangle tests of the cached packet walk end, and what two rules change, counted on the CPU: the library's exported
packet tree walked by a numpy restatement of trace_packet_cached (packet_walk.h) over child lists (tests/unit_list_model.py: build_list,
node_slot; its list_unit_walk is the check of this walk), the unit triangle masks by tools/sim_tri_reject.py's interval test, on the
metric's frame (1920 x 1080, units of 2 x 2 pixels x 16 samples per pass, rays from the oracle, unit bounds from the corner rays at
the shipped margin; unit-pick seed 11).

Rule 1 (mask_cache.h, tri_exit1_key / tri_exit2_key): a wave leaves a triangle before the division when every live ray is surely
rejected -- today on the near side (a numerator surely negative), now also on the far side (u, or u + v, surely above 1).
Rule 2 (trace_packet_cached): a list entry whose leaf has an empty unit triangle mask is marked by the visit that finds it so; later
pops of the entry stop at the mark.
Rule 3 (mask_cache.h, tri_may_hit): the unit triangle mask also drops a triangle when u > 1 or v > 1 for every ray inside the unit's
bounds (sim_tri_reject.interval_reject, far=True).  Every unit is walked under the masks without and with it: surviving tests, where
the removed tests would have ended, empty-mask leaf pops and pops stopped at a mark under each.

Asserted on every counted pass: no triangle that either form of rule 1 leaves is accepted by a live ray; no triangle the unit mask
drops is accepted by a live ray; every ray's best.t is bit-equal with and without the skip, and equal to the model's list walk.

usage: tri_exit_count.py [atrium|teapot] [units]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

F = np.float32
TINY, HUGE, SLACK = F(2.0 ** -40), F(2.0 ** 40), F(1.0 + 2.0 ** -20)


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
    passes = 16
    res, spp, seed = (1920, 1080), 16 * passes, 0x5EED
    if scene == "teapot":
        host, cam = mp.TriangleBvh.with_obj(os.path.join(ROOT, "tests", "golden", "teapot.obj")), mp.Camera.teapot_view()
    else:
        host, cam = mp.TriangleBvh.build(*scenes.atrium(1, 1.0)), scenes.atrium_camera()
    sarr = cam.build_sampler(res).as_array()
    tris = gm.LeafTriangles(host)
    entries, arena_entries = ul.header_sizes()
    nodes, root = host.device_tree(packet=True)[:2]
    root_rec = nodes.shape[0] * nodes.shape[1]
    keys = ("pops", "leaf_pops", "leaf_culled", "leaf_visits", "empty_pops", "empty_visits", "skipped", "tests", "old1", "old2", "old_full",
            "old_full_none", "new1", "new2", "new_full", "new_full_none", "some", "far_slack_lost", "removed1", "removed2", "removed_full")
    # one set of counts per rule of the unit triangle masks: False = without the far-side terms (-DMP_NO_MASK_FAR), True = the shipped rule
    cnts = {far: {k: 0 for k in keys} for far in (False, True)}

    def dot(a, b):
        return fma32(a[2], b[2], fma32(a[1], b[1], F(a[0]) * F(b[0])))

    def fms(a, b, c):
        return fma32(a, b, -c)

    def flipped(det, num):
        with np.errstate(invalid="ignore"):
            ok = np.abs(det) <= HUGE
        return np.where(ok, (num.view(np.uint32) ^ (det.view(np.uint32) & np.uint32(0x80000000))).view(F), F(1)).astype(F)

    def leaf_visit(link, header, o, d, live, best, cnt, far):
        """the leaf's surviving triangles for the live rays: the closest accepted t per ray (inf: none); cnt: the counts to add to, or None"""
        if link not in tris.cache:
            tris.nearest(link, o[:1], d[:1])
        v0, e1, e2 = tris.cache[link]
        lo, hi, _ = header
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            keep = ~interval_reject(v0, e1, e2, lo[0], hi[0], lo[2], hi[2], far=far)
            removed = ~interval_reject(v0, e1, e2, lo[0], hi[0], lo[2], hi[2], far=False) & ~keep  # what the far-side terms take out
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
            xu, xv, xt = flipped(det, un), flipped(det, vn), flipped(det, tn)
            near2 = np.fmin(np.fmin(xu, xv), xt)
            far_u, far_uv = fma32(np.abs(det), SLACK, -xu), fma32(np.abs(det), SLACK, -(xu + xv).astype(F))
            dead = ~live[:, None]
            old1 = (dead | (xu <= -TINY)).all(0)
            old2 = (dead | (near2 <= -TINY)).all(0)
            new1 = (dead | (np.fmin(xu, far_u) <= -TINY)).all(0)
            new2 = (dead | (np.fmin(np.fmin(near2, far_u), far_uv) <= -TINY)).all(0)
            # the rule as the issue states it (x > A, A = fl(|det| (1 + 2^-20))), for what sharing the near side's threshold gives up
            A = (np.abs(det) * SLACK).astype(F)
            rule2 = (dead | (near2 <= -TINY) | (xu > A) | ((xu + xv).astype(F) > A)).all(0)
        some = acc.any(0)
        assert not (some & ~keep).any(), "a triangle the unit mask drops is accepted by a live ray"
        assert not (some & (old1 | old2 | new1 | new2 | rule2)).any(), "a triangle the wave leaves is accepted by a live ray"
        assert not (old1 & ~new1).any() and not (old2 & ~new2).any()
        if cnt is not None:
            k = keep
            # where a removed triangle's test ends when it is still made (the walk with both early-outs): what its removal saves
            cnt["removed1"] += int((removed & new1).sum()); cnt["removed2"] += int((removed & ~new1 & new2).sum())
            cnt["removed_full"] += int((removed & ~new1 & ~new2).sum())
            cnt["tests"] += int(k.sum())
            cnt["old1"] += int((k & old1).sum()); cnt["old2"] += int((k & ~old1 & old2).sum())
            cnt["old_full"] += int((k & ~old1 & ~old2).sum()); cnt["old_full_none"] += int((k & ~old1 & ~old2 & ~some).sum())
            cnt["new1"] += int((k & new1).sum()); cnt["new2"] += int((k & ~new1 & new2).sum())
            cnt["new_full"] += int((k & ~new1 & ~new2).sum()); cnt["new_full_none"] += int((k & ~new1 & ~new2 & ~some).sum())
            cnt["some"] += int((k & some).sum())
            cnt["far_slack_lost"] += int((k & rule2 & ~new2).sum())
        tt = np.where(acc & keep[None, :], t, F(np.inf))
        return tt.min(1).astype(F) if tt.shape[1] else np.full(o.shape[0], np.inf, F), bool(keep.any())

    def walk_unit(header, rays, skip, cnt, far):
        """trace_packet_cached over one unit (ul.list_unit_walk with the leaf model above and rule 2): best t [passes, rays], or None
        for a unit with a pass that is left to the uncached walk (not what this tool counts)"""
        table, arena, marked, out, n = {}, [], set(), [], {"pops": 0, "skipped": 0}
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
                n["pops"] += 1
                if skip and pos in marked:
                    n["skipped"] += 1
                    continue
                idx = root_rec if pos is None else arena[pos]
                box, link = ul._record(nodes, root, idx)
                ok = gm._slab(box, o, inv, np.where(cur[2], best, F(-1)))
                if link & 63:
                    empty = None
                    if cnt is not None:
                        cnt["leaf_pops"] += 1
                    if not ok.any():
                        if cnt is not None:
                            cnt["leaf_culled"] += 1
                            # (is its mask empty?  only counted: the walk does not look)
                            empty = not leaf_visit(link, header, o, d, ok, best, None, far)[1]
                            cnt["empty_pops"] += empty
                        continue
                    t, any_kept = leaf_visit(link, header, o, d, ok, best, cnt, far)
                    if cnt is not None:
                        cnt["leaf_visits"] += 1
                        cnt["empty_pops"] += not any_kept
                        cnt["empty_visits"] += not any_kept
                    if not any_kept and pos is not None:
                        marked.add(pos)
                    best = np.where(ok & (t < best), t, best).astype(F)
                    continue
                if not ok.any():
                    continue
                node = link >> 6
                slot = ul.node_slot(node, entries)
                e = table.get(slot)
                if e is None or e[0] != node:
                    lst = ul.build_list(nodes, node, header, arena_entries - len(arena))
                    if lst is None:
                        table.clear(); arena.clear(); marked.clear()
                        if frames or cur[1]:
                            return None, n
                        lst = ul.build_list(nodes, node, header, arena_entries)
                    e = table[slot] = (node, len(arena), len(lst))
                    arena.extend(lst)
                if e[2]:
                    if cur[1]:
                        frames.append(cur)
                    cur = [e[1], e[2], ok]
            out.append(best)
        return np.array(out), n

    class MaskedTriangles:
        """the leaf model above as the `tris` of ul.list_unit_walk (every ray live: a ray that failed the leaf's box is not updated there)"""
        def __init__(self, header):
            self.header = header

        def nearest(self, link, o, d):
            return leaf_visit(link, self.header, o, d, np.ones(o.shape[0], bool), None, None, True)[0]

    rng = np.random.default_rng(11)
    n_units = n_pass = declined = 0
    for _ in range(units):
        x0, y0 = int(rng.integers(0, res[0] // 2)), int(rng.integers(0, res[1] // 2))
        up = ul.unit_passes(po, sarr, res, spp, seed, y0 * (res[0] // 2) + x0, ul.shipped_margin())
        if up is None:
            declined += 1
            continue
        header, rays = up
        saved = {far: dict(c) for far, c in cnts.items()}
        walks = {far: walk_unit(header, rays, False, cnts[far], far) for far in (False, True)}
        if walks[True][0] is None:  # (the lists do not depend on the triangle masks: both rules or neither)
            assert walks[False][0] is None
            for far in cnts:
                cnts[far].update(saved[far])
            declined += 1
            continue
        plain = walks[True][0]
        assert np.array_equal(plain.view(np.uint32), walks[False][0].view(np.uint32)), "best.t differs between the mask rules"
        for far in (False, True):
            skipped, n_skip = walk_unit(header, rays, True, None, far)
            n_plain = walks[far][1]
            assert n_plain["pops"] == n_skip["pops"] and n_plain["skipped"] == 0, "a pop that stops at a mark is still a pop of the list"
            cnts[far]["pops"] += n_plain["pops"]
            cnts[far]["skipped"] += n_skip["skipped"]
            assert np.array_equal(plain.view(np.uint32), skipped.view(np.uint32)), "best.t differs with the skip"
        model, _, _ = ul.list_unit_walk(nodes, root, MaskedTriangles(header), header, rays, entries, arena_entries)
        assert np.array_equal(plain.view(np.uint32), model.view(np.uint32)), "best.t differs from the model's list walk"
        n_units += 1
        n_pass += len(rays)

    cnt = cnts[True]
    p = lambda k: cnt[k] / n_pass
    q = lambda k: cnts[False][k] / n_pass
    print(f"{scene}: {n_units} units x {passes} passes of 2x2 pixels x 16 samples ({declined} units skipped); packet tree, node table {entries}, arena {arena_entries}")
    print("asserted on every pass: no triangle a wave leaves early (either rule) or the unit mask drops is accepted by a live ray; best.t bit-equal with and")
    print("without the skip of marked entries, and equal to tests/unit_list_model.py's list walk")
    print("per pass:")
    print(f"  pops (root + list entries)                          {p('pops'):7.2f}")
    print(f"  leaf pops / culled by the per-ray slab / visited     {p('leaf_pops'):7.2f} / {p('leaf_culled'):.2f} / {p('leaf_visits'):.2f}")
    print(f"  leaf pops whose unit triangle mask is empty (visited) {p('empty_pops'):6.2f} ({p('empty_visits'):.2f})")
    print(f"  ... that stop at a mark (rule 2)                     {p('skipped'):7.2f}   pops that go on to the record load: {p('pops'):.2f} -> {p('pops') - p('skipped'):.2f}")
    print(f"  triangle tests (survivors of the unit masks)         {p('tests'):7.2f}")
    print("  the unit masks without / with their far-side terms (u.lo > 1, v.lo > 1; every other line is with them):")
    print(f"    triangle tests (survivors)                         {q('tests'):7.2f} -> {p('tests'):.2f}")
    print(f"    the tests removed: would leave at the first early-out / at the second / run the division  {p('removed1'):.2f} / {p('removed2'):.2f} / {p('removed_full'):.2f}")
    print(f"    leaf pops whose mask is empty (visited)            {q('empty_pops'):7.2f} ({q('empty_visits'):.2f}) -> {p('empty_pops'):.2f} ({p('empty_visits'):.2f})")
    print(f"    pops that stop at a mark                           {q('skipped'):7.2f} -> {p('skipped'):.2f}")
    print(f"  {'':52s} {'near side only':>15s} {'with the far side':>18s}")
    for label, a, b in (("leave at the first early-out", "old1", "new1"), ("leave at the second", "old2", "new2"), ("run the division and the acceptance", "old_full", "new_full"),
                        ("... of those, accepted by no ray", "old_full_none", "new_full_none")):
        print(f"  {label:52s} {p(a):15.2f} {p(b):18.2f}")
    print(f"  triangles that some live ray passes (ignoring best.t) {p('some'):6.2f}")
    print(f"  left by `x > A` as stated but not by the shared threshold (difference below 2^-40): {cnt['far_slack_lost']} triangles in all")


if __name__ == "__main__":
    main()
