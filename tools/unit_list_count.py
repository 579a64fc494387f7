#!/usr/bin/env python3
"""What the cached packet walk costs per pass with per-unit child LISTS (mask_cache.h unit_list_build) against per-node masks,
counted on the CPU: the library's own exported trees (TriangleBvh.device_tree: the 16-slot packet tree and the wide tree) walked
by the numpy model of tests/unit_list_model.py -- mask_unit_walk, the walk before the lists, and list_unit_walk with the header's
table and arena sizes -- on the metric's frame (1920 x 1080, work units of 2 x 2 pixels x 16 samples per pass, rays from the
oracle, unit bounds from the corner rays).

Per tree and walk, per pass: pops, pops culled for every ray, inner links followed (node visits: table lookups), leaf visits; per
unit: lists built, table evictions, arena resets, absorbed nodes; the longest list.  Asserts that every ray's best.t is bit-equal
between the two walks and the two trees in every pass, that the leaves are visited in the same order, and that no ray passes a child
that the unit's bounds reject.

usage: unit_list_count.py [atrium|teapot] [units] [passes per unit]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import minipath_amd as mp
    from minipath_amd import scenes
    from oracle import pyoracle as po
    from tests import graft_model as gm
    from tests import unit_list_model as ul

    scene = sys.argv[1] if len(sys.argv) > 1 else "atrium"
    units = int(sys.argv[2]) if len(sys.argv) > 2 else 80
    passes = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    res, spp, seed = (1920, 1080), 16 * passes, 0x5EED
    if scene == "teapot":
        host, cam = mp.TriangleBvh.with_obj(os.path.join(ROOT, "tests", "golden", "teapot.obj")), mp.Camera.teapot_view()
    else:
        host, cam = mp.TriangleBvh.build(*scenes.atrium(1, 1.0)), scenes.atrium_camera()
    sarr = cam.build_sampler(res).as_array()
    tris = gm.LeafTriangles(host)
    entries, arena = ul.header_sizes()
    trees = {"packet tree": host.device_tree(packet=True)[:2], "wide tree": host.device_tree()[:2]}
    mask = {k: {"pops": 0, "culled": 0, "node_visits": 0, "leaf_visits": 0} for k in trees}
    lists = {k: ul.new_stats() for k in trees}
    rng = np.random.default_rng(11)
    n_units = n_pass = declined = 0
    for _ in range(units):
        x0, y0 = int(rng.integers(0, res[0] // 2)), int(rng.integers(0, res[1] // 2))
        up = ul.unit_passes(po, sarr, res, spp, seed, y0 * (res[0] // 2) + x0, ul.shipped_margin())
        if up is None:
            declined += 1  # the corner bounds decline or a pass leaves them: not what this tool counts
            continue
        header, rays = up
        n_units += 1
        n_pass += len(rays)
        bests = []
        for k, (nodes, root) in trees.items():
            mb, mo, c = ul.mask_unit_walk(nodes, root, tris, header, rays, check_rejected=True)
            for key in mask[k]:
                mask[k][key] += c[key]
            lb, lo, lists[k] = ul.list_unit_walk(nodes, root, tris, header, rays, entries, arena, stats=lists[k])
            assert np.array_equal(mb.view(np.uint32), lb.view(np.uint32)), "best.t differs between the mask walk and the list walk"
            assert all(b is None or a == b for a, b in zip(mo, lo)), "leaf visit order"
            bests.append(lb)
        assert np.array_equal(bests[0].view(np.uint32), bests[1].view(np.uint32)), "best.t differs between the trees"
    print(f"{scene}: {n_units} units x {passes} passes of 2x2 pixels x 16 samples ({declined} units skipped); node table {entries}, arena {arena}")
    print("every ray's best.t bit-equal between the walks and the trees in every pass; leaves visited in the same order; no rejected child passed")
    print(f"{'walk':34s} {'pops/pass':>10s} {'culled/pass':>12s} {'node visits/pass':>17s} {'leaf visits/pass':>17s} {'lists/unit':>11s} {'absorbed/unit':>14s} "
          f"{'evictions/unit':>15s} {'resets/unit':>12s} {'longest list':>13s}")
    for k in trees:
        m, s = mask[k], lists[k]
        print(f"{k + ', masks':34s} {m['pops'] / n_pass:10.2f} {m['culled'] / n_pass:12.2f} {m['node_visits'] / n_pass:17.2f} {m['leaf_visits'] / n_pass:17.2f}")
        print(f"{k + ', lists':34s} {s['pops'] / n_pass:10.2f} {s['culled'] / n_pass:12.2f} {s['links'] / n_pass:17.2f} {s['leaf_visits'] / n_pass:17.2f} "
              f"{s['builds'] / n_units:11.2f} {s['absorbed'] / n_units:14.1f} {s['evictions'] / n_units:15.2f} {s['resets'] / n_units:12.2f} {s['longest']:13d}")
        print(f"{'':34s} kept inner children left unexpanded: {s['not_nested'] / n_units:.2f} per unit not nested, {s['room_stops'] / n_units:.2f} for want of room; "
              f"{s['dropped'] / n_units:.1f} per unit dropped (no kept child)")


if __name__ == "__main__":
    main()
