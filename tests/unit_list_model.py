"""A numpy restatement of the cached packet walk's per-unit child LISTS (minipath_amd/csrc/mask_cache.h, unit_list_build, and
packet_walk.h, trace_packet_cached), on exported trees (TriangleBvh.device_tree: the packet tree, 16 slots, or the wide tree, 8).

build_list     the list of one node under a unit's bounds B, entry for entry what unit_list_build appends to the arena
list_unit_walk the walk of one unit over lists: node table (tag compare, direct-mapped on node_slot), arena, the reset when a list
               does not fit, and the pass that is left to the uncached walk when frames still point into the arena
mask_unit_walk the walk before the lists (tests/graft_model.py cached_unit_walk: one kept-children mask per node), with the order
               of its leaf visits -- what the list walk has to reproduce

The per-ray box and triangle tests are tests/graft_model.py's (shared by every walk of the model: they decide nothing here)."""
import os
import re

import numpy as np

from tests import graft_model as gm
from tests.conftest import ROOT

F = np.float32
NULL = gm.NULL
LIST_DEPTH = 64  # kListDepth


def header_sizes():
    """(node table entries, arena entries) as mask_cache.h defines them"""
    src = open(os.path.join(ROOT, "minipath_amd", "csrc", "mask_cache.h")).read()
    arena = re.findall(r"^#define\s+MP_ARENA_ENTRIES\s+(\d+)\b", src, re.M)
    assert len(arena) == 1
    return gm.mask_table_sizes()[0], int(arena[0])


def shipped_margin():
    """MP_MCACHE_MARGIN as mask_cache.h defines it"""
    src = open(os.path.join(ROOT, "minipath_amd", "csrc", "mask_cache.h")).read()
    return float(re.search(r"#define MP_MCACHE_MARGIN ([-0-9.e]+)f", src).group(1))


def node_slot(node, entries, slot_mask=0xFFFFFFFF):
    """mask_cache.h node_slot: the last tag dword holds the arena's fill, so the last two residues share a slot"""
    return min(node & (entries - 1) & slot_mask, entries - 2)


def kept_children(nodes, n, header):
    """slots of node n that the unit keeps (bounds_may_hit on the real children), ascending"""
    ab = gm._analytic_bounds()
    lo, hi, neg = header
    recs = nodes[n]
    real = recs[:, 6] != NULL
    with np.errstate(invalid="ignore", over="ignore"):
        keep = real & ~ab.box_reject(recs[:, :6].view(F), lo, hi, neg)
    return [int(j) for j in np.nonzero(keep)[0]]


def new_stats():
    return {"builds": 0, "evictions": 0, "resets": 0, "abandoned": 0, "absorbed": 0, "max_level": 0, "two_level_entries": 0,
            "not_nested": 0, "room_stops": 0, "dropped": 0, "longest": 0, "pops": 0, "culled": 0, "links": 0, "leaf_visits": 0, "absorbed_boxes": []}


def build_list(nodes, node, header, room, stats=None):
    """unit_list_build: the entries (record indices node * slots + slot) of node's list, or None when the node's own kept children do
    not fit `room` (the caller resets).  stats["absorbed_boxes"] collects (box of the absorbed child in its parent's record, boxes of
    its kept children) for the nestedness check."""
    stats = new_stats() if stats is None else stats
    slots = nodes.shape[1]
    mask = kept_children(nodes, node, header)
    if len(mask) > room:
        return None
    out, pend, stack, cur, level = [], len(mask), [], node, 0
    while True:
        while not mask and stack:
            cur, mask, level = stack.pop()
        if not mask:
            break
        j = mask.pop(0)
        pend -= 1
        rec = cur * slots + j
        link = int(nodes[cur, j, 6])
        emit = True
        if link & 63 == 0:
            m = link >> 6
            km = kept_children(nodes, m, header)
            if not km:
                emit = False
                stats["dropped"] += 1
            else:
                pbox = nodes[cur, j, :6].view(F)
                g = nodes[m][km][:, :6].view(F)
                nested = bool((pbox[None, :3] <= g[:, :3]).all() and (g[:, 3:] <= pbox[None, 3:]).all())
                if nested and len(stack) < LIST_DEPTH and len(out) + pend + len(km) <= room:
                    if mask:
                        stack.append((cur, mask, level))
                    cur, mask, level = m, list(km), level + 1
                    pend += len(km)
                    emit = False
                    stats["absorbed"] += 1
                    stats["max_level"] = max(stats["max_level"], level)
                    stats["absorbed_boxes"].append((pbox.copy(), g.copy()))
                elif not nested:
                    stats["not_nested"] += 1
                else:
                    stats["room_stops"] += 1
        if emit:
            out.append(rec)
            stats["two_level_entries"] += level >= 2
    stats["longest"] = max(stats["longest"], len(out))
    return out


def _record(nodes, root, idx):
    slots = nodes.shape[1]
    if idx == nodes.shape[0] * slots:  # the root's record: child 0 of the pseudo-node behind the last node
        return np.array([-np.inf] * 3 + [np.inf] * 3, F), root
    return nodes[idx // slots, idx % slots, :6].view(F), int(nodes[idx // slots, idx % slots, 6])


def list_unit_walk(nodes, root, tris, header, passes, entries, arena_entries, slot_mask=0xFFFFFFFF, stats=None):
    """trace_packet_cached over one unit.  Returns (best t [passes, rays], per pass the leaf links in visit order -- None for a pass
    that was left to the uncached walk --, stats)."""
    stats = new_stats() if stats is None else stats
    table, arena, out, orders = {}, [], [], []
    root_rec = nodes.shape[0] * nodes.shape[1]
    for o, d, inv in passes:
        best = np.full(o.shape[0], np.finfo(F).max, F)
        frames, order, abandoned = [], [], False
        cur = [None, 1, np.ones(o.shape[0], bool)]  # [first entry (None: the root's list), entries left, rays live at the visit]
        while True:
            if cur[1] == 0:
                if not frames:
                    break
                cur = frames.pop()
                continue
            cur[1] -= 1
            idx = root_rec if cur[0] is None else arena[cur[0] + cur[1]]
            box, link = _record(nodes, root, idx)
            ok = gm._slab(box, o, inv, np.where(cur[2], best, F(-1)))
            stats["pops"] += 1
            if not ok.any():
                stats["culled"] += 1
                continue
            stats["links" if link & 63 == 0 else "leaf_visits"] += 1
            if link & 63:
                order.append(link)
                t = tris.nearest(link, o, d)
                best = np.where(ok & (t < best), t, best).astype(F)
                continue
            node = link >> 6
            slot = node_slot(node, entries, slot_mask)
            e = table.get(slot)
            if e is None or e[0] != node:
                stats["builds"] += 1
                stats["evictions"] += e is not None
                lst = build_list(nodes, node, header, arena_entries - len(arena), stats)
                if lst is None:
                    table.clear()
                    arena.clear()
                    stats["resets"] += 1
                    if frames or cur[1]:
                        stats["abandoned"] += 1
                        abandoned = True
                        break
                    lst = build_list(nodes, node, header, arena_entries, stats)
                e = table[slot] = (node, len(arena), len(lst))
                arena.extend(lst)
                assert len(arena) <= arena_entries
            if e[2]:
                if cur[1]:
                    frames.append(cur)
                cur = [e[1], e[2], ok]
        if abandoned:
            best, order = gm.plain_walk(nodes, root, tris, o, d, inv), None
        out.append(best)
        orders.append(order)
    return np.array(out), orders, stats


def mask_unit_walk(nodes, root, tris, header, passes, check_rejected=False):
    """the walk over kept-children masks (graft_model.cached_unit_walk with a table that never evicts), with its leaf visits:
    (best t [passes, rays], per pass the leaf links in visit order, counts)"""
    masks, out, orders = {}, [], []
    counts = {"pops": 0, "culled": 0, "node_visits": 0, "leaf_visits": 0}
    for o, d, inv in passes:
        best = np.full(o.shape[0], np.finfo(F).max, F)
        frames, order = [], []
        cur = ([(np.array([-np.inf] * 3 + [np.inf] * 3, F), root)], np.ones(o.shape[0], bool))
        while True:
            todo, live = cur
            if not todo:
                if not frames:
                    break
                cur = frames.pop()
                continue
            box, link = todo.pop()
            counts["pops"] += 1
            ok = gm._slab(box, o, inv, np.where(live, best, F(-1)))
            if not ok.any():
                counts["culled"] += 1
                continue
            if link & 63:
                order.append(link)
                counts["leaf_visits"] += 1
                t = tris.nearest(link, o, d)
                best = np.where(ok & (t < best), t, best).astype(F)
                continue
            counts["node_visits"] += 1
            child = link >> 6
            if child not in masks:
                masks[child] = kept_children(nodes, child, header)
            if check_rejected:  # no ray of the pass passes a child the unit's bounds reject
                for i in np.nonzero(nodes[child, :, 6] != NULL)[0]:
                    assert int(i) in masks[child] or not gm._slab(nodes[child, i, :6].view(F), o, inv, np.where(ok, best, F(-1))).any(), (child, int(i))
            kids = [(nodes[child, i, :6].view(F), int(nodes[child, i, 6])) for i in masks[child]]
            if kids:
                if todo:
                    frames.append((todo, live))
                cur = (kids, ok)
        out.append(best)
        orders.append(order)
    return np.array(out), orders, counts


def unit_passes(oracle, sarr, res, spp, seed, unit_index, margin):
    """Unit `unit_index` (row-major, 2 x 2 pixels) of a frame as the packet kernel walks it with 16 samples in flight
    (graft_model.evict_unit_passes for any camera): (header (lo, hi, neg) of the corner bounds, passes [(o, d, inv)] of 64 rays),
    or None where mask_cache_begin_unit declines or a pass leaves the bounds."""
    ab = gm._analytic_bounds()
    smp = oracle.sampler_from_array(sarr)
    ux, uy = (unit_index % (res[0] // 2)) * 2, (unit_index // (res[0] // 2)) * 2
    state, lo, hi = ab.corner_header(sarr, ab.jitter_scale(), ux, ux + 1, uy, uy + 1, margin)
    if state == 0xFFFFFFFF:
        return None
    neg = np.array([(state >> k) & 1 for k in range(3)], bool)
    passes = []
    for s0 in range(0, spp, 16):
        rays = [oracle.sample_ray(smp, ux + (l // 16) % 2, uy + (l // 16) // 2,
                                  oracle.lib().mpo_sample_key(seed, res[0], spp, ux + (l // 16) % 2, uy + (l // 16) // 2, s0 + l % 16))
                for l in range(64)]
        o, d, inv = (np.array([list(getattr(r, k)) for r in rays], F) for k in ("o", "d", "inv"))
        v = np.stack([o, inv, d])
        if not (((v >= lo[:, None, :]) & (v <= hi[:, None, :])).all() and ((inv < 0) == neg[None]).all()):
            return None
        passes.append((o, d, inv))
    return (lo, hi, neg), passes


class ExactTriangles:
    """graft_model.LeafTriangles with the reference's own bits: a leaf's packets decompressed as RelativePoint8::decompress does
    (size.mul_add(relative, min): one rounding, restated in f64 with a round-to-odd sum so that the cast to f32 rounds once) and
    tested by the oracle's triangle test (pyoracle.tri8_intersect, triangle.rs:183-217), ray by ray and packet by packet.  With it
    a model walk's best.t can be compared with the oracle's, bit for bit.  Results are kept per (leaf, bundle of rays): the walks
    of one unit ask for the same ones."""

    def __init__(self, host, oracle):
        self.oracle = oracle
        base = gm.LeafTriangles(host)
        self.box, self.pk16 = base.box, base.pk16
        self.verts, self.rays, self.seen = {}, {}, {}

    @staticmethod
    def _fma32(a, b, c):
        """fl32(a * b + c) for f32 arrays: the product of two f32 is exact in f64; the f64 sum is made round-to-odd (TwoSum's
        residual is the sticky bit), which the final cast then rounds correctly"""
        p = np.float64(a) * np.float64(b)
        c = np.float64(c)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F)

    def _packets(self, link):
        if link not in self.verts:
            first, nreal = link >> 6, link & 63
            box = self.box[link]
            mn, size = box[:3], (box[3:] - box[:3]).astype(F)
            npk = (nreal + 7) // 8
            rel = (self.pk16[first:first + npk].astype(np.int32).astype(F) * (F(1) / F(65535))).astype(F)  # [packet][vertex][axis][lane]
            v = self._fma32(np.broadcast_to(size[None, None, :, None], rel.shape), rel, np.broadcast_to(mn[None, None, :, None], rel.shape))
            self.verts[link] = (np.ascontiguousarray(v), nreal)
        return self.verts[link]

    def nearest(self, link, o, d):
        """closest accepted distance of every ray (o, d: [rays, 3]) in the leaf, inf where none"""
        key = (link, o.tobytes(), d.tobytes())
        if key not in self.seen:
            v, nreal = self._packets(link)
            rk = (o.tobytes(), d.tobytes())
            if rk not in self.rays:
                self.rays[rk] = [self.oracle.ray_new(o[i], d[i]) for i in range(o.shape[0])]
            out = np.full(o.shape[0], np.inf, F)
            for i, ray in enumerate(self.rays[rk]):
                for p in range(v.shape[0]):
                    m, t, _, _ = self.oracle.tri8_intersect(v[p, 0], v[p, 1], v[p, 2], ray)
                    for lane in range(min(8, nreal - 8 * p)):
                        if (m >> lane) & 1 and t[lane] >= 0 and t[lane] < out[i]:
                            out[i] = t[lane]
            self.seen[key] = out
        return self.seen[key]
