"""Helpers of the cached packet walk's table and index-range tests (tests/test_packet_tree_limits_cpu.py,
tests/test_gpu_packet_tree_limits.py; the grafted scene also in tests/test_packet_tree_cpu.py).

1. The per-unit mask tables (minipath_amd/csrc/mask_cache.h): their sizes, read out of the header, and the oracle-side premise
   "this unit's walk meets two nodes / two leaves that share a table slot": a ray's closest hit names a leaf, the leaf a chain of
   ancestors in the exported tree, and the walk certainly looks every node of that chain up.

2. A scene given as reference-layout arrays whose packet tree has any wanted number of nodes: the teapot with a FILLER grafted in
   front of it.  Node 0 is a new root with two children: slot 0 -> node 1, the root of the filler, in a box of one quantisation step
   at the scene's min corner (no camera ray enters it), slot 1 -> the teapot's old root, in the full box.  The filler is n inner
   nodes without a leaf among them, in heap order (node j has the inner children 8 j + 1 ... 8 j + 8 while those exist, null links
   elsewhere, every box the full range of its parent's: the corner box again), so most of them have no children at all.  A node without real children is never
   absorbed by the wide and packet trees, so each filler node costs 128 bytes, no packets, and about one node of every tree.  The
   teapot's nodes follow the filler.

3. A numpy model of the cached walk's node table (cached_unit_walk), to show on the CPU that the eviction frame notices a walk that
   ignores the table's tags."""
import collections
import functools
import os
import re

import numpy as np

import minipath_amd as mp
from tests.conftest import ROOT, TEAPOT

NULL = 0xFFFFFFF8  # both the reference's null link and the device format's


@functools.lru_cache(maxsize=None)
def mask_table_sizes():
    """(MP_NODE_ENTRIES, MP_LEAF_ENTRIES) as mask_cache.h defines them, and checked to be what its tables use"""
    src = open(os.path.join(ROOT, "minipath_amd", "csrc", "mask_cache.h")).read()
    size = {}
    for name in ("MP_NODE_ENTRIES", "MP_LEAF_ENTRIES"):
        m = re.findall(r"^#define\s+" + name + r"\s+(\d+)\s*$", src, re.M)
        assert len(m) == 1, name
        size[name] = int(m[0])
        assert size[name] & (size[name] - 1) == 0
    assert re.search(r"constexpr int kMaskCacheEntries = MP_NODE_ENTRIES;", src) and re.search(r"constexpr int kLeafCacheEntries = MP_LEAF_ENTRIES;", src)
    return size["MP_NODE_ENTRIES"], size["MP_LEAF_ENTRIES"]


class Chains:
    """An exported device tree (TriangleBvh.device_tree) as lookup arrays: leaf_of[packet] = first packet of the packet's leaf,
    node_of[packet] = the node that holds the leaf's link, parent[node] (-1 for the root)."""

    def __init__(self, nodes, root, n_packets):
        assert root != NULL and (root & 63) == 0
        link = nodes[:, :, 6]
        real = link != NULL
        inner = real & ((link & 63) == 0)
        leaf = real & ((link & 63) != 0)
        self.count = nodes.shape[0]
        self.parent = np.full(self.count, -1, np.int64)
        owner = np.broadcast_to(np.arange(self.count)[:, None], link.shape)
        self.parent[link[inner] >> 6] = owner[inner]
        assert np.count_nonzero(self.parent < 0) == 1 and self.parent[root >> 6] < 0
        self.leaf_of = np.full(n_packets, -1, np.int64)
        self.node_of = np.full(n_packets, -1, np.int64)
        first, nreal, own = link[leaf] >> 6, link[leaf] & 63, owner[leaf]
        for f, n, o in zip(first.tolist(), nreal.tolist(), own.tolist()):
            k = (n + 7) // 8
            self.leaf_of[f:f + k] = f
            self.node_of[f:f + k] = o
        assert (self.leaf_of >= 0).all()

    def chain(self, node):
        out = []
        while node >= 0:
            out.append(node)
            node = int(self.parent[node])
        return out


def colliding_units(chains, unit_packets, node_entries, leaf_entries):
    """unit_packets: for every unit, the packets its sampled rays hit (closest hits of the oracle).  Returns (units that meet two
    distinct nodes with the same index & (node_entries - 1), units that meet two distinct leaves whose first packets agree in
    & (leaf_entries - 1)): a lower bound, the walk visits more than the hit chains."""
    node_units = leaf_units = 0
    up = {}
    for packets in unit_packets:
        nodes, leaves = set(), set()
        for p in set(packets):
            leaves.add(int(chains.leaf_of[p]))
            n = int(chains.node_of[p])
            if n not in up:
                up[n] = chains.chain(n)
            nodes.update(up[n])
        node_units += len({n & (node_entries - 1) for n in nodes}) < len(nodes)
        leaf_units += len({f & (leaf_entries - 1) for f in leaves}) < len(leaves)
    return node_units, leaf_units


def unit_hit_packets(oracle, orc, sampler, res, spp, seed, unit, rays_per_pixel):
    """The packets hit by samples 0 .. rays_per_pixel - 1 of every pixel, grouped by the kernel's units of unit = (w, h) pixels
    (row-major over the frame; the frame and its tiles are multiples of the unit)."""
    w, h = res
    assert w % unit[0] == 0 and h % unit[1] == 0 and rays_per_pixel <= spp
    L = oracle.lib()
    o = np.zeros((h, w, rays_per_pixel, 3), np.float32)
    d = np.zeros_like(o)
    for y in range(h):
        for x in range(w):
            for s in range(rays_per_pixel):
                r = oracle.sample_ray(sampler, x, y, L.mpo_sample_key(seed, w, spp, x, y, s))
                o[y, x, s], d[y, x, s] = r.o, r.d
    _, prim, _, _ = orc.trace(o.reshape(-1, 3), d.reshape(-1, 3))
    prim = prim.reshape(h, w, rays_per_pixel)
    out = []
    for y0 in range(0, h, unit[1]):
        for x0 in range(0, w, unit[0]):
            p = prim[y0:y0 + unit[1], x0:x0 + unit[0]].reshape(-1)
            out.append((p[p != oracle.NO_PRIM] >> 3).tolist())
    return out


# ---- the frame of the table-eviction cases ----------------------------------------------------------------------------------------
# scenes.atrium(1, 0.5): 1 398 literal, 1 388 wide and 1 027 packet-tree nodes, 18 326 packets -- both walked trees exceed the node
# table, the leaves the leaf table many times over; the benchmark's interior view on a small frame.
EVICT_DETAIL, EVICT_RES, EVICT_TS, EVICT_SEED = 0.5, (96, 64), 32, 5
# kernel family -> (samples per pixel, the kernel's unit in pixels (the family's unit, kernels_*.hip: BW x BH for the samples in flight), sampled rays per pixel)
EVICT_FAMILIES = {
    "packet, 16 in flight": (64, (2, 2), 8),
    "packet, 4 in flight": (16, (4, 4), 4),
    "feature planes, 4 in flight": (16, (4, 4), 4),
}


@functools.lru_cache(maxsize=None)
def evict_mesh():
    from minipath_amd import scenes

    return scenes.atrium(1, EVICT_DETAIL)


@functools.lru_cache(maxsize=None)
def evict_host():
    return mp.TriangleBvh.build(*evict_mesh())


@functools.lru_cache(maxsize=None)
def evict_oracle(oracle):
    """the oracle over the product builder's own tree (builder parity is tests/test_host_cpu.py's)"""
    h = evict_host()
    return oracle.Bvh.from_arrays(*h.export(), h.info().root_link, *h.get_bounding_box())


@functools.lru_cache(maxsize=None)
def _evict_unit_packets(oracle, spp, unit, rays_per_pixel):
    from minipath_amd import scenes

    smp = oracle.sampler_from_array(scenes.atrium_camera().build_sampler(EVICT_RES).as_array())
    return unit_hit_packets(oracle, evict_oracle(oracle), smp, EVICT_RES, spp, EVICT_SEED, unit, rays_per_pixel)


def evict_collisions(oracle, family, tree):
    """(units, units with a node-slot collision, units with a leaf-slot collision) of a kernel family on the eviction frame, for
    tree = (nodes, root, ...) as TriangleBvh.device_tree returns it -- the tree that family's walk uses"""
    spp, unit, rpp = EVICT_FAMILIES[family]
    packets = _evict_unit_packets(oracle, spp, unit, rpp)
    chains = Chains(tree[0], tree[1], evict_host().info().packet_count)
    return (len(packets),) + colliding_units(chains, packets, *mask_table_sizes())


def plan_facts(host):
    """what a launch plan reads off a plain TriangleBvh scene (tests/plan_probe.py), taken from its exports"""
    wide, lit = host.device_tree(), host.device_tree(literal=True)
    return {"kind": 0, "stack_bound": max(wide[2], lit[2]), "nodes": wide[0].shape[0], "packets": host.info().packet_count,
            "tris_bounded": 1, "boxes_ordered": 1, "members": 0}


# ---- the grafted scene ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _teapot_arrays():
    host = mp.TriangleBvh.with_obj(TEAPOT)
    info = host.info()
    assert info.root_link == 0, "the teapot's root is inner node 0"
    return host.export(), np.array(list(info.bbox_min), np.float32), np.array(list(info.bbox_max), np.float32)


def _filler_links(n, fertile):
    """reference links [n, 8] of the filler: nodes numbered breadth-first, a node's children consecutive; of a node's (up to)
    eight children the first `fertile` get children of their own.  fertile = 8 is the heap: node j -> 8 j + 1 ... 8 j + 8."""
    link = np.full((n, 8), NULL, np.uint32)
    parents, nxt = collections.deque([0]), 1
    while nxt < n:
        j = parents.popleft()
        m = min(8, n - nxt)
        link[j, :m] = (1 + nxt + np.arange(m, dtype=np.uint32)) << 3  # array index = 1 + filler index
        parents.extend(range(nxt, nxt + min(m, fertile)))
        nxt += m
    return link


def grafted_arrays(n_filler, fertile=8):
    """(inner, packets, shading, vertex normals, vertex tex, root link, bbox min, bbox max) of the grafted scene (see above):
    1 + n_filler + the teapot's inner nodes; what TriangleBvh.from_arrays and oracle.Bvh.from_arrays take.
    fertile < 8 makes the filler deeper and its traversal stack shallower: with 2, a node's stack bound is 8 + its height (the
    heap's: 7 per level), which keeps the scene within the 24 entries the fused path kernel's cached camera pass has LDS for."""
    (t_inner, packets, shading, vn, vt), bmin, bmax = _teapot_arrays()
    assert 1 <= fertile <= 8 and n_filler >= 1
    nt = t_inner.shape[0]
    inner = np.zeros((1 + n_filler + nt, 128), np.uint8)
    q = inner.view(np.uint16).reshape(-1, 64)[:, :48].reshape(-1, 2, 3, 8)  # [node][min / max][axis][slot] (a view: the last axis split)
    assert np.shares_memory(q, inner)
    link = inner.view(np.uint32).reshape(-1, 32)[:, 24:]
    # the new root: slot 0 = one step at the min corner -> the filler, slot 1 = the full range -> the teapot
    link[0] = NULL
    q[0, 0, :, 0], q[0, 1, :, 0] = 0, 1
    q[0, 0, :, 1], q[0, 1, :, 1] = 0, 65535
    link[0, 0] = 1 << 3
    link[0, 1] = (1 + n_filler) << 3
    # the filler: every box the full range
    q[1:1 + n_filler, 1] = 65535
    link[1:1 + n_filler] = _filler_links(n_filler, fertile)
    # the teapot's nodes behind the filler: inner links move by 1 + n_filler nodes, leaf links stay
    inner[1 + n_filler:] = t_inner
    tl = link[1 + n_filler:]
    moved = (tl != NULL) & ((tl & 7) == 0)
    tl[moved] += np.uint32((1 + n_filler) << 3)
    return inner, packets, shading, vn, vt, 0, bmin, bmax


def grafted_host(n_filler, fertile=8, ctx=None):
    return mp.TriangleBvh.from_arrays(*grafted_arrays(n_filler, fertile), ctx=ctx)


@functools.lru_cache(maxsize=None)
def top_filler_size(fertile=8):
    """The largest filler whose scene still gets the 16-slot packet tree, searched on host-only scenes (the callers assert what
    they need of n and n + 1).  Starts where the packet tree fits whatever is absorbed -- it has at most the reference's
    1 + n + 27 nodes --, doubles the step until the export has 8 slots, then bisects."""
    def slots(n):
        return grafted_host(n, fertile).device_tree(packet=True)[0].shape[1]

    lo = (1 << 16) - 2 - (1 + _teapot_arrays()[0][0].shape[0])
    assert slots(lo) == 16
    step = 64
    while slots(lo + step) == 16:
        lo, step = lo + step, 2 * step
        assert step < (1 << 20)
    hi = lo + step  # 16 slots at lo, 8 at hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if slots(mid) == 16 else (lo, mid)
    return lo


def corner_camera(bmin, bmax, distance=5.0):
    """A camera just outside the scene's min corner that looks into the filler's box -- one quantisation step of the scene's box,
    a ten-thousandth of a unit on the teapot -- from `distance` box diagonals away: a pinhole (f/1e6: the default lens is fifty
    times wider than the box), all directions of one sign pattern.  The box fills about the middle third of the frame."""
    bmin, bmax = np.asarray(bmin, np.float64), np.asarray(bmax, np.float64)
    step = (bmax - bmin) / 65535.0
    at = bmin + 0.5 * step
    eye = at - distance * np.linalg.norm(step) * np.array([0.66, 0.45, 0.6])
    return mp.Camera.default().look_at(tuple(float(v) for v in eye), tuple(float(v) for v in at), (0.0, 1.0, 0.0)).f_number(1e6)


# ---- a numpy model of the cached walk's node table ----------------------------------------------------------------------------------

def _analytic_bounds():
    import sys

    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import analytic_bounds as ab
    return ab


class LeafTriangles:
    """the triangles of a leaf link of an exported tree, decompressed as tests/test_packet_tree_cpu.py does, and one plain numpy
    triangle test for a bundle of rays (it decides nothing about parity with the reference: the model's walks share it)"""

    def __init__(self, host):
        lit = host.device_tree(literal=True)[0]
        link = lit[:, :, 6]
        leaf = (link != NULL) & ((link & 63) != 0)
        self.box = dict(zip(link[leaf].tolist(), lit[:, :, :6][leaf].view(np.float32)))
        self.pk16 = host.export()[1].copy().view(np.uint16).reshape(-1, 3, 3, 8)
        self.cache = {}

    def nearest(self, link, o, d):
        """closest accepted distance of every ray (o, d: [rays, 3]) in the leaf, inf where none"""
        F = np.float32
        if link not in self.cache:
            first, nreal = link >> 6, link & 63
            box = self.box[link]
            mn, size = box[:3], (box[3:] - box[:3]).astype(F)
            npk = (nreal + 7) // 8
            rel = self.pk16[first:first + npk].astype(F) * (F(1) / F(65535))
            p = (np.float64(size)[None, None, :, None] * np.float64(rel) + np.float64(mn)[None, None, :, None]).astype(F)
            p = p.transpose(0, 3, 1, 2).reshape(npk * 8, 3, 3)[:nreal]
            self.cache[link] = (p[:, 0], (p[:, 1] - p[:, 0]).astype(F), (p[:, 2] - p[:, 0]).astype(F))
        v0, e1, e2 = (a[None] for a in self.cache[link])  # [1, tris, 3]
        o, d = o[:, None], d[:, None]
        h = np.cross(d, e2)
        det = (e1 * h).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            invd = 1.0 / det
            s = o - v0
            u = invd * (s * h).sum(-1)
            q = np.cross(s, e1)
            v = invd * (d * q).sum(-1)
            tt = invd * (e2 * q).sum(-1)
            ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (tt >= 0)
        return np.where(ok, tt, np.inf).min(1).astype(F)


def _slab(box, o, inv, limit):
    """aabb.rs:254-284 for one box and a bundle of rays with finite inverse directions: t1 <= t2 per ray"""
    a, c = (box[:3][None] - o) * inv, (box[3:][None] - o) * inv
    lo, hi = np.minimum(a, c), np.maximum(a, c)
    t1 = np.maximum(np.maximum(lo[:, 0], 0), np.maximum(lo[:, 1], lo[:, 2]))
    t2 = np.minimum(np.minimum(hi[:, 0], limit), np.minimum(hi[:, 1], hi[:, 2]))
    return t1 <= t2


def plain_walk(nodes, root, tris, o, d, inv):
    """the reference's walk (ray_bvh_intersection.rs:26-62), every ray of the bundle on its own and no table: best t per ray"""
    F = np.float32
    best = np.full(o.shape[0], np.finfo(F).max, F)
    for r in range(o.shape[0]):
        stack = [(root, F(-np.inf))]
        while stack:
            link, t1 = stack.pop()
            if t1 > best[r]:
                continue
            if link & 63:
                best[r] = min(best[r], tris.nearest(link, o[r:r + 1], d[r:r + 1])[0])
                continue
            recs = nodes[link >> 6]
            recs = recs[recs[:, 6] != NULL]
            if recs.shape[0] == 0:
                continue
            boxes = recs[:, :6].view(F)
            a, c = (boxes[:, :3] - o[r]) * inv[r], (boxes[:, 3:] - o[r]) * inv[r]
            lo, hi = np.minimum(a, c), np.maximum(a, c)
            e1 = np.maximum(np.maximum(lo[:, 0], 0), np.maximum(lo[:, 1], lo[:, 2]))
            e2 = np.minimum(np.minimum(hi[:, 0], best[r]), np.minimum(hi[:, 1], hi[:, 2]))
            stack.extend((int(recs[k, 6]), F(e1[k])) for k in range(recs.shape[0]) if e1[k] <= e2[k])
    return best


def cached_unit_walk(nodes, root, tris, header, passes, node_entries, honour_tags=True):
    """trace_packet_cached's use of the NODE table over one unit: header = (lo, hi, neg) of the unit's bounds B
    (tools/analytic_bounds.py corner_header), passes = [(o, d, inv)] bundles inside B.  A node visit looks the node's slot
    (node & (node_entries - 1)) up; on a miss it computes the mask of the children some ray inside B may pass (box_reject) and
    stores (node, mask); a frame holds the node, its children still to pop (highest first) and the rays live at its visit; a child
    is tested when it is popped, against best.t as it is then.  honour_tags=False takes whatever entry the slot holds: the walk
    that a wrong tag compare would be (a bit of such a mask that names a null slot is skipped: the model must not leave the tree).
    Returns (best t [passes, rays], lookups that found another node's entry in the slot)."""
    ab = _analytic_bounds()
    F = np.float32
    lo, hi, neg = header
    table, evictions, out = {}, 0, []
    for o, d, inv in passes:
        best = np.full(o.shape[0], np.finfo(F).max, F)
        frames = []
        cur = (None, [(np.array([-np.inf] * 3 + [np.inf] * 3, F), root)], np.ones(o.shape[0], bool))  # the root's pseudo-node
        while True:
            node, todo, live = cur
            if not todo:
                if not frames:
                    break
                cur = frames.pop()
                continue
            box, link = todo.pop()  # highest child first
            ok = _slab(box, o, inv, np.where(live, best, F(-1)))
            if not ok.any():
                continue
            if link & 63:
                t = tris.nearest(link, o, d)
                best = np.where(ok & (t < best), t, best).astype(F)
                continue
            child = link >> 6
            slot = child & (node_entries - 1)
            e = table.get(slot)
            evictions += e is not None and e[0] != child
            if e is not None and (e[0] == child or not honour_tags):
                mask = e[1]
            else:
                recs = nodes[child]
                real = recs[:, 6] != NULL
                keep = real & ~ab.box_reject(recs[:, :6].view(F), lo, hi, neg)
                mask = [int(i) for i in np.nonzero(keep)[0]]
                table[slot] = (child, mask)
            kids = [(nodes[child, i, :6].view(F), int(nodes[child, i, 6])) for i in mask if int(nodes[child, i, 6]) != NULL]
            if kids:
                if todo:
                    frames.append((node, todo, live))
                cur = (child, kids, ok)
        out.append(best)
    return np.array(out), evictions


def evict_unit_passes(oracle, unit_index, margin):
    """Unit `unit_index` (row-major) of the eviction frame as the packet kernel walks it at 64 samples per pixel, 16 in flight:
    (header (lo, hi, neg) of mask_cache_begin_unit's corner bounds, the four passes [(o, d, inv)] of 2 x 2 pixels x 16 samples)"""
    from minipath_amd import scenes

    ab = _analytic_bounds()
    res, spp = EVICT_RES, 64
    sarr = scenes.atrium_camera().build_sampler(res).as_array()
    smp = oracle.sampler_from_array(sarr)
    ux, uy = (unit_index % (res[0] // 2)) * 2, (unit_index // (res[0] // 2)) * 2
    state, lo, hi = ab.corner_header(sarr, ab.jitter_scale(), ux, ux + 1, uy, uy + 1, margin)
    assert state != 0xFFFFFFFF, "the corner rays set the unit's bounds"
    neg = np.array([(state >> k) & 1 for k in range(3)], bool)
    passes = []
    for s0 in range(0, spp, 16):
        rays = [oracle.sample_ray(smp, ux + (l // 16) % 2, uy + (l // 16) // 2,
                                  oracle.lib().mpo_sample_key(EVICT_SEED, res[0], spp, ux + (l // 16) % 2, uy + (l // 16) // 2, s0 + l % 16))
                for l in range(64)]
        o, d, inv = (np.array([list(getattr(r, k)) for r in rays], np.float32) for k in ("o", "d", "inv"))
        v = np.stack([o, inv, d])
        assert ((v >= lo[:, None, :]) & (v <= hi[:, None, :])).all() and ((inv < 0) == neg[None]).all(), "no pass leaves the bounds: the table is never cleared"
        passes.append((o, d, inv))
    return (lo, hi, neg), passes
