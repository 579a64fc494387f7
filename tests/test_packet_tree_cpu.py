"""CPU tests of the PACKET tree (minipath_amd/csrc/device_tree.cpp; mp_scene_device_tree which = 2): the tree the cached packet
walk uses -- the wide tree's absorption of FP-nested thin nodes carried on to sixteen slots per node.

Checked here without a GPU, on host-only scenes: structure (at most 16 real children, null links only behind the last real child,
children behind their parent, the root's pseudo-record), the leaf sequence against the literal tree, the floating-point containment
of every absorbed reference node on the exported floats, node accounting, and -- with a numpy model of the reference's
explicit-stack walk run on the literal, wide and packet trees -- the same leaf sequence and the same closest distance, bit for bit,
for rays with finite inverse directions, rays that graze box planes included.  The 8-slot fallback (Context option
"packet_tree_slots" = 8) needs a context and is checked on the GPU (tests/test_gpu_packet_tree.py); here, the wide and literal
exports must not depend on the packet export.  (The model's triangle test is plain numpy: it decides
nothing about parity with the reference, only whether the trees are equivalent under one and the same test.)"""
import ctypes as C
import functools

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib, scenes
from tests import graft_model, meshes
from tests.conftest import TEAPOT

NULL = 0xFFFFFFF8
F = np.float32
# the stand-in at a small detail (thin binary top, non-nestable nodes: asserted below), the teapot, two meshes (`doubled`: exact ties)
SCENES = ["teapot", "atrium:0.1", "soup_5000", "grid_40+doubled"]
# ... and the teapot behind a filler of childless nodes (tests/graft_model.py), as many as the 16-bit format just holds: 65 534 nodes
# of the packet tree, the teapot's leaves in the last of them
GRAFT = "graft"


@functools.lru_cache(maxsize=None)
def _host(name):
    if name == "teapot":
        return mp.TriangleBvh.with_obj(TEAPOT)
    if name == GRAFT:
        return graft_model.grafted_host(graft_model.top_filler_size())
    if name.startswith("atrium"):
        return mp.TriangleBvh.build(*scenes.atrium(1, float(name.split(":")[1])))
    base, _, mod = name.partition("+")
    pos, nrm, tex, tri = meshes.doubled(base)[:4] if mod == "doubled" else meshes.make(base)
    return mp.TriangleBvh.build(pos, nrm, tex, tri)


@functools.lru_cache(maxsize=None)
def _trees(name):
    """{kind: (nodes, root, stack bound, absorbed)} -- exported once per scene and shared; nobody writes to them"""
    h = _host(name)
    out = {"lit": h.device_tree(literal=True), "wide": h.device_tree(), "packet": h.device_tree(packet=True)}
    for t in out.values():
        t[0].setflags(write=False)
    return out


def _slots(nodes, n):
    """real slots of device node n: list of (box f32[6], link)"""
    return [(nodes[n, i, :6].view(F), int(nodes[n, i, 6])) for i in range(nodes.shape[1]) if int(nodes[n, i, 6]) != NULL]


def _leaf_order(nodes, root):
    """leaf links in the order a full DFS (children pushed ascending, popped descending) reaches them"""
    if root == NULL:
        return []
    if root & 63:
        return [root]
    seq, stack = [], [root]
    while stack:
        link = stack.pop()
        if link & 63:
            seq.append(link)
            continue
        stack.extend(l for _, l in _slots(nodes, link >> 6))
    return seq


def _subtree_signatures(nodes, root):
    """{node index: (first terminal in ascending-child order, number of terminals)}.  A terminal is a leaf, named by its link, or a
    node without children (the filler of the grafted scene), named by its place among such nodes in a depth-first walk in
    ascending-child order: absorption keeps that order, so the name is the same on every tree."""
    first, count, order, stack = {}, {}, [], [root >> 6]
    while stack:
        n = stack.pop()
        order.append(n)
        stack.extend(l >> 6 for _, l in reversed(_slots(nodes, n)) if (l & 63) == 0)
    empties = 0
    for n in order:  # pre-order, children ascending
        if not _slots(nodes, n):
            first[n], count[n] = ("childless", empties), 1
            empties += 1
    for n in reversed(order):
        if n in first:
            continue
        f, c = None, 0
        for _, l in _slots(nodes, n):
            lf, lc = (l, 1) if l & 63 else (first[l >> 6], count[l >> 6])
            f = lf if f is None else f
            c += lc
        first[n], count[n] = f, c
    return first, count


@pytest.mark.parametrize("name", SCENES + [GRAFT])
def test_packet_tree_structure_and_containment(name):
    host, t = _host(name), _trees(name)
    pk, proot, pbound, absorbed, _ = t["packet"]
    lit, lroot, _, _ = t["lit"]
    wide, _, _, wabsorbed = t["wide"]
    assert pk.shape[1:] == (16, 8) and lit.shape[1:] == (8, 8) and wide.shape[1:] == (8, 8)
    assert lit.shape[0] > 0 and (proot & 63) == 0
    # count + absorbed = the reference's inner nodes; the packet tree goes on where the wide tree stops
    assert pk.shape[0] + absorbed == host.info().inner_count == lit.shape[0]
    assert absorbed >= wabsorbed and pk.shape[0] <= wide.shape[0]
    real = pk[:, :, 6] != NULL
    # at most 16 real children (the shape), at least two, null links only behind the last real child, n = their number
    assert np.all(real[:, :-1] >= real[:, 1:])
    assert np.array_equal(pk[:, 0, 7], real.sum(1))
    if name == GRAFT:  # the nodes at the bottom of the filler's heap have no children at all and are never absorbed: the literal tree's
        assert np.all((real.sum(1) >= 2) | (real.sum(1) == 0))
        assert (real.sum(1) == 0).sum() == ((lit[:, :, 6] != NULL).sum(1) == 0).sum() > pk.shape[0] // 2
    else:
        assert np.all(real.sum(1) >= 2)
    # unused slots are zero boxes
    assert not pk[:, :, :6][~real].any()
    # children have larger indices than their parent, every node but the root has exactly one parent: pre-order numbering
    inner = real & ((pk[:, :, 6] & 63) == 0)
    child = (pk[:, :, 6] >> 6)[inner]
    parent = np.broadcast_to(np.arange(pk.shape[0])[:, None], inner.shape)[inner]
    assert np.all(child > parent) and proot == 0
    assert np.array_equal(np.sort(child), np.arange(1, pk.shape[0]))
    first_inner = [next((l >> 6 for _, l in _slots(pk, n) if (l & 63) == 0), None) for n in range(pk.shape[0])]
    assert all(c is None or c == n + 1 for n, c in enumerate(first_inner))  # a node's first subtree follows it
    # same leaves in the same order as the literal tree
    assert _leaf_order(pk, proot) == _leaf_order(lit, lroot)
    # every reference node that is no longer a node of its own has all its child boxes FP-contained in its own box: checked on the
    # exported floats of the literal tree, the node identified by (first leaf, leaf count, box bytes)
    pfirst, pcount = _subtree_signatures(pk, proot)
    lfirst, lcount = _subtree_signatures(lit, lroot)
    kept = {(pfirst[l >> 6], pcount[l >> 6], box.tobytes()) for n in range(pk.shape[0]) for box, l in _slots(pk, n) if (l & 63) == 0}
    gone = not_nestable = 0
    for n in range(lit.shape[0]):
        for box, l in _slots(lit, n):
            if l & 63:
                continue
            c = l >> 6
            nested = bool(np.all(box[:3] <= box[3:])) and all(
                np.all(cb[:3] <= cb[3:]) and np.all(box[:3] <= cb[:3]) and np.all(cb[3:] <= box[3:]) for cb, _ in _slots(lit, c))
            not_nestable += not nested
            if (lfirst[c], lcount[c], box.tobytes()) in kept:
                continue
            gone += 1
            assert nested, (n, c)
    assert gone == absorbed
    # every box of the packet tree is a box of the literal tree (the same floats), attached to the same leaf / subtree
    lit_boxes = {(l if l & 63 else (lfirst[l >> 6], lcount[l >> 6]), box.tobytes()) for n in range(lit.shape[0]) for box, l in _slots(lit, n)}
    for n in range(pk.shape[0]):
        for box, l in _slots(pk, n):
            assert (l if l & 63 else (pfirst[l >> 6], pcount[l >> 6]), box.tobytes()) in lit_boxes
    if name.startswith("atrium"):
        # the stand-in keeps what the packet tree is for and what it must not touch at this detail: a thin top (2-child nodes of the
        # literal tree that the wide tree cannot absorb for want of slots) and nodes that are not FP-nested
        assert not_nestable > 0
        assert absorbed > wabsorbed and (real.sum(1) > 8).any()
        assert (lit[:, 0, 7] == 2).sum() > (pk[:, 0, 7] == 2).sum()
    assert pbound >= 1


@pytest.mark.parametrize("name", SCENES + [GRAFT])
def test_root_pseudo_record(name):
    """The record behind the last node (record count * slots) is the root's: an unbounded box, which every ray passes with t1 = 0,
    and the root's link.  The cached walk starts there: child 0 of pseudo-node `count`, which the 16-bit format must hold."""
    pk, proot, _, _, rec = _trees(name)["packet"]
    assert pk.shape[0] + 1 < (1 << 16)
    assert np.array_equal(rec[:6].view(F), np.array([-np.inf] * 3 + [np.inf] * 3, F))
    assert int(rec[6]) == proot == 0  # node 0 << 6


@pytest.mark.parametrize("name", SCENES + [GRAFT])
def test_other_exports_do_not_move(name):
    """which = 0 / 1 after the packet export: the arrays of before.  (The fallback -- "packet_tree_slots" = 8: the export is the wide
    tree byte for byte -- needs a context to set the option on: tests/test_gpu_packet_tree.py.)"""
    host, t = _host(name), _trees(name)
    for kind, again in (("wide", host.device_tree()), ("lit", host.device_tree(literal=True))):
        assert again[0].tobytes() == t[kind][0].tobytes() and again[1:] == t[kind][1:]
    n = C.c_uint32()
    with pytest.raises(Exception):
        _lib.check(_lib.lib().mp_scene_device_tree(host.handle, 3, None, C.byref(n), None, None, None))


def _walk(nodes, root, tris_of, o, d, inv, childless=None):
    """the reference's walk (ray_bvh_intersection.rs:26-62) on a device-format tree: (leaf sequence, best t, deepest stack);
    childless: a list that receives the visited nodes without children"""
    best = np.finfo(F).max
    stack = [(root, F(-np.inf))]
    seq, deepest = [], 1
    while stack:
        link, t1 = stack.pop()
        if t1 > best:
            continue
        if link & 63:
            seq.append(link)
            t = tris_of(link, o, d)
            if t < best:
                best = t
            continue
        sl = _slots(nodes, link >> 6)
        if not sl:  # a node without children (the grafted scene's filler): visited, nothing pushed
            if childless is not None:
                childless.append(link >> 6)
            continue
        boxes = np.array([b for b, _ in sl], F)
        a = (boxes[:, :3] - o) * inv
        c = (boxes[:, 3:] - o) * inv
        lo, hi = np.minimum(a, c), np.maximum(a, c)
        e1 = np.maximum(np.maximum(lo[:, 0], 0), np.maximum(lo[:, 1], lo[:, 2]))
        e2 = np.minimum(np.minimum(hi[:, 0], best), np.minimum(hi[:, 1], hi[:, 2]))
        for k, (_, l) in enumerate(sl):
            if e1[k] <= e2[k]:
                stack.append((l, F(e1[k])))
        deepest = max(deepest, len(stack))
    return seq, best, deepest


@pytest.mark.parametrize("name", SCENES + [GRAFT])
def test_walk_reaches_the_same_leaves_on_all_three_trees(name):
    host, t = _host(name), _trees(name)
    lit, lroot, lbound, _ = t["lit"]
    info = host.info()
    bmin, bmax = np.array(list(info.bbox_min), F), np.array(list(info.bbox_max), F)
    _, packets, *_ = host.export()
    pk16 = packets.copy().view(np.uint16).reshape(-1, 3, 3, 8)
    leaf_box = {l: box for n in range(lit.shape[0]) for box, l in _slots(lit, n) if l & 63}
    cache = {}

    def tris_of(link, o, d):
        if link not in cache:
            first, nreal = link >> 6, link & 63
            box = leaf_box[link]
            mn, size = box[:3], (box[3:] - box[:3]).astype(F)
            npk = (nreal + 7) // 8
            rel = pk16[first:first + npk].astype(F) * (F(1) / F(65535))
            p = (np.float64(size)[None, None, :, None] * np.float64(rel) + np.float64(mn)[None, None, :, None]).astype(F)
            p = p.transpose(0, 3, 1, 2).reshape(npk * 8, 3, 3)[:nreal]
            cache[link] = (p[:, 0], (p[:, 1] - p[:, 0]).astype(F), (p[:, 2] - p[:, 0]).astype(F))
        v0, e1, e2 = cache[link]
        h = np.cross(d, e2)
        det = (e1 * h).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            invd = 1.0 / det
            s = o - v0
            u = invd * (s * h).sum(-1)
            q = np.cross(s, e1)
            v = invd * (d * q).sum(-1)
            tt = invd * (e2 * q).sum(-1)
            ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (tt >= 0)
        return F(np.where(ok, tt, np.inf).min())

    rng = np.random.default_rng(11)
    ext = bmax - bmin
    n = 160
    o = (bmin - 0.2 * ext + rng.random((n, 3)) * ext * 1.4).astype(F)
    d = rng.standard_normal((n, 3)).astype(F)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    planes = lit[:, :, :6].view(F).reshape(-1, 6)
    planes = planes[np.isfinite(planes).all(1) & (lit[:, :, 6].reshape(-1) != NULL)]
    if name == GRAFT:
        # the rays of this part are aimed at the teapot's boxes; a box that touches the filler's corner box (the root's slot 0) would
        # send its rays through all 66 k filler nodes: those are the bundle's below
        corner = lit[0, 0, :6].view(F)
        planes = planes[~(planes[:, :3] <= corner[3:]).all(1)]
        assert planes.shape[0] > 100
    for k in range(0, 80):
        b = planes[rng.integers(0, planes.shape[0])]
        if k < 40:
            # origin on a corner of a box: entry distances of 0 and ties
            o[k] = b[:3] if k % 2 else b[3:]
        else:
            # a ray that runs inside a box plane (grazes it): the origin's and the target's coordinate on one axis are the plane's,
            # the direction's component there is tiny but not zero (finite inverse)
            ax = k % 3
            tgt = (b[:3] + rng.random(3).astype(F) * (b[3:] - b[:3])).astype(F)
            tgt[ax] = b[ax + 3 * (k % 2)]
            o[k, ax] = tgt[ax]
            dd = (tgt - o[k]).astype(F)
            dd[ax] = F(1e-30) if k % 4 < 2 else F(-1e-30)
            nn = np.linalg.norm(dd)
            d[k] = dd / nn if nn > 0 else d[k]
    d = np.where(d == 0, F(1e-30), d).astype(F)
    with np.errstate(over="ignore"):
        inv = (F(1) / d).astype(F)
    keep = np.isfinite(inv).all(1)
    assert keep.sum() >= n - 8
    visited = absorbed_steps = 0
    for k in np.nonzero(keep)[0]:
        ls, lt, ld = _walk(lit, lroot, tris_of, o[k], d[k], inv[k])
        assert ld <= lbound
        for kind in ("wide", "packet"):
            nodes, root, bound = t[kind][:3]
            s, bt, deep = _walk(nodes, root, tris_of, o[k], d[k], inv[k])
            assert s == ls, (kind, k)
            assert np.array_equal(np.array([bt], F).view(np.uint32), np.array([lt], F).view(np.uint32)), (kind, k)
            assert deep <= bound
        visited += len(ls)
    assert visited > 50  # the rays do reach leaves
    if name != GRAFT:
        return
    # a bundle into the filler's corner box, from outside the scene and from inside it: every tree visits the same nodes without
    # children -- none of them is ever absorbed --, in the same order up to their numbering, and then the teapot's leaves as the others do
    n_filler = graft_model.top_filler_size()
    tgt = (corner[:3].astype(np.float64) + corner[3:].astype(np.float64)) / 2
    for toward in (np.array([0.66, 0.45, 0.6]), np.array([-0.5, -0.62, -0.6])):
        ob = (tgt - toward * (0.3 if toward[0] > 0 else -0.1) * float(ext.max())).astype(F)
        db = (tgt - ob.astype(np.float64)).astype(F)
        db /= np.linalg.norm(db)
        ib = (F(1) / db).astype(F)
        assert np.isfinite(ib).all()
        seen = {}
        for kind in ("lit", "wide", "packet"):
            nodes, root, bound = t[kind][:3]
            seen[kind] = []
            s, bt, deep = _walk(nodes, root, tris_of, ob, db, ib, seen[kind])
            assert deep <= bound
            if kind == "lit":
                ls, lt = s, bt
            assert s == ls and np.array_equal(np.array([bt], F).view(np.uint32), np.array([lt], F).view(np.uint32)), kind
        counts = {k: len(v) for k, v in seen.items()}
        assert counts["lit"] == counts["wide"] == counts["packet"] > n_filler // 2, counts
        assert len(set(seen["packet"])) == counts["packet"] and max(seen["packet"]) > (1 << 15)
