"""CPU tests of the cached packet walk's per-unit child lists on the numpy model (tests/unit_list_model.py), over exported trees of
both formats (TriangleBvh.device_tree: the 16-slot packet tree and the wide tree) and the oracle's rays: units of 2 x 2 pixels x
16 samples, four passes each, under the corner bounds mask_cache_begin_unit gives them.

For every unit: best.t of the list walk is bit-equal to the mask walk's (the walk before the lists), to the reference's per-ray walk
(graft_model.plain_walk) and to the C oracle's (Bvh.trace over the same scene): the model's triangle test is the oracle's own
(unit_list_model.ExactTriangles: the reference's decompression and pyoracle.tri8_intersect), so a miss (FLT_MAX) and every hit
distance carry the reference's bits; the leaf visits come in the mask walk's order; every absorbed node's kept children are
FP-nested in its box; and with a table of four slots and an arena of 32 entries -- lists that do not fit, resets, passes left to
the uncached walk -- the results stay the same.

Coverage floors, a quarter of what the model counts on these units (ATRIUM_UNITS: 38 units spread over the eviction frame; packet
tree / wide tree):
    entries that stand in for a node at least two absorbed levels down     542 / 547   (floor 135; deepest: 5 / 8 levels)
    kept inner children left unexpanded because a kept child sticks out     17 / 21     (floor 4)
    table evictions with four slots                                          8 / 8      (floor 2)
    arena resets with 32 entries, each with a pass left to the uncached walk 20 / 20    (floor 5)
    absorptions refused for want of room, 32 entries                        40 / 44     (floor 10)
(53 / 57 lists for the 38 units, the longest 98 entries: the shipped arena of 384 is never reset on them.)
The teapot (18 packet-tree and 27 wide-tree nodes) has none of these: its units are the plain case."""
import functools

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import scenes
from tests import graft_model as gm
from tests import unit_list_model as ul
from tests.conftest import TEAPOT

F = np.float32
ATRIUM_UNITS = tuple(range(7, 1536, 41))
TEAPOT_RES, TEAPOT_SEED = (64, 48), 21
TEAPOT_UNITS = tuple(range(5, 768, 31))
TINY = (32, 3)  # arena entries, slot mask: the `lists_tiny` build of the library (minipath_amd/csrc/Makefile)


@functools.lru_cache(maxsize=None)
def teapot_host():
    return mp.TriangleBvh.with_obj(TEAPOT)


def scene(name, oracle):
    """(host scene, oracle scene, sampler array, resolution, seed, units)"""
    if name == "atrium":
        return (gm.evict_host(), gm.evict_oracle(oracle), scenes.atrium_camera().build_sampler(gm.EVICT_RES).as_array(), gm.EVICT_RES,
                gm.EVICT_SEED, ATRIUM_UNITS)
    return (teapot_host(), oracle.Bvh.from_obj(TEAPOT), mp.Camera.teapot_view().build_sampler(TEAPOT_RES).as_array(), TEAPOT_RES,
            TEAPOT_SEED, TEAPOT_UNITS)


@functools.lru_cache(maxsize=None)
def exact_triangles(oracle, name):
    """one per scene: its results are shared by the walks of both trees"""
    return ul.ExactTriangles(scene(name, oracle)[0], oracle)


def tree(host, kind):
    return (host.device_tree(packet=True) if kind == "packet" else host.device_tree())[:2]


@functools.lru_cache(maxsize=None)
def _walks(oracle, name, kind):
    """every unit's passes walked four ways, once: [(unit, passes, mask best, mask leaf order, list best, list order, tiny best,
    tiny order)], the list walk's stats and the tiny walk's"""
    host, _, sarr, res, seed, units = scene(name, oracle)
    nodes, root = tree(host, kind)
    assert nodes.shape[1] == (16 if kind == "packet" else 8)
    tris = exact_triangles(oracle, name)
    entries, arena = ul.header_sizes()
    full, tiny, rows = ul.new_stats(), ul.new_stats(), []
    for u in units:
        up = ul.unit_passes(oracle, sarr, res, 64, seed, u, ul.shipped_margin())
        if up is None:
            continue
        header, passes = up
        mb, mo, _ = ul.mask_unit_walk(nodes, root, tris, header, passes)
        lb, lo, full = ul.list_unit_walk(nodes, root, tris, header, passes, entries, arena, stats=full)
        tb, to, tiny = ul.list_unit_walk(nodes, root, tris, header, passes, entries, TINY[0], TINY[1], stats=tiny)
        rows.append((u, header, passes, mb, mo, lb, lo, tb, to))
    return rows, full, tiny


CASES = [(n, k) for n in ("atrium", "teapot") for k in ("packet", "wide")]


@pytest.mark.parametrize("name,kind", CASES)
def test_list_walk_equals_the_mask_walk_and_the_reference(oracle, name, kind):
    host, orc, *_ = scene(name, oracle)
    nodes, root = tree(host, kind)
    tris = exact_triangles(oracle, name)
    rows, full, _ = _walks(oracle, name, kind)
    assert len(rows) >= 20
    fmax = np.finfo(F).max
    for i, (u, header, passes, mb, mo, lb, lo, _, _) in enumerate(rows):
        assert np.array_equal(lb.view(np.uint32), mb.view(np.uint32)), (u, "best.t differs from the mask walk's")
        assert lo == mo, (u, "leaf visit order")
        ot = np.array([orc.trace(o, d)[0] for o, d, _ in passes])
        assert np.array_equal(ot.view(np.uint32), lb.view(np.uint32)), (u, "best.t differs from the oracle's")
        if i % 6 == 0:  # the model's mask walk is graft_model's, and both are the reference's per-ray walk
            plain = np.array([gm.plain_walk(nodes, root, tris, *p) for p in passes])
            assert np.array_equal(plain.view(np.uint32), lb.view(np.uint32)), u
            tagged, _ = gm.cached_unit_walk(nodes, root, tris, header, passes, 1 << 20)
            assert np.array_equal(tagged.view(np.uint32), mb.view(np.uint32)), u
    assert full["resets"] == 0 and full["abandoned"] == 0, "the shipped arena holds these units' lists"
    print(name, kind, {k: v for k, v in full.items() if k != "absorbed_boxes"})


@pytest.mark.parametrize("name,kind", CASES)
def test_absorbed_children_are_nested(oracle, name, kind):
    _, full, tiny = _walks(oracle, name, kind)
    assert full["absorbed"] > 0
    for st in (full, tiny):
        for pbox, g in st["absorbed_boxes"]:
            assert g.shape[0] >= 1 and (pbox[None, :3] <= g[:, :3]).all() and (g[:, 3:] <= pbox[None, 3:]).all()


@pytest.mark.parametrize("name,kind", CASES)
def test_tiny_arena_and_table_keep_the_results(oracle, name, kind):
    rows, _, tiny = _walks(oracle, name, kind)
    walked = 0
    for u, _, _, mb, mo, _, _, tb, to in rows:
        assert np.array_equal(tb.view(np.uint32), mb.view(np.uint32)), u
        for a, b in zip(mo, to):
            assert b is None or a == b, (u, "leaf visit order")
            walked += b is not None
    assert walked >= 2 * len(rows), "most passes still walk lists"
    assert tiny["longest"] <= TINY[0]
    print(name, kind, {k: v for k, v in tiny.items() if k != "absorbed_boxes"})


@pytest.mark.parametrize("kind", ["packet", "wide"])
def test_coverage_floors_on_the_atrium(oracle, kind):
    _, full, tiny = _walks(oracle, "atrium", kind)
    assert full["max_level"] >= 2 and full["two_level_entries"] >= 135, full["two_level_entries"]
    assert full["not_nested"] >= 4, full["not_nested"]
    assert tiny["evictions"] >= 2, tiny["evictions"]
    assert tiny["resets"] >= 5 and tiny["abandoned"] >= 5 and tiny["room_stops"] >= 10, (tiny["resets"], tiny["abandoned"], tiny["room_stops"])
