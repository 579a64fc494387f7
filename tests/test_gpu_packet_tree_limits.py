"""GPU tests (-m gpu) of the cached packet walk (packet_walk.h, trace_packet_cached) where its two word formats can go
wrong without a small scene noticing.  Helpers and constructions: tests/graft_model.py; the premises are asserted on the CPU too
(tests/test_packet_tree_limits_cpu.py).

A. Evictions in the per-unit mask tables (mask_cache.h: the node table direct-mapped on node & (MP_NODE_ENTRIES - 1), the leaf
   table on first packet & (MP_LEAF_ENTRIES - 1)) under both formats: a scene whose two walked trees exceed the node table, on a
   small interior frame.  Before any launch every case asserts, from the oracle's closest hits, that at least five of its kernel's
   units meet two nodes, and five two leaves, that share a slot: an entry that survived its eviction, or a tag compared in the
   wrong bits, culls a child or a triangle that a ray hits.

B. The top of the 16-bit index range and the size fallback: the teapot behind a filler of childless nodes, as many as the format
   just holds (65 534 packet-tree nodes: frame words, stacked frames and table entries of the teapot's nodes have bit 31 set, the
   pseudo-node's word is one below the all-ones tag) and one more (the wide tree with 8-bit masks and 17-bit indices, under the
   default option).  Both on a default context, bit-equal to the oracle over the same arrays and to each other.

Every case names the cached kernel it ran.  The fused path kernel's cached camera pass has LDS for scenes with a traversal-stack
bound of at most 24: the scene of part A (45) cannot reach it under any option and has no such case; in part B the heap-shaped
filler (36) cannot either, so that case runs on a deeper filler with a shallower stack (23), under "paths_pooled" = 0
(tests/test_packet_tree_limits_cpu.py asserts what the plans name for each)."""
import functools

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import scenes
from tests import aov_model
from tests import dispatch_cases as dc
from tests import graft_model as gm
from tests.test_gpu_packet_tree import _check_export, _frame, _options, bits, ctxs  # noqa: F401  (ctxs: the module's fixture)

pytestmark = pytest.mark.gpu


def _planes(ctx, obj, cam, st, which):
    """the feature planes `which` of one frame: ({name: image}, kernels reported)"""
    import torch

    _options(ctx)
    fr = mp.FrameRenderer(mp.Scene(obj), cam, st)
    out = fr.render_aov(**{k: k in which for k in ("shade", "normal", "albedo", "ids")})
    names = dc.launched(ctx)
    img = {k: fr.untile_plane(out[k]).cpu().numpy() for k in which}
    torch.cuda.synchronize()
    return img, names


# ---- A ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def evict_objs(ctxs):
    """the eviction scene on both contexts, built once"""
    return {slots: mp.TriangleBvh.build(*gm.evict_mesh(), ctx) for slots, ctx in ctxs.items()}


def _assert_collisions(oracle, family, objs):
    """the premise, per format, on the tree that format's walk uses"""
    node_entries, _ = gm.mask_table_sizes()
    counted = {}
    for slots, obj in objs.items():
        _check_export(obj, slots)
        tree = obj.device_tree(packet=True)
        assert tree[0].shape[0] > node_entries
        units, node_units, leaf_units = gm.evict_collisions(oracle, family, tree)
        assert node_units >= 5 and leaf_units >= 5, (family, slots, units, node_units, leaf_units)
        counted[slots] = (units, node_units, leaf_units)
    return counted


@functools.lru_cache(maxsize=None)
def _evict_oracle_image(oracle, spp):
    smp = oracle.sampler_from_array(scenes.atrium_camera().build_sampler(gm.EVICT_RES).as_array())
    f, u8, *_ = gm.evict_oracle(oracle).render_image_mt(smp, *gm.EVICT_RES, spp, gm.EVICT_SEED, gm.EVICT_TS, 16)
    return f, u8


@pytest.mark.parametrize("family,s_in_flight", [("packet, 16 in flight", 16), ("packet, 4 in flight", 4)])
def test_packet_kernel_evicts_table_entries(ctxs, evict_objs, oracle, family, s_in_flight):
    spp = gm.EVICT_FAMILIES[family][0]
    counted = _assert_collisions(oracle, family, evict_objs)
    # counted (units, node-slot, leaf-slot): 16 in flight {16: (1536, 14, 45), 8: (1536, 19, 45)}; 4 in flight {16: (384, 7, 50), 8: (384, 11, 50)}
    assert counted[16][0] == counted[8][0] == gm.EVICT_RES[0] * gm.EVICT_RES[1] * s_in_flight // 64
    of, ou8 = _evict_oracle_image(oracle, spp)
    assert np.count_nonzero(of[..., 3]) > of.shape[0] * of.shape[1] // 2
    got = {}
    for slots, ctx in ctxs.items():
        f, u8, names, _ = _frame(ctx, evict_objs[slots], scenes.atrium_camera(), mp.RenderSettings(gm.EVICT_TS, spp, gm.EVICT_RES, seed=gm.EVICT_SEED))
        assert names == [f"render_tiles_packet_kernel<{s_in_flight}, false, 8, false, true>"], (slots, names)
        diff = int(np.sum(bits(f) != bits(of)))
        assert diff == 0 and np.array_equal(u8, ou8), (slots, diff)
        got[slots] = f
    assert np.array_equal(bits(got[16]), bits(got[8]))


def test_feature_plane_kernel_evicts_table_entries(ctxs, evict_objs, oracle):
    family = "feature planes, 4 in flight"
    spp = gm.EVICT_FAMILIES[family][0]
    _assert_collisions(oracle, family, evict_objs)  # counted (units, node-slot, leaf-slot): {16: (384, 7, 50), 8: (384, 11, 50)}
    smp = oracle.sampler_from_array(scenes.atrium_camera().build_sampler(gm.EVICT_RES).as_array())
    want = aov_model.planes(oracle, gm.evict_oracle(oracle).intersect, smp, gm.EVICT_RES[0], spp, gm.EVICT_SEED, (0, 0, *gm.EVICT_RES))
    assert np.count_nonzero(want["ids"][..., 3]) > gm.EVICT_RES[0] * gm.EVICT_RES[1] // 2
    which = ("ids", "albedo", "normal")  # normal = {n.xyz, depth}
    got = {}
    for slots, ctx in ctxs.items():
        img, names = _planes(ctx, evict_objs[slots], scenes.atrium_camera(), mp.RenderSettings(gm.EVICT_TS, spp, gm.EVICT_RES, seed=gm.EVICT_SEED), which)
        assert names == ["render_aov_packet_kernel<4, false, 8, false, true>"], (slots, names)
        for k in which:
            diff = int(np.sum(bits(img[k]) != bits(want[k])))
            assert diff == 0, (slots, k, diff)
        got[slots] = img
    for k in which:
        assert np.array_equal(bits(got[16][k]), bits(got[8][k]))


# ---- B ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def graft_objs(ctxs):
    """{0: the scene with the largest filler that keeps the packet tree, 1: one filler node more}, on the default-option context,
    with what their exports must be"""
    n = gm.top_filler_size()  # (found: 66 440)
    objs = {extra: gm.grafted_host(n + extra, ctx=ctxs[16]) for extra in (0, 1)}
    assert all(o.packet_tree_slots == 16 for o in objs.values())
    pk = objs[0].device_tree(packet=True)
    assert pk[0].shape == ((1 << 16) - 2, 16, 8)
    chains = gm.Chains(pk[0], pk[1], objs[0].info().packet_count)
    assert chains.node_of.min() >= (1 << 15) and chains.node_of.max() == pk[0].shape[0] - 1
    fk, wide = objs[1].device_tree(packet=True), objs[1].device_tree()
    assert fk[0].shape == wide[0].shape and fk[0].shape[1] == 8 and fk[0].shape[0] + 1 >= (1 << 16) and fk[0].tobytes() == wide[0].tobytes()
    return objs


@functools.lru_cache(maxsize=None)
def _graft_oracle(oracle, extra):
    return oracle.Bvh.from_arrays(*gm.grafted_arrays(gm.top_filler_size() + extra))


@pytest.mark.parametrize("spp,s_in_flight", [(16, 4), (64, 16)])
def test_packet_kernel_at_the_top_of_the_index_range(ctxs, graft_objs, oracle, spp, s_in_flight):
    res, ts, seed = dc.RES, dc.TS, 21
    smp = oracle.sampler_from_array(mp.Camera.teapot_view().build_sampler(res).as_array())
    got = {}
    for extra, obj in graft_objs.items():
        of, ou8, *_ = _graft_oracle(oracle, extra).render_image_mt(smp, *res, spp, seed, ts, 16)
        assert 0.0 < of[..., 3].mean() < 1.0, "hits and misses in view"
        f, u8, names, _ = _frame(ctxs[16], obj, mp.Camera.teapot_view(), mp.RenderSettings(ts, spp, res, seed=seed))
        assert len(names) == 1 and names[0].endswith(", true>"), names
        assert names == [f"render_tiles_packet_kernel<{s_in_flight}, false, 8, false, true>"], names
        diff = int(np.sum(bits(f) != bits(of)))
        assert diff == 0 and np.array_equal(u8, ou8), (extra, diff)
        got[extra] = f
    assert np.array_equal(bits(got[0]), bits(got[1]))


def test_feature_planes_at_the_top_of_the_index_range(ctxs, graft_objs, oracle):
    res, ts, spp, seed = dc.RES, dc.TS, 16, 21
    smp = oracle.sampler_from_array(mp.Camera.teapot_view().build_sampler(res).as_array())
    which = ("ids", "albedo")
    got = {}
    for extra, obj in graft_objs.items():
        want = aov_model.planes(oracle, _graft_oracle(oracle, extra).intersect, smp, res[0], spp, seed, (0, 0, *res))
        hit = want["ids"][..., 3] == 1
        assert 0 < hit.sum() < hit.size, "hits and misses in view"
        img, names = _planes(ctxs[16], obj, mp.Camera.teapot_view(), mp.RenderSettings(ts, spp, res, seed=seed), which)
        assert len(names) == 1 and names[0].endswith(", true>"), names
        assert names == ["render_aov_packet_kernel<4, false, 8, false, true>"], names
        for k in which:
            diff = int(np.sum(bits(img[k]) != bits(want[k])))
            assert diff == 0, (extra, k, diff)
        got[extra] = img
    for k in which:
        assert np.array_equal(bits(got[0][k]), bits(got[1][k]))


def test_walk_through_the_childless_filler(ctxs, graft_objs, oracle):
    """A pinhole just outside the scene's min corner that looks into the filler's box: a ray that enters it visits every one of the
    filler's 66 k nodes, and the nodes at the bottom of the heap have no children -- a mask of zero, no frame opened --, under
    both formats; every pass thrashes the node table.  16 x 16 pixels in tiles of 8, 16 samples: 4 096 rays, about 340 of them
    through the filler (the oracle takes about two seconds for them on one thread)."""
    res, ts, spp, seed = (16, 16), 8, 16, 3
    n = gm.top_filler_size()
    cam = gm.corner_camera(*graft_objs[0].get_bounding_box())
    smp = oracle.sampler_from_array(cam.build_sampler(res).as_array())
    got = {}
    for extra, obj in graft_objs.items():
        of, ou8, _, rays, counters = _graft_oracle(oracle, extra).render_image_mt(smp, *res, spp, seed, ts, 16, want_counters=True)
        # (counted: 22.2 M inner-node visits) at least a hundred rays walked the whole filler, and rays hit the teapot behind it
        assert rays == res[0] * res[1] * spp and counters.inner_visited > 100 * n and np.count_nonzero(of[..., 3]) > 0
        f, u8, names, _ = _frame(ctxs[16], obj, cam, mp.RenderSettings(ts, spp, res, seed=seed))
        assert names == ["render_tiles_packet_kernel<4, false, 8, false, true>"], names
        diff = int(np.sum(bits(f) != bits(of)))
        assert diff == 0 and np.array_equal(u8, ou8), (extra, diff)
        got[extra] = f
    assert np.array_equal(bits(got[0]), bits(got[1]))


def test_path_kernel_cached_camera_pass_at_the_top_of_the_index_range(ctxs, oracle):
    """The teapot at depth 2, 32 spp behind the filler with two fertile children per node (68 365 nodes for 65 534 of the packet tree,
    traversal-stack bound 23) and one node more.  The scene is "big": the pooled kernel by default, the fused kernel with its
    cached camera pass (units of four passes of 8) under "paths_pooled" = 0."""
    res, spp, seed, ts, depth = dc.RES, 32, 9, dc.TS, 2
    n = gm.top_filler_size(fertile=2)
    smp = oracle.sampler_from_array(mp.Camera.teapot_view().build_sampler(res).as_array())
    got = {}
    for extra in (0, 1):
        obj = gm.grafted_host(n + extra, fertile=2, ctx=ctxs[16])
        pk = obj.device_tree(packet=True)
        assert pk[0].shape[1:] == ((16, 8) if extra == 0 else (8, 8)) and (pk[0].shape[0] == (1 << 16) - 2 if extra == 0 else pk[0].shape[0] + 1 >= (1 << 16))
        assert gm.Chains(pk[0], pk[1], obj.info().packet_count).node_of.min() >= (1 << 15)
        of, ou8, _, oseg = oracle.Bvh.from_arrays(*gm.grafted_arrays(n + extra, fertile=2)).render_image_paths_mt(smp, *res, spp, seed, depth, ts, 16)
        assert 0.0 < of[..., 3].mean() < 1.0, "hits and misses in view"
        f, u8, names, seg = _frame(ctxs[16], obj, mp.Camera.teapot_view(), mp.RenderSettings(ts, spp, res, seed=seed, max_depth=depth), paths_pooled=0)
        assert names == ["render_paths_kernel<8, false, false, true>"], (extra, names)
        diff = int(np.sum(bits(f) != bits(of)))
        assert diff == 0 and np.array_equal(u8, ou8), (extra, diff)
        assert seg == oseg and seg > res[0] * res[1] * spp
        got[extra] = f
    assert np.array_equal(bits(got[0]), bits(got[1]))
