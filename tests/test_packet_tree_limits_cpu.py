"""CPU tests of the premises of tests/test_gpu_packet_tree_limits.py, on host-only scenes (helpers: tests/graft_model.py):

- the end of the 16-bit word format (device_tree.cpp, packet_tree_applies: `packet.count + 1 < 2^16`, restated by
  TriangleBvh.device_tree to shape the export): the grafted scene with the largest filler that still gets the packet tree has
  exactly 65 534 nodes -- the pseudo-node's word is 65 534 << 16 | 1, one below the all-ones tag --, one filler node more falls
  back to the wide tree under the default option; the teapot's leaves sit in nodes with bit 15 set (bit 31 of the words);
- the launch plans (launch_plan.cpp through tests/plan_probe.py) name the cached kernels for the frames the GPU tests render;
- on the eviction frame every kernel family's units meet nodes and leaves that share a table slot, under both trees.
- and the frame can tell: on a numpy model of the walk's node table a walk that ignored the tags changes rays' closest distances.
The structure, containment and walk-equivalence checks of the grafted scene are tests/test_packet_tree_cpu.py's ("graft")."""
import numpy as np
import pytest

from tests import graft_model as gm
from tests import plan_probe as pp
from tests.test_unit_bounds_cpu import shipped_margin

F = np.float32
TEAPOT_NODES = 27  # the teapot's inner nodes (tests/dispatch_cases.py FACTS)


def _is_root_record(rec, root):
    return np.array_equal(rec[:6].view(F), np.array([-np.inf] * 3 + [np.inf] * 3, F)) and int(rec[6]) == root


def test_the_16_bit_format_holds_65534_nodes_and_no_more():
    n = gm.top_filler_size()  # (found: 66 440)
    top, over = gm.grafted_host(n), gm.grafted_host(n + 1)
    pk, proot, pbound, pabs, rec = top.device_tree(packet=True)
    assert pk.shape == ((1 << 16) - 2, 16, 8) and proot == 0 and _is_root_record(rec, proot)
    assert pk.shape[0] + pabs == top.info().inner_count == 1 + n + TEAPOT_NODES
    assert pbound <= 64  # (counted: 64) the frame stack's registers
    # the last fillers before the end add one packet-tree node each: the end is reached, not jumped over
    assert [gm.grafted_host(k).device_tree(packet=True)[0].shape[:2] for k in range(n - 3, n)] == [((1 << 16) - 5 + i, 16) for i in range(3)]
    # one filler node more: 65 535 nodes would be needed, the pseudo-node's index would be the all-ones tag -- the wide tree, byte for
    # byte, under the default option, with the root's record behind it
    assert over.packet_tree_slots == 16
    fk, froot, fbound, fabs_, frec = over.device_tree(packet=True)
    wide, wroot, wbound, wabs = over.device_tree()
    assert fk.shape == wide.shape == (1 + (n + 1) + TEAPOT_NODES - wabs, 8, 8) and wide.shape[0] + 1 >= (1 << 16)
    assert fk.tobytes() == wide.tobytes() and (froot, fbound, fabs_) == (wroot, wbound, wabs) and _is_root_record(frec, wroot)
    # the wide tree of the scene that keeps the packet tree is one node smaller: the fallback is the packet tree's doing
    assert top.device_tree()[0].shape[0] == wide.shape[0] - 1


def test_teapot_leaves_sit_in_the_top_half_of_the_index_range():
    n = gm.top_filler_size()
    host = gm.grafted_host(n)
    pk, proot, *_ = host.device_tree(packet=True)
    chains = gm.Chains(pk, proot, host.info().packet_count)
    # (counted: nodes 65 517 ... 65 533) every word that names them -- frame, stacked frame, table entry -- has bit 31 set
    assert chains.node_of.min() >= (1 << 15) and chains.node_of.max() == pk.shape[0] - 1 == (1 << 16) - 3
    # ... and so has every node between them and the root's second child: the walk stacks frames of such nodes
    below_root = {c for p in range(chains.node_of.size) for c in chains.chain(int(chains.node_of[p]))[:-1]}
    assert min(below_root) >= (1 << 15)
    # under the fallback the indices need 17 bits
    over = gm.grafted_host(n + 1)
    wide, wroot, *_ = over.device_tree()
    assert gm.Chains(wide, wroot, over.info().packet_count).node_of.max() == wide.shape[0] - 1 >= (1 << 16)


@pytest.mark.parametrize("extra", [0, 1])
def test_plans_of_the_grafted_scene(extra):
    """72 x 40 in tiles of 32 (tests/dispatch_cases.py): the packet and feature-plane kernels are the cached ones.  The path kernel's
    cached camera pass is out of reach of the heap-shaped filler -- the scene is "big", so the default plan is the pooled kernel, and
    with "paths_pooled" = 0 the cached form needs a traversal-stack bound of at most 24 for its LDS (the heap: 36) --; the filler
    with two fertile children per node (stack bound 23, the teapot's own 22 + 1) reaches it."""
    facts = gm.plan_facts(gm.grafted_host(gm.top_filler_size() + extra))
    assert facts["stack_bound"] <= 64 and facts["nodes"] * 256 > (1 << 20)
    assert pp.name(pp.plan(pp.RENDER, pp.launch(facts, 6, 32, 16))) == "render_tiles_packet_kernel<4, false, 8, false, true>"
    assert pp.name(pp.plan(pp.RENDER, pp.launch(facts, 6, 32, 64))) == "render_tiles_packet_kernel<16, false, 8, false, true>"
    assert pp.name(pp.plan(pp.AOV, pp.launch(facts, 6, 32, 16))) == "render_aov_packet_kernel<4, false, 8, false, true>"
    assert pp.name(pp.plan(pp.RENDER, pp.launch(facts, 6, 32, 32, max_depth=2))) == "render_paths_pooled_kernel<4>"
    assert pp.name(pp.plan(pp.RENDER, pp.launch(facts, 6, 32, 32, max_depth=2, pooled=0))) == "render_paths_kernel<8, false, false>"
    deep = gm.plan_facts(gm.grafted_host(gm.top_filler_size(fertile=2) + extra, fertile=2))
    assert deep["stack_bound"] <= 24 and deep["nodes"] * 256 > (1 << 20)
    assert pp.name(pp.plan(pp.RENDER, pp.launch(deep, 6, 32, 32, max_depth=2))) == "render_paths_pooled_kernel<4>"
    assert pp.name(pp.plan(pp.RENDER, pp.launch(deep, 6, 32, 32, max_depth=2, pooled=0))) == "render_paths_kernel<8, false, false, true>"
    assert pp.name(pp.plan(pp.RENDER, pp.launch({**deep, "stack_bound": 25}, 6, 32, 32, max_depth=2, pooled=0))) == "render_paths_kernel<8, false, false>"


def test_the_deep_filler_ends_at_65534_nodes_too():
    """the filler shape of the path kernel's case (two fertile children per node): the same facts at its own n"""
    n = gm.top_filler_size(fertile=2)  # (found: 68 365)
    top, over = gm.grafted_host(n, fertile=2), gm.grafted_host(n + 1, fertile=2)
    pk, proot, *_ = top.device_tree(packet=True)
    assert pk.shape == ((1 << 16) - 2, 16, 8)
    chains = gm.Chains(pk, proot, top.info().packet_count)
    assert chains.node_of.min() >= (1 << 15) and chains.node_of.max() == pk.shape[0] - 1
    fk, wide = over.device_tree(packet=True), over.device_tree()
    assert fk[0].shape == wide[0].shape and fk[0].shape[1] == 8 and fk[0].shape[0] + 1 >= (1 << 16) and fk[0].tobytes() == wide[0].tobytes()
    assert _is_root_record(fk[4], wide[1])


def test_plans_of_the_eviction_frame():
    """96 x 64 in tiles of 32.  As above for the path kernel: this scene's stack bound is 45."""
    facts = gm.plan_facts(gm.evict_host())
    n_tiles = 6
    assert facts["nodes"] > gm.mask_table_sizes()[0] and facts["stack_bound"] <= 64
    assert pp.name(pp.plan(pp.RENDER, pp.launch(facts, n_tiles, gm.EVICT_TS, 16))) == "render_tiles_packet_kernel<4, false, 8, false, true>"
    assert pp.name(pp.plan(pp.RENDER, pp.launch(facts, n_tiles, gm.EVICT_TS, 64))) == "render_tiles_packet_kernel<16, false, 8, false, true>"
    assert pp.name(pp.plan(pp.AOV, pp.launch(facts, n_tiles, gm.EVICT_TS, 16))) == "render_aov_packet_kernel<4, false, 8, false, true>"
    assert pp.name(pp.plan(pp.RENDER, pp.launch(facts, n_tiles, gm.EVICT_TS, 32, max_depth=2))) == "render_paths_pooled_kernel<4>"
    assert pp.name(pp.plan(pp.RENDER, pp.launch(facts, n_tiles, gm.EVICT_TS, 32, max_depth=2, pooled=0))) == "render_paths_kernel<8, false, false>"


def test_units_of_the_eviction_frame_collide_in_both_tables(oracle):
    """The premise of the GPU cases, on host-only scenes: device_tree(packet=True) is the 16-slot context's tree, device_tree() the
    8-slot context's.  Counted (units, with a node-slot collision, with a leaf-slot collision):
        packet, 16 in flight (2 x 2 pixels, 8 of 64 samples):  packet tree 1 536, 14, 45;  wide tree 1 536, 19, 45
        4 in flight, both kernels (4 x 4 pixels, 4 of 16):      packet tree   384,  7, 50;  wide tree   384, 11, 50"""
    host = gm.evict_host()
    node_entries, leaf_entries = gm.mask_table_sizes()
    trees = {"packet": host.device_tree(packet=True), "wide": host.device_tree()}
    assert trees["packet"][0].shape[1] == 16 and min(t[0].shape[0] for t in trees.values()) > node_entries
    assert host.info().packet_count > 100 * leaf_entries
    for family in gm.EVICT_FAMILIES:
        for kind, tree in trees.items():
            units, node_units, leaf_units = gm.evict_collisions(oracle, family, tree)
            assert node_units >= 5 and leaf_units >= 5, (family, kind, units, node_units, leaf_units)


@pytest.mark.parametrize("kind", ["packet", "wide"])
def test_a_walk_that_ignored_the_tags_would_change_the_frame(oracle, kind):
    """Sensitivity, on the model only (a kernel with a stale mask could leave the tree): gm.cached_unit_walk over the first five
    units of the 16-in-flight family whose hit chains collide in the node table.  With the tags honoured every ray's closest
    distance is the plain per-ray walk's, bit for bit, although entries are evicted; with the tags ignored -- the slot's entry taken
    for whatever node is looked up -- rays lose or change their hits.  (Counted over all colliding units: 13 of 14 units of the
    packet tree and 17 of 19 of the wide tree change, up to 151 of a unit's 256 rays.)"""
    host = gm.evict_host()
    node_entries, leaf_entries = gm.mask_table_sizes()
    nodes, root = (host.device_tree(packet=True) if kind == "packet" else host.device_tree())[:2]
    chains = gm.Chains(nodes, root, host.info().packet_count)
    spp, unit, rpp = gm.EVICT_FAMILIES["packet, 16 in flight"]
    packets = gm._evict_unit_packets(oracle, spp, unit, rpp)
    colliding = [i for i, p in enumerate(packets) if gm.colliding_units(chains, [p], node_entries, leaf_entries)[0]]
    tris = gm.LeafTriangles(host)
    evicted = changed = 0
    for u in colliding[:5]:
        header, passes = gm.evict_unit_passes(oracle, u, shipped_margin())
        plain = np.array([gm.plain_walk(nodes, root, tris, *p) for p in passes])
        tagged, ev = gm.cached_unit_walk(nodes, root, tris, header, passes, node_entries)
        assert ev > 0, u  # the premise's lower bound holds on the model: the unit's lookups do find other nodes' entries
        assert np.array_equal(tagged.view(np.uint32), plain.view(np.uint32)), u
        untagged, _ = gm.cached_unit_walk(nodes, root, tris, header, passes, node_entries, honour_tags=False)
        evicted += ev
        changed += int(np.sum(untagged.view(np.uint32) != plain.view(np.uint32)))
    assert evicted >= 5 and changed >= 1, (kind, evicted, changed)
