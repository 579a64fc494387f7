"""Preconditions of the exact-tie tests (tests/test_gpu_exact_ties.py), on the CPU with the oracle alone: the doubled meshes do
put pairs of bit-identical triangles into one packet, for a large share of the hits; such a pair ties in t, u and v bit for bit;
the oracle resolves every tie to the lower lane, and mostly not to lane 0; the product's builder lays these meshes out as the
oracle's does; and the material tables of the bounce-mode cases make a wrong winner visible in the image.  Without these the
GPU cases would pass for any tie order."""
import numpy as np
import pytest

import minipath_amd as mp
from tests import meshes, plan_probe
from tests import tie_model as tm
from tests.test_host_cpu import _assert_same_bvh

NO = tm.NO


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Doubled:
    """a doubled mesh as the oracle builds it with tri_material = source, its rays, its hits, the twin of every slot"""

    def __init__(self, oracle, name):
        self.orc = tm.oracle_scene(oracle, name, "source")
        self.real, self.twin = tm.twin_slots(self.orc)
        self.o, self.d = tm.rays(name, self.orc)
        self.t, self.prim, self.u, self.v = self.orc.trace(self.o, self.d)
        self.hit = self.prim != NO
        self.tied = tm.tied(self.prim, self.twin)


@pytest.fixture(scope="module")
def doubled(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Doubled(oracle, name)
        return cache[name]

    return get


@pytest.mark.parametrize("name", tm.DOUBLED)
def test_the_twin_sits_in_the_hit_packet_for_two_hits_in_five(doubled, name):
    """Measured: soup_300 0.483 of 234 hits, grid_40 0.549 of 2637, sphere_24 0.505 of 2651, sliver_fan 0.477 of 2038."""
    s = doubled(name)
    assert s.real.sum() == 2 * (s.real.sum() // 2) == tm.arrays(name)[3].shape[0]
    share = s.tied.sum() / s.hit.sum()
    print(f"{name}: {s.orc.n_packets} packets, {int(s.hit.sum())} hits, twin in the hit packet {share:.3f}")
    assert s.hit.sum() >= 200 and share >= tm.MIN_TIED_SHARE


def _without(oracle, s, slots):
    """the BVH of s with the triangles in `slots` collapsed to a point (v1 = v2 = v0: det = 0, u is NaN or infinite, no ray
    accepts it); nodes, boxes and every other slot as they were"""
    pk = s.orc.packets_bytes().view(np.uint16).reshape(-1, 3, 3, 8).copy()  # [packet][vertex][axis][lane]
    p, lane = slots >> 3, slots & 7
    pk[p, 1, :, lane] = pk[p, 0, :, lane]
    pk[p, 2, :, lane] = pk[p, 0, :, lane]
    bmin, bmax = s.orc.bbox()
    return oracle.Bvh.from_arrays(s.orc.inner_nodes_bytes(), pk.view(np.uint8).reshape(-1, 144), s.orc.tri_shading(), s.orc.vertex_normals(),
                                  s.orc.vertex_tex(), s.orc.root, bmin, bmax, material=s.orc.tri_material())


@pytest.mark.parametrize("name", tm.DOUBLED)
def test_twins_in_one_packet_tie_in_full(oracle, doubled, name):
    """Re-traced with the winner's slot removed, every hit whose twin sits in its packet lands on the twin with the same t, u
    and v, bit for bit.  (Two re-traces: the lower lane of every such pair removed, then the upper; each ray is read from the one
    that removed its winner.)"""
    s = doubled(name)
    slots = np.nonzero(s.real)[0]
    pair = slots[(s.twin[slots] >> 3) == (slots >> 3)]
    lower, upper = pair[pair < s.twin[pair]], pair[pair > s.twin[pair]]
    assert lower.size == upper.size > 0
    w = s.prim[s.tied].astype(np.int64)
    checked = 0
    for removed in (lower, upper):
        t2, prim2, u2, v2 = _without(oracle, s, removed).trace(s.o, s.d)
        mine = np.isin(w, removed)
        idx = np.nonzero(s.tied)[0][mine]
        assert np.array_equal(prim2[idx].astype(np.int64), s.twin[w[mine]])
        for a, b in ((t2, s.t), (u2, s.u), (v2, s.v)):
            assert np.array_equal(bits(a[idx]), bits(b[idx]))
        checked += idx.size
    assert checked == s.tied.sum()


@pytest.mark.parametrize("name", tm.DOUBLED)
def test_the_lower_lane_wins_and_is_mostly_not_lane_0(doubled, name):
    """Measured share of winners outside lane 0: soup_300 0.717, grid_40 0.716, sphere_24 0.757, sliver_fan 0.768."""
    s = doubled(name)
    w = s.prim[s.tied].astype(np.int64)
    assert np.all(w < s.twin[w]), f"{int(np.sum(w > s.twin[w]))} ties went to the upper lane"
    off0 = np.mean((w & 7) != 0)
    print(f"{name}: {w.size} tied hits, winner outside lane 0 {off0:.3f}")
    assert off0 >= 0.5


@pytest.mark.parametrize("which", ["copy", "source"])
@pytest.mark.parametrize("name", tm.names())
def test_builders_agree_on_the_tie_meshes(oracle, name, which):
    """Many identical centroids per bin, and roots that are one packet: scene_build.cpp == the oracle's builder, byte for byte."""
    pos, nrm, tex, tri, *_ = tm.arrays(name)
    mat = tm.material_ids(name, which)
    _assert_same_bvh(mp.TriangleBvh.build(pos, nrm, tex, tri, tri_material=mat), oracle.Bvh.build(pos, nrm, tex, tri, tri_material=mat))


@pytest.mark.parametrize("k", tm.CUTS)
def test_small_roots(oracle, k):
    """2, 8 and 10 rows: one partly filled packet, one full packet, one slot over"""
    orc = tm.oracle_scene(oracle, f"soup_300[:{k}]", "source")
    assert orc.n_packets == (2 * k + 7) // 8 and tm.twin_slots(orc)[0].sum() == 2 * k


@pytest.mark.parametrize("k", meshes.STACK_SIZES)
def test_a_stack_reports_slot_0_of_packet_0(oracle, k):
    name = f"stack_{k}"
    orc = tm.oracle_scene(oracle, name)
    assert orc.n_packets == (k + 7) // 8
    o, d = tm.rays(name, orc)
    _, prim, _, _ = orc.trace(o, d)
    grid = prim[: 32 * 32]
    assert 300 < (grid != NO).sum() < 32 * 32 and (prim[32 * 32:] != NO).sum() > 500
    assert np.all(prim[prim != NO] == 0)


def _frame(orc, oracle, table, group, spp=16):
    orc.set_materials(table, tm.SKY)
    f, _, _, seg = orc.render_image_paths_mt(tm.sampler(oracle, group), *tm.RES, spp, tm.SEED, tm.DEPTH, tm.TS, 8)
    return f, seg


@pytest.mark.parametrize("group", [False, True], ids=["plain", "group"])
@pytest.mark.parametrize("table", ["GREY", "RGB"])
@pytest.mark.parametrize("name", tm.PATH_MESHES)
def test_a_wrong_winner_would_change_the_bounce_frames(oracle, doubled, name, table, group):
    """The oracle's own frame under the bounce-mode table, against (a) its frame with the materials of the two copies swapped
    and (b) its frame with the materials swapped only inside the pairs that share a packet -- what a walk that resolved every
    tie to the upper lane would shade.  Both must differ in more than 5 % of the pixels."""
    tab = getattr(tm, table)
    orc = tm.oracle_scene(oracle, name, "copy", group)
    base, seg = _frame(orc, oracle, tab, group)
    assert seg > tm.RES[0] * tm.RES[1] * 16, "paths bounce"
    swapped, _ = _frame(orc, oracle, tm.swapped(tab), group)
    share_a = np.mean(np.any(bits(base) != bits(swapped), axis=-1))
    # (b) the same arrays with the material ids exchanged inside every pair that shares a packet
    s = doubled(name)
    plain = tm.oracle_scene(oracle, name, "copy")
    mat = plain.tri_material()
    slots = np.nonzero(s.real)[0]
    pair = slots[(s.twin[slots] >> 3) == (slots >> 3)]
    mat2 = mat.copy()
    mat2[pair] = mat[s.twin[pair]]
    bmin, bmax = plain.bbox()

    def rebuilt():
        return oracle.Bvh.from_arrays(plain.inner_nodes_bytes(), plain.packets_bytes(), plain.tri_shading(), plain.vertex_normals(),
                                      plain.vertex_tex(), plain.root, bmin, bmax, material=mat2)

    wrong = rebuilt()
    if group:
        member = rebuilt()
        wrong.set_group([member, member], tm.group_translations())
    upper, _ = _frame(wrong, oracle, tab, group)
    share_b = np.mean(np.any(bits(base) != bits(upper), axis=-1))
    print(f"{name} {table} {'group' if group else 'plain'}: pixels that differ: copies swapped {share_a:.3f}, ties to the upper lane {share_b:.3f}")
    assert share_a > 0.05 and share_b > 0.05


def _facts(name, group, rgb):
    """what a launch plan reads off a tie scene, from the host-only build (tests/dispatch_cases.py FACTS)"""
    pos, nrm, tex, tri, *_ = tm.arrays(name)
    gpu = mp.TriangleBvh.build(pos, nrm, tex, tri)
    nodes, _, bound, _ = gpu.device_tree()
    assert bound > tm.LDS_REGS
    if group:
        return {"kind": 0, "stack_bound": bound, "nodes": 0, "packets": 0, "tris_bounded": 0, "boxes_ordered": 0, "members": 2, "rgb": rgb}
    return {"kind": 0, "stack_bound": bound, "nodes": len(nodes), "packets": gpu.info().packet_count, "tris_bounded": 1, "boxes_ordered": 1,
            "members": 0, "rgb": rgb}


@pytest.mark.parametrize("name", ["grid_40", "sphere_24"])
def test_the_frames_plan_to_the_kernels_they_name(name):
    """Every frame case of the GPU file selects the instantiation it is filed under (the GPU file asserts the launched names)."""
    from tests import dispatch_cases as dc

    n_tiles = -(-tm.RES[0] // tm.TS) * -(-tm.RES[1] // tm.TS)
    for cases, of in ((tm.AOV_CASES, tm.AOV_MESHES), (tm.PATH_CASES, tm.PATH_MESHES), (tm.RENDER_CASES, tm.RENDER_MESHES)):
        for key, row in cases.items() if name in of else ():
            o = {**dc.DEFAULTS, **row["opts"]}
            facts = _facts(name, "group" in row["scene"], int(row["scene"].endswith("+rgb")))
            inp = plan_probe.launch(facts, n_tiles, tm.TS, row["spp"], traversal=1 if row["traversal"] == "groups" else 0,
                                    max_depth=tm.DEPTH if row["api"] in ("paths", "wf") else 0, samples=o["packet_samples_in_flight"],
                                    lanes=o["packet_rays_per_lane"], cache=o["packet_mask_cache"], pooled=o["paths_pooled"], regs=o["packet_stack_registers"])
            out = plan_probe.plan(plan_probe.API[row["api"]], inp)
            assert out.rc == 0, (key, out.error)
            if row["api"] == "wf":
                got = {plan_probe.name(out), plan_probe.name(out, "vertex"), plan_probe.name(out, "trace"), "wf_scan_kernel", "wf_scatter_kernel", "wf_accumulate_kernel"}
            else:
                got = {plan_probe.name(out)}
            assert got == tm.expected_names(key, row), (key, got)


@pytest.mark.parametrize("name", tm.DOUBLED)
def test_the_fuzz_tool_draws_the_same_doubled_meshes(name):
    """tools/fuzz_gpu.py writes the doubling recipe out for itself (it needs only meshes.make): same rows, same copy ids."""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("fuzz_gpu", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    pos, nrm, tex, tri, copy_id = mod.doubled(name)
    want = meshes.doubled(name)
    for a, b in zip((pos, nrm, tex, tri, copy_id), want[:5]):
        assert (a is None and b is None) or (a.dtype == b.dtype and np.array_equal(a, b))
