"""What the exact-tie tests (tests/test_exact_ties_cpu.py, tests/test_gpu_exact_ties.py) share: the scenes of meshes.doubled /
meshes.stack by name, where the twins of a doubled mesh sit in the built packets, and the material tables that make the two
copies differ.  Plain numpy over the oracle, importable without a GPU.

The rule under test (ray_bvh_intersection.rs:104-140, :59): triangles are taken in (packet, lane) order and replace the best hit
on a strict `t < best.t`, so of two triangles of one packet with the same t the lower lane wins.  prim = packet * 8 + lane."""
import numpy as np

from tests import dispatch_cases as _dc
from tests import meshes

F = np.float32
NO = 0xFFFFFFFF
DOUBLED = ("soup_300", "grid_40", "sphere_24", "sliver_fan")
CUTS = (1, 4, 5)  # source triangles of doubled soup_300: a root that is one partly filled packet, a full one, one slot over
N_RAYS = 4096
RAY_SEED = 3
MIN_TIED_SHARE = 0.40  # of the hits; the oracle measures 0.477 to 0.549 on the four doubled meshes

# copy 0 dark, copy 1 bright and emitting: a wrong winner changes the throughput and the emission of every path through the hit
GREY = [(0.2, 0.0), (0.9, 2.5)]
RGB = [{"albedo": (0.2, 0.15, 0.1), "emission": 0.0, "albedo2": (0.1, 0.2, 0.3), "checker": 6.0}, ((0.9, 0.8, 0.7), (2.5, 2.0, 1.5))]
# the three-entry tables of tests/test_gpu_dispatch_matrix.py, for the scenes built with tri_material = source % 3
GREY3 = [(0.8, 0.0), (0.2, 2.5), (0.6, 0.0)]
RGB3 = [{"albedo": (0.9, 0.85, 0.8), "albedo2": (0.1, 0.15, 0.7), "checker": 6.0}, ((0.7, 0.2, 0.3), (0.0, 0.0, 0.0)),
        {"albedo": 0.4, "emission": (1.5, 0.5, 0.0), "albedo2": (0.2, 0.9, 0.2), "checker": 0.75}]
SKY = 0.3


def names():
    """every tie scene: the doubled meshes, doubled soup_300 cut down to CUTS source triangles, the stacks"""
    return list(DOUBLED) + [f"soup_300[:{k}]" for k in CUTS] + [f"stack_{k}" for k in meshes.STACK_SIZES]


def arrays(name):
    """(pos, nrm, tex, tri, copy_id, source) of a tie scene; a stack is k copies of source triangle 0"""
    if name.startswith("stack_"):
        pos, nrm, tex, tri = meshes.stack(int(name[6:]))
        return pos, nrm, tex, tri, np.arange(tri.shape[0], dtype=np.uint32), np.zeros(tri.shape[0], np.uint32)
    if "[:" in name:
        base, _, k = name.partition("[:")
        return meshes.doubled(base, keep=int(k[:-1]))
    return meshes.doubled(name)


def rays(name, orc):
    """the rays of a tie scene: meshes.random_rays(4096, 3) over the box of its oracle BVH; a stack adds the 32 x 32 grid through
    its triangle (in front, so that short calls hold hits); in a cut-down soup every other ray is aimed at a triangle"""
    bmin, bmax = orc.bbox()
    o, d = meshes.random_rays(N_RAYS, RAY_SEED, bmin, bmax)
    if name.startswith("stack_"):
        go, gd = meshes.stack_rays(32)
        o, d = np.concatenate([go, o]), np.concatenate([gd, d])
    if "[:" in name:  # a handful of small triangles in a wide box: every other ray aimed at (and around) one of them
        pos, _, _, tri, *_ = arrays(name)
        rng = np.random.default_rng(RAY_SEED + 1)
        w = rng.dirichlet((1.0, 1.0, 1.0), N_RAYS // 2) * 1.2 - 0.1
        tgt = np.einsum("nk,nkc->nc", w, pos[tri[rng.integers(0, tri.shape[0], N_RAYS // 2)]].astype(np.float64))
        d[1::2] = (tgt - o[1::2]).astype(F)
    return np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)


def twin_slots(orc_by_source):
    """Of an oracle BVH built with tri_material = source: (real, twin); real[s] = slot s (packet * 8 + lane) holds a triangle
    and not padding, twin[s] = the slot of the other copy of its source triangle (-1 for padding).  The builders never read the
    material, so the table holds for every build of the same arrays."""
    sh, src = orc_by_source.tri_shading(), orc_by_source.tri_material()
    real = ~((sh[:, 0] == sh[:, 1]) & (sh[:, 1] == sh[:, 2]))  # padding: vertex indices 0, 0, 0 (building.rs:203-204)
    slots = np.nonzero(real)[0]
    order = slots[np.argsort(src[slots], kind="stable")]
    assert order.size % 2 == 0 and np.array_equal(src[order[0::2]], src[order[1::2]]), "every source triangle twice"
    assert order.size < 4 or not np.any(src[order[0:-2:2]] == src[order[2::2]]), "and only twice"
    twin = np.full(src.shape[0], -1, np.int64)
    twin[order[0::2]], twin[order[1::2]] = order[1::2], order[0::2]
    return real, twin


def tied(prim, twin):
    """mask over rays: a hit whose twin sits in the packet of the hit"""
    p = np.where(prim == NO, 0, prim).astype(np.int64)
    return (prim != NO) & (twin[p] >= 0) & ((twin[p] >> 3) == (p >> 3))


def swapped(table):
    """the table with the materials of the two copies exchanged"""
    return [table[1], table[0]] + list(table[2:])


# ---- the scenes as the oracle holds them, the views, the cases of the GPU file --------------------------------------------------
RES, TS, DEPTH, SEED = (64, 48), 32, 3, 0x5EED
VIEW = ((0.4, 5.0, 4.5), (0.0, 0.0, 0.0))  # a doubled mesh alone
GROUP_SHIFT = (4.25, 0.5, -1.0)  # the second member of the two-member group
GROUP_VIEW = ((2.0, 7.0, 9.0), (2.0, 0.0, 0.0))
LDS_REGS = 3  # packet_stack_registers below the stack bound of grid_40 and sphere_24 doubled


def material_ids(name, which):
    """tri_material of a tie scene: "copy" = copy_id, "source" = source, "source%3" """
    *_, copy_id, source = arrays(name)
    return {"copy": copy_id, "source": source, "source%3": (source % 3).astype(np.uint32)}[which]


def group_translations():
    return np.array([(0.0, 0.0, 0.0), GROUP_SHIFT], F)


def oracle_scene(oracle, name, which="copy", group=False):
    """the oracle's BVH of a tie scene; group: the container of {the scene, the scene shifted by GROUP_SHIFT} (its materials apply)"""
    pos, nrm, tex, tri, *_ = arrays(name)
    mat = material_ids(name, which)
    orc = oracle.Bvh.build(pos, nrm, tex, tri, tri_material=mat)
    if group:
        member = oracle.Bvh.build(pos, nrm, tex, tri, tri_material=mat)
        orc.set_group([member, member], group_translations())
    return orc


def camera(group=False):
    import minipath_amd as mp

    eye, at = GROUP_VIEW if group else VIEW
    return mp.Camera.default().look_at(eye, at, (0, 1, 0))


def sampler(oracle, group=False, res=RES):
    return oracle.sampler_from_array(camera(group).build_sampler(res).as_array())


# ---- the frames of tests/test_gpu_exact_ties.py: kernel name -> row of tests/dispatch_cases.py (scene "mesh" = the doubled mesh
# of the case, "mesh+group" = the two-member group over it, "+rgb" = under the coloured table); every frame RES, tile TS.  Each
# instantiation is reached the way its row of dispatch_cases.CASES reaches it; tests/test_exact_ties_cpu.py sends the rows
# through the launch plans.
_row = _dc._row
# (the doubled sphere's deeper stack leaves the fused path kernel's cached camera pass no LDS: the bounce frames run on the grid)
AOV_MESHES, PATH_MESHES, RENDER_MESHES = ("grid_40", "sphere_24"), ("grid_40",), ("grid_40",)
AOV_CASES = {
    "render_aov_packet_kernel<16, false, 8, false, true>": _row("aov", "mesh", 64),
    "render_aov_packet_kernel<4, false, 8, false, true>": _row("aov", "mesh", 16),
    "render_aov_packet_kernel<1, false, 8>": _row("aov", "mesh", 1),
    "render_aov_packet_kernel<4, false, 8>": _row("aov", "mesh", 4),
    "render_aov_packet_kernel<16, false, 8>": _row("aov", "mesh", 16, cache=0),
    "render_aov_packet_kernel<16, true, 8>": _row("aov", "mesh", 16, regs=LDS_REGS),
    "render_aov_packet_kernel<1, true, 8>": _row("aov", "mesh", 1, regs=LDS_REGS),
    "render_aov_packet_kernel<16, false, 6, true>": _row("aov", "mesh+group", 16),
    "render_aov_packet_kernel<16, true, 6, true>": _row("aov", "mesh+group", 16, regs=LDS_REGS),
    "render_aov_packet_kernel<1, false, 6, true>": _row("aov", "mesh+group", 1),
}
PATH_CASES = {}
for _s, _spp in ((1, 1), (2, 3), (4, 6), (8, 16)):  # the fused kernel takes its samples in flight from the sample count alone
    for _rgb in (False, True):
        PATH_CASES[f"render_paths_kernel<{_s}, false, {str(_rgb).lower()}>"] = _row("paths", "mesh" + ("+rgb" if _rgb else ""), _spp)
PATH_CASES["render_paths_kernel<8, false, false, true>"] = _row("paths", "mesh", 64)  # the cached camera pass: units of four passes
PATH_CASES["render_paths_kernel<8, false, true, true>"] = _row("paths", "mesh+rgb", 64)
PATH_CASES["render_paths_kernel<8, true, false>"] = _row("paths", "mesh+group", 16)
PATH_CASES["render_paths_kernel<8, true, true>"] = _row("paths", "mesh+group+rgb", 16)
PATH_CASES["render_paths_pooled_kernel<2>"] = _row("paths", "mesh", 16, pooled=2)
PATH_CASES["render_paths_pooled_kernel<4>"] = _row("paths", "mesh", 32, pooled=3)
for _obj, _rgb in ((0, 0), (0, 1), (1, 0), (1, 1)):  # the staged pipeline: every kernel it launches is named
    _scene, _, _names = _dc._wf(_obj, 0, _rgb)
    _scene = _scene.replace("group", "mesh+group").replace("teapot", "mesh")
    PATH_CASES[f"staged: {_names[0]} + {_names[1]}"] = _row("wf", _scene, 16, also=_names)
RENDER_CASES = {  # one per packet family
    "render_tiles_packet_kernel<4, false, 8, false, true>": _row("render", "mesh", 16),
    "render_tiles_packet_kernel<16, false, 7>": _row("render", "mesh", 16, cache=0),
    "render_tiles_packet_kernel<16, true, 7>": _row("render", "mesh", 16, cache=0, regs=LDS_REGS),
    "render_tiles_packet2_kernel<6>": _row("render", "mesh", 16, cache=0, lanes=2),
    "render_tiles_kernel<1, false>": _row("render", "mesh", 5, traversal="groups"),
    "render_tiles_packet_kernel<16, false, 6, true>": _row("render", "mesh+group", 16),
}


def expected_names(key, row):
    """the kernels a case must report: its key, or every stage of the staged pipeline (in any order)"""
    return set(row["also"]) if row["api"] == "wf" else {key}
