"""The long-wave cases: frames on which every wave of a persistent render kernel runs many work units in a row.  Plain data,
importable without a GPU, in the style of tests/dispatch_cases.py: tests/test_long_waves_cpu.py shows through the launch plans
that every case does what it claims, tests/test_gpu_long_waves.py renders every case against the oracle.

Why: a wave draws units from the work queues in a loop (MP_NEXT_UNIT, render_state.h) and keeps its LDS region between two of
them -- the mask-cache header, tables and list arena, the empty-leaf marks, the parked feature sums, the LDS stack and ray queue --
and the pooled path kernel its pool slab in global memory.  The plans size a grid as min(one unit per wave, cu_count x blocks
per CU) (launch_plan.cpp), so a wave loops only where the second term binds: at 256 CUs from 8 192 waves on, which none of the
frames that the other GPU tests compare whole with the oracle reaches (tests/dispatch_cases.py's header).  The context option
"blocks_per_cu" = 1 makes the launchers see cu_count / 8 CUs (mp_ctx::launch_cus): 32 CUs and 1 024 waves on an MI355X, where a
frame of about two million primary rays -- what the oracle renders in a few seconds -- gives every wave eight units.

A case: api      "render", "paths", "wf" (staged), "aov" (feature planes) as in dispatch_cases, "variant" = a render in the
                 `lists_tiny` build of the library (four table slots, 32 arena entries), in a process of its own
        scene    a key of SCENES
        res, ts  the frame and its tile size (32 unless stated); every frame is whole tiles
        spp      samples per pixel; passes: the frame as MP_FLAG_ACCUMULATE passes [(samples, kernel, pixels per unit)]
        depth    max_depth (0 = reference semantics)
        opts     launch options over dispatch_cases.DEFAULTS, by their option names; traversal as RenderSettings takes it
        formats  True: rendered once per tree format (packet_tree_slots 16 and 8) against one oracle frame
        kernels  every kernel name the call must report; kernels[0] is the persistent kernel the case is about
        ppu      pixels per work unit of kernels[0], restated from the kernels' BW x BH (PIXELS_PER_UNIT)
        floor    units per wave the case must reach at cu_count / 8 CUs: FLOOR; HALVED for a path case whose frame was halved
The sizes are set for 256 CUs.  The floor is a condition, not a measurement: with U units on W waves some wave runs at least
U / W of them (pigeonhole), so U / W >= 8 guarantees a wave with eight units in a row."""
from tests import dispatch_cases as dc

SEED = 0x10AD
TS = 32
FLOOR, HALVED = 8, 4
CUS_FULL, CUS_LEVER = 256, 32  # an MI355X, and what its launchers see under blocks_per_cu = 1
PLANES = ("shade", "normal", "albedo", "ids")

PK, AOV = "render_tiles_packet_kernel", "render_aov_packet_kernel"


def cached(s, family=PK):
    return f"{family}<{s}, false, 8, false, true>"


def pixels_per_unit(name):
    """the pixel block BW x BH of a persistent kernel, by its reported name (kernels_tiles.hip, kernels_aov.hip, kernels_paths.hip,
    kernels_staged.hip)"""
    family, _, args = name.partition("<")
    if family in (PK, AOV):
        return 64 // int(args.split(",")[0])  # BW * BH * S == 64
    return PIXELS_PER_UNIT[family]


PIXELS_PER_UNIT = {
    "render_tiles_packet2_kernel": 8,   # 4 x 2, two rays per lane
    "render_paths_kernel": 8,           # 4 x 2 at 8 samples in flight (every path case here)
    "render_paths_pooled_kernel": 8,    # 4 x 2
    "wf_camera_kernel": 4,              # 2 x 2
    "render_tiles_kernel": 64,          # 8 x 8, 8 lanes per ray
}

# What a launch plan reads off the scenes that dispatch_cases.FACTS does not hold (tests/test_long_waves_cpu.py compares these
# with the host builder's exports, tests/test_gpu_long_waves.py with what the live scenes report).
#   evict     tests/graft_model.py evict_mesh() = scenes.atrium(1, 0.5), through scenes.atrium_camera(): the interior view of
#             the eviction tests; both walked trees exceed the node table
#   interior  scenes.atrium(1, 0.05) through the same camera: every path survives to max_depth, the pooled kernel's queue stays
#             full and all of its slab is rewritten per unit
FACTS = {
    **dc.FACTS,
    "evict": {"kind": 0, "stack_bound": 45, "nodes": 1388, "packets": 18326, "tris_bounded": 1, "boxes_ordered": 1, "members": 0},
    "interior": {"kind": 0, "stack_bound": 31, "nodes": 144, "packets": 1838, "tris_bounded": 1, "boxes_ordered": 1, "members": 0},
}
# where a scene's mesh and camera come from: "matrix" = the scene of that name as tests/test_gpu_dispatch_matrix.py builds it (World),
# a number = scenes.atrium(1, that detail) through scenes.atrium_camera()
SCENES = {"teapot": "matrix", "teapot+rgb": "matrix", "group": "matrix", "atrium": "matrix", "evict": 0.5, "interior": 0.05}


def scene_facts(key):
    base, _, rgb = key.partition("+")
    return {**FACTS[base], "rgb": 1 if rgb else 0}


def _case(api, scene, res, spp, kernels, depth=0, ts=TS, formats=False, passes=None, shuffle=False, floor=FLOOR, traversal="packets", **opts):
    assert res[0] % ts == 0 and res[1] % ts == 0 and ts % 8 == 0, "whole tiles, whole pixel blocks"
    assert set(opts) <= set(dc.DEFAULTS), opts
    kernels = tuple(kernels)
    return {"api": api, "scene": scene, "res": tuple(res), "ts": ts, "spp": spp, "depth": depth, "opts": opts, "traversal": traversal,
            "formats": formats, "passes": passes, "shuffle": shuffle, "kernels": kernels, "ppu": pixels_per_unit(kernels[0]), "floor": floor}


def n_tiles(case):
    return (case["res"][0] // case["ts"]) * (case["res"][1] // case["ts"])


def units(case, ppu=None):
    """work units of the case's launch: every tile slot holds ceil(ts / BW) * ceil(ts / BH) of them, ts a multiple of the block"""
    return n_tiles(case) * (case["ts"] * case["ts"] // (ppu or case["ppu"]))


CASES = {}

# ---- the cached packet walk, one context per tree format; about two million primary rays each ------------------------------------
# (teapot view: units that miss, units on the silhouette and interior units alternate inside one wave.  The S = 32 frame is a small
# launch with the cache on, so the plan picks 32 in flight.)
CACHED_FRAMES = {4: ((512, 256), 16), 8: ((256, 256), 32), 16: ((256, 128), 64), 32: ((128, 128), 128)}
for _scene in ("teapot", "evict"):
    for _s, (_res, _spp) in CACHED_FRAMES.items():
        CASES[f"cached walk, {_scene}, {_s} in flight"] = _case("render", _scene, _res, _spp, [cached(_s)], formats=True)
# the 16-in-flight teapot frame once more as ragged MP_FLAG_ACCUMULATE passes in shuffled tile order, against the 96-spp frame.
# The floor holds for the first pass; the second, on 8-pixel units of the same frame, runs 4 096 units on the 1 024 waves: four each.
CASES["cached walk, teapot, ragged passes 64 + 32"] = _case(
    "render", "teapot", CACHED_FRAMES[16][0], 96, [cached(16), cached(8)], formats=True, shuffle=True,
    passes=((64, cached(16), 4), (32, cached(8), 8)))
# ---- the same walk with four table slots and 32 arena entries: lists die in mid-unit, the next unit starts on what they left -------
CASES["cached walk, lists_tiny build, evict, 16 in flight"] = _case("variant", "evict", CACHED_FRAMES[16][0], 64, [cached(16)], formats=True)
# ---- uncached and other tile kernels ---------------------------------------------------------------------------------------------
CASES["uncached, 16 in flight"] = _case("render", "teapot", (256, 128), 17, [PK + "<16, false, 7>"], packet_mask_cache=0)
CASES["uncached, 16 in flight, stack in LDS"] = _case("render", "teapot", (256, 128), 17, [PK + "<16, true, 7>"], packet_mask_cache=0,
                                                      packet_stack_registers=dc.LDS_REGS["teapot"])
CASES["uncached, big scene, 32 in flight"] = _case("render", "atrium", (128, 128), 33, [PK + "<32, false, 8>"], packet_mask_cache=0)
CASES["two rays per lane"] = _case("render", "teapot", (256, 256), 17, ["render_tiles_packet2_kernel<6>"], packet_mask_cache=0, packet_rays_per_lane=2)
CASES["object group, 16 in flight"] = _case("render", "group", (256, 128), 17, [PK + "<16, false, 6, true>"])
CASES["8-lane groups"] = _case("render", "teapot", (1024, 512), 3, ["render_tiles_kernel<1, false>"], traversal="groups")
# ---- path kernels: 256 x 256, segment counts compared ----------------------------------------------------------------------------
PATH_RES = (256, 256)
CASES["paths, cached camera pass"] = _case("paths", "teapot", PATH_RES, 32, ["render_paths_kernel<8, false, false, true>"], depth=3)
CASES["paths"] = _case("paths", "teapot", PATH_RES, 17, ["render_paths_kernel<8, false, false>"], depth=3)
CASES["paths, pooled, two sub-passes"] = _case("paths", "teapot", PATH_RES, 16, ["render_paths_pooled_kernel<2>"], depth=3, paths_pooled=2)
CASES["paths, pooled, four sub-passes"] = _case("paths", "teapot", PATH_RES, 32, ["render_paths_pooled_kernel<4>"], depth=3, paths_pooled=3)
CASES["paths, pooled, four sub-passes, interior"] = _case("paths", "interior", PATH_RES, 32, ["render_paths_pooled_kernel<4>"], depth=2, paths_pooled=3)
# ---- the staged pipeline: 16 camera units per wave; 327 680 paths against cus * 16 blocks of 256 in the flat kernels --------------
CASES["staged pipeline"] = _case("wf", "teapot+rgb", (256, 256), 5, ["wf_camera_kernel<false, false>", "wf_vertex_kernel<3, false>", "wf_scan_kernel",
                                                                    "wf_scatter_kernel", "wf_trace_groups_kernel<false>", "wf_accumulate_kernel"], depth=3)
# ---- feature planes, against the same call at blocks_per_cu = 0 and ("shade") against the oracle ----------------------------------
for _s in (16, 4):
    CASES[f"feature planes, {_s} in flight"] = _case("aov", "teapot", *CACHED_FRAMES[_s], [cached(_s, AOV)])


def launches(case):
    """the case's launches: [(first sample, samples, kernel names, pixels per unit of the persistent kernel)]"""
    if case["passes"] is None:
        return [(0, case["spp"], case["kernels"], case["ppu"])]
    out, begin = [], 0
    for n, kernel, ppu in case["passes"]:
        out.append((begin, n, (kernel,), ppu))
        begin += n
    assert begin == case["spp"]
    return out


def planned(case, cus, facts=None):
    """The case's launches through the launch plans (tests/plan_probe.py; host code only) at `cus` CUs: per launch
    {"names": the kernels the plans name, "grid": blocks of the persistent kernel, "units": its work units, "per_wave": units per
    wave (blocks of four waves), "out": the plan}.  facts: what the plan reads off the scene, scene_facts(case's scene) if not given."""
    from tests import plan_probe as pp

    o = {**dc.DEFAULTS, **case["opts"]}
    api = {"variant": pp.RENDER, **pp.API}[case["api"]]
    out = []
    for begin, n, _, ppu in launches(case):
        inp = pp.launch(facts or scene_facts(case["scene"]), n_tiles(case), case["ts"], case["spp"], (begin, n), cus=cus,
                        traversal=1 if case["traversal"] == "groups" else 0, max_depth=case["depth"], samples=o["packet_samples_in_flight"],
                        lanes=o["packet_rays_per_lane"], cache=o["packet_mask_cache"], pooled=o["paths_pooled"], regs=o["packet_stack_registers"])
        p = pp.plan(api, inp)
        assert p.rc == 0, p.error
        if api == pp.STAGED:
            # the probe reports the grids of a batch of tb tiles: the whole frame, in one sample chunk
            assert p.tb == n_tiles(case) and p.sc == n, "one tile batch, one sample chunk"
            names = [pp.name(p), pp.name(p, "vertex"), "wf_scan_kernel", "wf_scatter_kernel", pp.name(p, "trace"), "wf_accumulate_kernel"]
            u = units(case, ppu)
            out.append({"names": names, "grid": p.cam_grid, "units": u, "per_wave": u / (4 * p.cam_grid), "out": p, "paths": p.n_max,
                        "flat_grid": p.flat_grid})
            continue
        u = units(case, ppu)
        out.append({"names": [pp.name(p)], "grid": p.grid, "units": u, "per_wave": u / (4 * p.grid), "out": p})
    return out
