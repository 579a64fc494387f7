"""The launch plans (minipath_amd/csrc/launch_plan.cpp) on the CPU, through libmp_plan_probe.so: which instantiation a call selects,
with what grid and LDS, and what it refuses.  Every row of tests/dispatch_cases.py must plan to its own name (the GPU matrix then
shows that the launcher launches what the plan says); every threshold of the rules is taken from both sides; the geometry cases
carry numbers worked out by hand from the rules' expressions, 256 CUs and 160 KB of LDS per CU throughout."""
import pytest

from tests import dispatch_cases as dc
from tests import plan_probe as pp
from tests.plan_probe import AOV, BOUNDED, OCCLUDED, RENDER, STAGED, TRACE

TEAPOT, ATRIUM, GROUP, SPHERE = (dc.scene_facts(k) for k in ("teapot", "atrium", "group", "sphere"))
RGB, GROUP_RGB = dc.scene_facts("teapot+rgb"), dc.scene_facts("group+rgb")
FRAME = (510, 64)   # the benchmark's frame: 1920 x 1080 in 30 x 17 tiles of 64 x 64 = 32 640 work units of 8 x 8 pixels: not small
SMALL = (6, 32)     # the matrix's frame: 96 work units: a small launch
PK = "render_tiles_packet_kernel"
REACHED = set()


def kernel(api, facts, frame, spp, n_rays=0, **kw):
    out = pp.plan(api, pp.launch(facts, frame[0], frame[1], spp, **kw), n_rays)
    assert out.rc == 0, out.error
    REACHED.add(pp.name(out))
    return pp.name(out)


def refusal(api, facts, frame, spp, **kw):
    out = pp.plan(api, pp.launch(facts, frame[0], frame[1], spp, **kw))
    return out.rc, out.error.decode()


# ---- every row of the census plans to its own name ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.CASES))
def test_case_rows_plan_to_their_names(name):
    row = dc.CASES[name]
    if row["api"] in ("rays", "untile", "async"):  # launched by a fixed id, no rule; the async worker's render is planned
        assert name in pp.table()
        for other in row["also"]:
            assert pp.row_names({**dc.CASES[other], "spp": row["spp"]}) == {other}
        return
    names = pp.row_names(row)
    REACHED.update(names)
    assert names == {name, *row["also"]}


@pytest.mark.parametrize("guard", list(dc.GATES))
def test_gate_rows_plan_to_the_uncached_name(guard):
    expected, row = dc.GATES[guard]
    assert pp.row_names(row) == {expected}


@pytest.mark.parametrize("which", list(dc.RAGGED))
def test_ragged_passes_plan_by_the_pass(which):
    row, passes = dc.RAGGED[which]
    begin = 0
    for n, expected in passes:
        assert pp.row_names(row, passes=(begin, n)) == {expected}, (begin, n)
        begin += n


# ---- the benchmark's frame: the two rules no oracle render reaches ---------------------------------------------------------------
def test_the_benchmark_frame_is_pinned():
    assert kernel(RENDER, ATRIUM, FRAME, 256) == PK + "<16, false, 8, false, true>"   # cached table, not a small launch
    assert kernel(RENDER, ATRIUM, FRAME, 256, cache=0) == PK + "<32, false, 8>"       # big && nspp >= 128
    assert kernel(RENDER, ATRIUM, FRAME, 127, cache=0) == PK + "<16, false, 8>"
    assert kernel(RENDER, ATRIUM, FRAME, 128, cache=0) == PK + "<32, false, 8>"
    assert kernel(RENDER, ATRIUM, FRAME, 128) == PK + "<16, false, 8, false, true>"   # not small: 16 in flight, not 32
    assert kernel(RENDER, ATRIUM, SMALL, 128) == PK + "<32, false, 8, false, true>"


# ---- thresholds, both sides ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp, s", [(1, 1), (2, 2), (3, 2), (4, 4), (7, 4), (8, 8), (15, 8), (16, 16), (31, 16), (32, 16), (127, 16), (128, 16)])
def test_samples_in_flight_follow_the_pass_uncached(spp, s):
    assert kernel(RENDER, TEAPOT, FRAME, spp, cache=0) == PK + f"<{s}, false, 7>"
    # the pass's samples, not the frame's
    assert kernel(RENDER, TEAPOT, FRAME, 256, cache=0, passes=(100, spp)) == PK + f"<{s}, false, 7>"


@pytest.mark.parametrize("spp, name", [(15, "<8, false, 7>"), (16, "<4, false, 8, false, true>"), (31, "<4, false, 8, false, true>"),
                                       (32, "<8, false, 8, false, true>"), (63, "<8, false, 8, false, true>"), (64, "<16, false, 8, false, true>"),
                                       (128, "<16, false, 8, false, true>")])
def test_cached_table(spp, name):
    assert kernel(RENDER, TEAPOT, FRAME, spp) == PK + name


def test_small_launches_keep_32_in_flight():
    assert kernel(RENDER, TEAPOT, SMALL, 31, cache=0) == PK + "<16, false, 7>"
    assert kernel(RENDER, TEAPOT, SMALL, 32, cache=0) == PK + "<32, false, 7>"
    assert kernel(RENDER, TEAPOT, SMALL, 127) == PK + "<16, false, 8, false, true>"
    assert kernel(RENDER, TEAPOT, SMALL, 128) == PK + "<32, false, 8, false, true>"
    # units * 16 < CUs * 32 * 24: 12 288 units at 256 CUs; a 64 x 64 tile holds 64
    assert kernel(RENDER, TEAPOT, (191, 64), 33, cache=0) == PK + "<32, false, 7>"
    assert kernel(RENDER, TEAPOT, (192, 64), 33, cache=0) == PK + "<16, false, 7>"
    assert kernel(RENDER, TEAPOT, (192, 64), 33, cache=0, cus=257) == PK + "<32, false, 7>"


def test_units_of_four_passes():
    """nspp >= 4 S decides the cache where the samples in flight are requested"""
    for s in (4, 8, 16, 32):
        assert kernel(RENDER, TEAPOT, FRAME, 4 * s - 1, samples=s) == PK + f"<{s}, false, 7>"
        assert kernel(RENDER, TEAPOT, FRAME, 4 * s, samples=s) == PK + f"<{s}, false, 8, false, true>"
    assert kernel(RENDER, TEAPOT, FRAME, 256, samples=2) == PK + "<2, false, 7>"  # no cached form of 1, 2 or 64 in flight
    assert kernel(RENDER, TEAPOT, FRAME, 256, samples=64) == PK + "<64, false, 7>"


def test_the_1_mb_scene_size():
    """nodes * 256 + packets * 384 > 2^20"""
    at = {**TEAPOT, "nodes": 1, "packets": 2730}   # 256 + 1 048 320 = 2^20 exactly: not over
    over = {**TEAPOT, "nodes": 2, "packets": 2730}
    assert kernel(RENDER, at, FRAME, 17, cache=0) == PK + "<16, false, 7>"
    assert kernel(RENDER, over, FRAME, 17, cache=0) == PK + "<16, false, 8>"
    assert kernel(RENDER, at, FRAME, 128, cache=0) == PK + "<16, false, 7>"
    assert kernel(RENDER, over, FRAME, 128, cache=0) == PK + "<32, false, 8>"
    assert kernel(RENDER, at, FRAME, 16, max_depth=2) == "render_paths_kernel<8, false, false>"
    assert kernel(RENDER, over, FRAME, 16, max_depth=2) == "render_paths_pooled_kernel<2>"


def test_mask_cache_guards():
    cached = PK + "<16, false, 8, false, true>"
    assert kernel(RENDER, TEAPOT, FRAME, 64) == cached
    assert kernel(RENDER, {**TEAPOT, "nodes": (1 << 24) - 1}, FRAME, 64) == PK + "<16, false, 8, false, true>"
    assert kernel(RENDER, {**TEAPOT, "nodes": 1 << 24}, FRAME, 64) == PK + "<16, false, 8>"  # the cache tag holds 24 bits
    assert kernel(RENDER, {**TEAPOT, "tris_bounded": 0}, FRAME, 64) == PK + "<16, false, 7>"
    assert kernel(RENDER, {**TEAPOT, "stack_bound": 64}, FRAME, 64) == cached
    assert kernel(RENDER, {**TEAPOT, "stack_bound": 65}, FRAME, 64) == PK + "<16, true, 7>"
    assert kernel(RENDER, TEAPOT, FRAME, 64, cache=2) == cached


def test_the_pooled_gate():
    pooled2, pooled4, plain = "render_paths_pooled_kernel<2>", "render_paths_pooled_kernel<4>", "render_paths_kernel<8, false, false>"
    assert kernel(RENDER, ATRIUM, FRAME, 16, max_depth=2) == pooled2           # auto: a big scene
    assert kernel(RENDER, TEAPOT, FRAME, 16, max_depth=2) == plain             # auto: not a big scene
    assert kernel(RENDER, ATRIUM, FRAME, 16, max_depth=2, pooled=0) == plain
    assert kernel(RENDER, TEAPOT, FRAME, 16, max_depth=2, pooled=2) == pooled2
    assert kernel(RENDER, TEAPOT, FRAME, 16, max_depth=2, pooled=3) == pooled2
    assert kernel(RENDER, ATRIUM, FRAME, 16, max_depth=1) == plain             # max_depth >= 2
    assert kernel(RENDER, ATRIUM, FRAME, 15, max_depth=2) == plain             # nspp >= 16
    assert kernel(RENDER, {**ATRIUM, "rgb": 1}, FRAME, 16, max_depth=2) == "render_paths_kernel<8, false, true>"
    assert kernel(RENDER, {**GROUP, "nodes": 214, "packets": 2898}, FRAME, 16, max_depth=2, pooled=3) == "render_paths_kernel<8, true, false>"
    # two sub-passes, four from 32 samples on unless "two" is asked for
    assert kernel(RENDER, ATRIUM, FRAME, 31, max_depth=2) == pooled2
    assert kernel(RENDER, ATRIUM, FRAME, 32, max_depth=2) == pooled4
    assert kernel(RENDER, ATRIUM, FRAME, 32, max_depth=2, pooled=3) == pooled4
    assert kernel(RENDER, ATRIUM, FRAME, 32, max_depth=2, pooled=2) == pooled2


def test_the_path_kernels_cached_camera_pass():
    cached, plain = "render_paths_kernel<8, false, false, true>", "render_paths_kernel<8, false, false>"
    assert kernel(RENDER, TEAPOT, FRAME, 31, max_depth=3) == plain
    assert kernel(RENDER, TEAPOT, FRAME, 32, max_depth=3) == cached
    assert kernel(RENDER, RGB, FRAME, 32, max_depth=3) == "render_paths_kernel<8, false, true, true>"
    assert kernel(RENDER, TEAPOT, FRAME, 32, max_depth=3, cache=0) == plain
    assert kernel(RENDER, {**TEAPOT, "boxes_ordered": 0}, FRAME, 32, max_depth=3) == plain
    assert kernel(RENDER, {**TEAPOT, "tris_bounded": 0}, FRAME, 32, max_depth=3) == plain
    assert kernel(RENDER, TEAPOT, FRAME, 32, max_depth=3, regs=21) == plain
    assert kernel(RENDER, GROUP, FRAME, 32, max_depth=3) == "render_paths_kernel<8, true, false>"
    # the LDS bound: (384 * 4 + 64 * bound + 3712) * 4 waves * 6 waves per SIMD <= 163 840:
    # bound 24: 6 784 * 24 = 162 816 fits; bound 25: 6 848 * 24 = 164 352 does not
    assert kernel(RENDER, {**TEAPOT, "stack_bound": 24}, FRAME, 32, max_depth=3) == cached
    assert kernel(RENDER, {**TEAPOT, "stack_bound": 25}, FRAME, 32, max_depth=3) == plain


@pytest.mark.parametrize("spp, s", [(1, 1), (2, 2), (3, 2), (4, 4), (7, 4), (8, 8), (31, 8)])
def test_path_samples_in_flight(spp, s):
    for facts, obj in ((TEAPOT, "false"), (GROUP, "true")):
        assert kernel(RENDER, facts, FRAME, spp, max_depth=3) == f"render_paths_kernel<{s}, {obj}, false>"


def test_two_rays_per_lane():
    two = "render_tiles_packet2_kernel<6>"
    assert kernel(RENDER, TEAPOT, FRAME, 17, cache=0, lanes=2) == two
    assert kernel(RENDER, TEAPOT, FRAME, 15, cache=0, lanes=2) == PK + "<8, false, 7>"        # 16 in flight only
    assert kernel(RENDER, TEAPOT, FRAME, 64, lanes=2) == two                                  # S = 16 by the cached table: the form wins
    assert kernel(RENDER, TEAPOT, FRAME, 17, cache=0, lanes=2, regs=21) == PK + "<16, true, 7>"
    assert kernel(RENDER, GROUP, FRAME, 17, lanes=2) == PK + "<16, false, 6, true>"
    assert kernel(RENDER, SPHERE, FRAME, 17, lanes=2) == PK + "<16, false, 7>"
    # stack_cap <= 64, whatever the registers hold
    assert kernel(RENDER, {**TEAPOT, "stack_bound": 64}, FRAME, 17, cache=0, lanes=2) == two
    assert kernel(RENDER, {**TEAPOT, "stack_bound": 65}, FRAME, 17, cache=0, lanes=2, regs=65) == PK + "<16, false, 7>"


def test_requested_samples_in_flight():
    assert kernel(RENDER, TEAPOT, FRAME, 3, cache=0, samples=16) == PK + "<16, false, 7>"  # the request beats the sample count
    for asked in (64, 65, 1000):  # clamped to 64
        out = pp.plan(RENDER, pp.launch(TEAPOT, *SMALL, 70, cache=0, samples=asked))
        assert (pp.name(out), out.grid) == (PK + "<64, false, 7>", 1536)  # 24 blocks of units x 64
    out = pp.plan(RENDER, pp.launch(TEAPOT, *SMALL, 70, cache=0, samples=32))
    assert (pp.name(out), out.grid) == (PK + "<32, false, 7>", 768)


def test_object_groups_run_16_or_1():
    k16, k1 = PK + "<16, false, 6, true>", PK + "<1, false, 6, true>"
    assert kernel(RENDER, GROUP, FRAME, 16) == k16
    assert kernel(RENDER, GROUP, FRAME, 15) == k1
    assert kernel(RENDER, GROUP, FRAME, 256) == k16
    assert kernel(RENDER, GROUP, FRAME, 64, samples=32) == k16
    assert kernel(RENDER, GROUP, FRAME, 64, samples=16) == k16
    assert kernel(RENDER, GROUP, FRAME, 64, samples=15) == k1
    assert kernel(RENDER, GROUP, FRAME, 15, samples=16) == k1   # 16 in flight need 16 samples
    assert kernel(RENDER, GROUP, FRAME, 16, regs=21) == PK + "<16, true, 6, true>"


def test_feature_planes_run_16_4_or_1():
    A = "render_aov_packet_kernel"
    for spp, name in ((3, "<1, false, 8>"), (4, "<4, false, 8>"), (15, "<4, false, 8>"), (16, "<4, false, 8, false, true>"),
                      (63, "<4, false, 8, false, true>"), (64, "<16, false, 8, false, true>")):
        assert kernel(AOV, TEAPOT, FRAME, spp) == A + name, spp
    assert kernel(AOV, TEAPOT, FRAME, 15, cache=0) == A + "<4, false, 8>"
    assert kernel(AOV, TEAPOT, FRAME, 16, cache=0) == A + "<16, false, 8>"
    # a request is rounded down to 16 / 4 / 1; the cache wants four passes of it
    for asked, name in ((3, "<1, false, 8>"), (4, "<4, false, 8, false, true>"), (15, "<4, false, 8, false, true>"), (16, "<16, false, 8>"), (64, "<16, false, 8>")):
        assert kernel(AOV, TEAPOT, FRAME, 63, samples=asked) == A + name, asked
    assert kernel(AOV, TEAPOT, FRAME, 64, samples=16) == A + "<16, false, 8, false, true>"
    assert kernel(AOV, TEAPOT, FRAME, 15, samples=4) == A + "<4, false, 8>"
    # object groups and LDS stacks: no form of 4 in flight
    for facts, kw, tail in ((GROUP_RGB, {}, "false, 6, true>"), (GROUP_RGB, {"regs": 21}, "true, 6, true>"), (TEAPOT, {"regs": 21}, "true, 8>")):
        assert kernel(AOV, facts, FRAME, 15, **kw) == A + "<1, " + tail
        assert kernel(AOV, facts, FRAME, 16, **kw) == A + "<16, " + tail
        assert kernel(AOV, facts, FRAME, 64, samples=8, **kw) == A + "<1, " + tail


def test_ray_queries_and_the_8_lane_groups():
    for api, stem in ((TRACE, "trace_rays_kernel<%s>"), (BOUNDED, "query_rays_kernel<%s, kBounded>"), (OCCLUDED, "query_rays_kernel<%s, kAnyHit>")):
        assert kernel(api, TEAPOT, (0, 0), 0, n_rays=1) == stem % "false"
        assert kernel(api, SPHERE, (0, 0), 0, n_rays=1) == stem % "false"
        assert kernel(api, GROUP, (0, 0), 0, n_rays=1) == stem % "true"
    assert kernel(RENDER, TEAPOT, FRAME, 64, traversal=1) == "render_tiles_kernel<1, false>"
    assert kernel(RENDER, GROUP, FRAME, 64, traversal=1) == "render_tiles_kernel<1, true>"


# ---- refusals: today's code and message ------------------------------------------------------------------------------------------
STACKS = "scene too deep for the LDS traversal stacks"
STACK = "scene too deep for the LDS traversal stack"
CHUNKED = "coloured / textured materials are not combined with MP_FLAG_CHUNKED_SUM"


def test_refusals():
    U = pp.MP_ERR_UNSUPPORTED
    assert refusal(RENDER, SPHERE, FRAME, 8, max_depth=2) == (U, "the path extension is defined for TriangleBvh scenes only")
    assert refusal(STAGED, SPHERE, FRAME, 8, max_depth=2) == (U, "the staged path evaluation needs MP_FLAG_PATHS and a TriangleBvh scene or an object group")
    assert refusal(STAGED, TEAPOT, FRAME, 8, max_depth=0)[0] == U
    assert refusal(RENDER, RGB, FRAME, 8, max_depth=2, chunked=1) == (U, CHUNKED)
    assert refusal(STAGED, RGB, FRAME, 8, max_depth=2, chunked=1) == (U, CHUNKED)
    assert refusal(RENDER, TEAPOT, FRAME, 8, max_depth=2, chunked=1)[0] == 0   # a grey table may
    assert refusal(RENDER, RGB, FRAME, 8, chunked=1)[0] == 0                   # and so may reference semantics
    # the 8-lane-group walk's queue and stacks, (1 536 + 64 * bound) * 4 bytes: bound 616 gives 163 840 = 160 KB, 617 gives 164 096.
    # launch_render_tiles refuses whatever the form (the bound is the scene's, not the kernel's).
    deep, deeper = {**TEAPOT, "stack_bound": 616}, {**TEAPOT, "stack_bound": 617}
    for api, kw in ((RENDER, {}), (RENDER, {"max_depth": 2}), (RENDER, {"traversal": 1}), (STAGED, {"max_depth": 2})):
        assert refusal(api, deep, FRAME, 8, **kw)[0] == 0, kw
        assert refusal(api, deeper, FRAME, 8, **kw) == (U, STACKS), kw
    for api in (TRACE, BOUNDED, OCCLUDED):
        assert refusal(api, deep, FRAME, 8)[0] == 0
        assert refusal(api, deeper, FRAME, 8) == (U, STACKS)
    # the packet walk's entries beyond the registers, 16 bytes each for four waves: the staged camera pass checks them first
    # (2 561 entries: 163 904 bytes); the feature planes add their parked sums (S = 16: 512 bytes; 2 552 entries fit, 2 553 do not)
    assert refusal(STAGED, {**TEAPOT, "stack_bound": 2625}, FRAME, 8, max_depth=2) == (U, STACK)
    assert refusal(AOV, {**TEAPOT, "stack_bound": 2616}, FRAME, 16)[0] == 0
    assert refusal(AOV, {**TEAPOT, "stack_bound": 2617}, FRAME, 16) == (U, STACK)
    # staged: tile_size^2 * min(nspp, 64) <= 2^28
    assert refusal(STAGED, TEAPOT, (1, 2048), 64, max_depth=2)[0] == 0
    assert refusal(STAGED, TEAPOT, (1, 2049), 64, max_depth=2) == (U, "tile_size too large for the staged path evaluation")
    assert refusal(STAGED, TEAPOT, (1, 2049), 63, max_depth=2)[0] == 0


# ---- geometry, worked out by hand from the rules ---------------------------------------------------------------------------------
def geometry(api, facts, frame, spp, n_rays=0, **kw):
    out = pp.plan(api, pp.launch(facts, frame[0], frame[1], spp, **kw), n_rays)
    assert out.rc == 0, out.error
    return out


def test_geometry_of_the_benchmark_frame():
    # 510 tiles x 8 x 8 units = 32 640 units, want = 8 160 blocks of four waves at one unit per wave
    o = geometry(RENDER, ATRIUM, FRAME, 256)
    # cached, S = 16: min(8 160 * 16, 256 CUs * 8) = 2 048; 4 waves x 928 dwords x 4 = 14 848 bytes; stack in registers
    assert (pp.name(o), o.grid, o.lds, o.lds_per_wave) == (PK + "<16, false, 8, false, true>", 2048, 14848, 0)
    o = geometry(RENDER, ATRIUM, FRAME, 256, cache=0)
    assert (o.grid, o.lds, o.lds_per_wave) == (2048, 0, 0)
    # a deep scene: 600 - 64 = 536 entries x 16 = 8 576 bytes per wave, 34 304 per block, 163 840 / 34 304 = 4 blocks per CU
    o = geometry(RENDER, {**TEAPOT, "stack_bound": 600}, FRAME, 17, cache=0)
    assert (pp.name(o), o.grid, o.lds, o.lds_per_wave) == (PK + "<16, true, 7>", 1024, 34304, 8576)
    # a short frame fills less than the machine: 10 tiles = 640 units = 160 blocks x S = 4
    o = geometry(RENDER, TEAPOT, (10, 64), 5, cache=0, cus=1024)
    assert (pp.name(o), o.grid) == (PK + "<4, false, 7>", 640)
    # paths, atrium (bound 34): 1 536 + 64 * 34 = 3 712 bytes per wave, 14 848 per block, 11 blocks fit: 8
    o = geometry(RENDER, ATRIUM, FRAME, 8, max_depth=8)
    assert (pp.name(o), o.grid, o.lds, o.lds_per_wave, o.pool_bytes) == ("render_paths_kernel<8, false, false>", 2048, 14848, 3712, 0)
    # pooled, four sub-passes: stacks only, 64 * 34 = 2 176 per wave; pool 24 rows x 64 x 4 = 6 144 floats per wave,
    # 2 048 blocks x 4 waves x 6 144 x 4 bytes = 201 326 592
    o = geometry(RENDER, ATRIUM, FRAME, 256, max_depth=8)
    assert (pp.name(o), o.grid, o.lds, o.lds_per_wave, o.pool_stride, o.pool_bytes) == ("render_paths_pooled_kernel<4>", 2048, 8704, 2176, 6144, 201326592)
    # two rays per lane: 510 x 16 x 32 = 261 120 units of 8 pixels
    o = geometry(RENDER, ATRIUM, FRAME, 16, cache=0, lanes=2)
    assert (pp.name(o), o.units2, o.grid, o.lds, o.lds_per_wave) == ("render_tiles_packet2_kernel<6>", 261120, 2048, 0, 0)


def test_geometry_of_a_clipped_small_launch():
    # 72 x 40 in 32 x 32 tiles: 6 tiles x 4 x 4 = 96 units, want = 24
    o = geometry(RENDER, TEAPOT, SMALL, 64)
    assert (pp.name(o), o.grid, o.lds, o.lds_per_wave) == (PK + "<16, false, 8, false, true>", 384, 14848, 0)
    o = geometry(RENDER, TEAPOT, SMALL, 33, cache=0)
    assert (pp.name(o), o.grid, o.lds) == (PK + "<32, false, 7>", 768, 0)
    # three registers of a stack of 22: 19 x 16 = 304 bytes per wave
    o = geometry(RENDER, TEAPOT, SMALL, 17, cache=0, regs=3)
    assert (pp.name(o), o.grid, o.lds, o.lds_per_wave) == (PK + "<16, true, 7>", 384, 1216, 304)
    o = geometry(RENDER, TEAPOT, SMALL, 17, cache=0, lanes=2)   # 6 x 8 x 16 units of 8 pixels
    assert (o.units2, o.grid) == (768, 192)
    o = geometry(RENDER, TEAPOT, SMALL, 5, traversal=1)         # 1 536 + 64 * 22 = 2 944 bytes per wave
    assert (pp.name(o), o.grid, o.lds, o.lds_per_wave) == ("render_tiles_kernel<1, false>", 24, 11776, 2944)
    o = geometry(RENDER, TEAPOT, SMALL, 9, max_depth=3)
    assert (o.grid, o.lds, o.lds_per_wave) == (192, 11776, 2944)
    o = geometry(RENDER, TEAPOT, SMALL, 32, max_depth=3)        # + 3 712 of mask cache per wave
    assert (pp.name(o), o.grid, o.lds, o.lds_per_wave) == ("render_paths_kernel<8, false, false, true>", 192, 26624, 6656)
    # pooled, two sub-passes: 64 * 22 = 1 408 per wave; 3 072 floats per wave, 192 x 4 x 3 072 x 4 bytes
    o = geometry(RENDER, TEAPOT, SMALL, 16, max_depth=3, pooled=2)
    assert (pp.name(o), o.grid, o.lds, o.lds_per_wave, o.pool_stride, o.pool_bytes) == ("render_paths_pooled_kernel<2>", 192, 5632, 1408, 3072, 9437184)


def test_geometry_of_the_feature_planes():
    # 24 x 16 in 16 x 16 tiles: 2 tiles x 2 x 2 = 8 units, want = 2; parked sums 4 waves x (64 / S) x 32 bytes
    o = geometry(AOV, TEAPOT, (2, 16), 64)
    assert (o.grid, o.lds, o.lds_per_wave) == (32, 512 + 14848, 0)
    o = geometry(AOV, TEAPOT, (2, 16), 16)
    assert (o.grid, o.lds) == (8, 2048 + 14848)
    o = geometry(AOV, TEAPOT, FRAME, 3)
    assert (o.grid, o.lds) == (2048, 8192)
    # 536 entries in LDS: 34 304 + 8 192 = 42 496 bytes, three blocks per CU
    o = geometry(AOV, {**TEAPOT, "stack_bound": 600}, FRAME, 3)
    assert (pp.name(o), o.grid, o.lds, o.lds_per_wave) == ("render_aov_packet_kernel<1, true, 8>", 768, 42496, 8576)


def test_geometry_of_the_staged_pipeline():
    # 6 tiles of 32 x 32 at 5 samples: 5 120 paths per tile, one batch of 6 tiles: 30 720 paths, 6 x 512 bins;
    # 30 720 x 96 bytes + 3 x (3 072 + 64) x 4 = 2 986 752
    o = geometry(STAGED, TEAPOT, SMALL, 5, max_depth=3)
    assert (o.sc, o.tb, o.n_max, o.nbins, o.nchan, o.ws_bytes) == (5, 6, 30720, 3072, 1, 2986752)
    # camera: 6 x 16 x 16 units of 2 x 2 pixels / 4; flat: 30 720 / 256; pixels: 6 144 / 256; trace: 256 CUs x 8
    assert (o.cam_grid, o.flat_grid, o.px_grid, o.trace_grid) == (384, 120, 24, 2048)
    assert (o.lds, o.lds_per_wave, o.trace_lds, o.trace_lds_per_wave) == (0, 0, 11776, 2944)
    assert {pp.name(o), pp.name(o, "vertex"), pp.name(o, "trace")} == {"wf_camera_kernel<false, false>", "wf_vertex_kernel<1, false>", "wf_trace_groups_kernel<false>"}
    # the benchmark's frame at 256 samples: chunks of 64 samples, 262 144 paths per tile, 2^21 / 2^18 = 8 tiles per batch
    o = geometry(STAGED, ATRIUM, FRAME, 256, max_depth=8)
    assert (o.sc, o.tb, o.n_max, o.nbins, o.ws_bytes) == (64, 8, 2097152, 4096, 2097152 * 96 + 4160 * 12)
    assert (o.cam_grid, o.flat_grid, o.px_grid, o.trace_grid, o.trace_lds) == (2048, 4096, 128, 2048, 14848)
    o = geometry(STAGED, {**ATRIUM, "rgb": 1}, FRAME, 256, max_depth=8)
    assert (o.nchan, o.ws_bytes) == (3, 2097152 * 112 + 4160 * 12)  # 88 + 8 per channel
    # a tile of more than 2^21 paths is a batch of its own
    o = geometry(STAGED, TEAPOT, (3, 256), 64, max_depth=2)
    assert (o.tb, o.n_max) == (1, 4194304)
    o = geometry(STAGED, TEAPOT, SMALL, 5, max_depth=3, regs=3)
    assert (pp.name(o), o.lds, o.lds_per_wave) == ("wf_camera_kernel<true, false>", 1216, 304)


def test_geometry_of_the_ray_queries():
    # 6 000 rays = 94 chunks of 64 = 24 blocks of four waves
    for api in (TRACE, BOUNDED, OCCLUDED):
        o = geometry(api, TEAPOT, (0, 0), 0, n_rays=6000)
        assert (o.grid, o.lds, o.lds_per_wave) == (24, 11776, 2944)
        assert geometry(api, TEAPOT, (0, 0), 0, n_rays=10 ** 7).grid == 2048
        assert geometry(api, TEAPOT, (0, 0), 0, n_rays=1).grid == 1


# ---- the table has no unreachable row -------------------------------------------------------------------------------------------
FIXED = {"set_u64_kernel", "generate_rays_kernel", "untile_kernel", "quantise_kernel", "wf_scan_kernel", "wf_scatter_kernel", "wf_accumulate_kernel"}


def test_every_table_row_is_reached():
    """every id is the answer of a plan to an input of test_case_rows_plan_to_their_names, or one of the kernels without a rule,
    which their launcher names by a constant"""
    reached = set()
    for row in dc.CASES.values():
        if row["api"] in pp.API:
            reached |= pp.row_names(row)
    names = pp.table()
    assert len(names) == len(set(names))
    assert FIXED <= set(names)
    assert set(names) - reached - FIXED == set(), "table rows no plan input of the tests reaches"
    assert reached - set(names) == set()
