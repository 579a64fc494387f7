"""The dispatch census: one parity case per kernel instantiation of minipath_amd/csrc/kernel_table.h, keyed by the name
mp_ctx_last_kernels reports (the kernel with its template arguments as the table's row writes them).  Plain data, importable
without a GPU: tests/test_dispatch_census_cpu.py asserts that the keys are exactly the table's rows, tests/test_launch_plan_cpu.py
sends every row through the launch plans (launch_plan.cpp) and must get the row's name, and tests/test_gpu_dispatch_matrix.py runs
every row on the GPU against the oracle.

A row: api    "render" (reference semantics), "paths" (MP_FLAG_PATHS), "wf" (+ MP_FLAG_WAVEFRONT), "aov" (feature planes),
              "trace" / "bounded" / "occluded" (ray queries), "rays" (mp_generate_rays), "untile", "async" (mp.render)
       scene  "teapot", "atrium" (scenes.atrium(1, 0.08): traversal arrays over 1 MB, stack bound 34), "group" ({teapot, soup,
              sphere}), "sphere", "atrium*2^27" (the atrium scaled until its coordinates pass the triangle masks' 2^30 bound);
              "+rgb" = under a coloured / checker material table.  FACTS holds what a launch plan reads off each scene.
       spp    samples per pixel (= samples of the pass)
       opts   the five launch options, every one set explicitly by every case (DEFAULTS, then the row's)
       also   other names the same call must report besides the row's key (the staged pipeline's stages, the async worker's render)

Why each row selects its kernel follows plan_render_tiles / plan_render_aov / plan_render_paths_wavefront as they stand; the
frames of the matrix (72 x 40 and smaller) are all "small launches" there (units * 16 < CUs * 32 * 24), so 32 or more samples
select 32 in flight.  On the GPU the 32-in-flight forms, <32, *, 8> included, are reached through that rule.  The plans' other
two ways to them (`big && nspp >= 128`, and the cached table of a launch that is not small) need frames of 12 288 work units or
more, whose oracle renders do not fit a test; tests/test_launch_plan_cpu.py pins both by name on the benchmark's own frame.
At these sizes every launch is also one work unit per wave: the frames on which the waves of the persistent kernels run many
units in a row are those of tests/long_waves.py (the context option blocks_per_cu = 1, tests/test_gpu_long_waves.py).

The matrix's own tiling is regular: at tile sizes 32 and 16 the clipped column and row of its frames are 8 pixels wide and high, a
whole number of every pixel block of the packet kernels (8x8 ... 1x1), so there a work unit lies wholly inside its tile or wholly
outside.  The oracle's frame does not depend on the tiling, so every render / paths / wf / aov row runs again, against the same
oracle frames, on the tile lists of tests/tile_geometries.py (tile sizes 13 and 1, and a partition into unaligned blocks), whose
units are cut by their tiles: the lanes outside the tile inside a live unit, the slots' untouched remainder and the hand-out order
are then held per instantiation (tiled_rows; tests/test_tile_geometries_cpu.py shows that every row keeps its name there and that
units are in fact cut).  STAGED_BATCHES are the frames that take the staged pipeline through several tile batches."""

DEFAULTS = {"packet_samples_in_flight": 0, "packet_mask_cache": 1, "packet_stack_registers": 64, "packet_rays_per_lane": 1, "paths_pooled": 1}
# the frames of the matrix: render / path / staged cases 3 x 2 tiles with the right column and bottom row clipped; the feature planes'
# model costs one ctypes call per ray; path cases bounce (max_depth >= 2); ray queries
RES, TS = (72, 40), 32
AOV_RES, AOV_TS = (24, 16), 16
DEPTH = 3
N_RAYS = 6000
LDS_REGS = {"teapot": 3, "group": 3, "atrium": 8}  # packet_stack_registers below the scene's stack bound (22, 22, 34)

# What a launch plan reads off a scene (DevScene): kind 0 TriangleBvh / object group, 1 Sphere; the traversal-stack bound; nodes of
# the wide tree and packets (an object group has no arrays of its own: 0, its members are walked one by one); whether the triangle
# masks' coordinate bound holds and every child box is ordered; the members of a group.  test_gpu_dispatch_matrix.py asserts that
# the live scenes report the same stack bound, node and packet counts; tris_bounded and boxes_ordered are not reported by the API
# and are held by the kernel names of the rows that read them (the cached rows and the gate "triangle coordinates beyond 2^30").
FACTS = {
    "teapot": {"kind": 0, "stack_bound": 22, "nodes": 27, "packets": 319, "tris_bounded": 1, "boxes_ordered": 1, "members": 0},
    "atrium": {"kind": 0, "stack_bound": 34, "nodes": 214, "packets": 2898, "tris_bounded": 1, "boxes_ordered": 1, "members": 0},
    "atrium*2^27": {"kind": 0, "stack_bound": 34, "nodes": 214, "packets": 2898, "tris_bounded": 0, "boxes_ordered": 1, "members": 0},
    "group": {"kind": 0, "stack_bound": 22, "nodes": 0, "packets": 0, "tris_bounded": 0, "boxes_ordered": 0, "members": 3},
    "sphere": {"kind": 1, "stack_bound": 1, "nodes": 0, "packets": 0, "tris_bounded": 0, "boxes_ordered": 0, "members": 0},
}


def scene_facts(key):
    """FACTS of a row's scene, "+rgb" = a coloured table"""
    base, _, rgb = key.partition("+")
    return {**FACTS[base], "rgb": 1 if rgb else 0}


# the table holds these too, but they are utilities, not instantiations of the render / query paths: no row
EXCLUDED = {
    "set_u64_kernel": "one-thread store that initialises the ray-segment counter; its value is asserted by every counted case",
}


def launched(ctx):
    """ctx.last_kernels() without the utilities of EXCLUDED: FrameRenderer always passes a segment counter, so its render calls
    report set_u64_kernel before the render kernel"""
    return [k for k in ctx.last_kernels() if k not in EXCLUDED]


# launch sites of the test probes, outside family_launch.h and outside the library (libmp_probe.so / libmp_mask_probe.so)
PROBE_FILES = {
    "probe.hip": "test probe of ray_math.h (tests/test_ray_math_gpu.py): its kernels are the test, not the product",
    "mask_probe.hip": "test probe of mask_cache.h (tests/test_mask_cache_gpu.py): its kernels are the test, not the product",
}


def _row(api, scene, spp, also=(), **opts):
    short = {"samples": "packet_samples_in_flight", "cache": "packet_mask_cache", "regs": "packet_stack_registers",
             "lanes": "packet_rays_per_lane", "pooled": "paths_pooled", "traversal": "traversal"}
    o = {short[k]: v for k, v in opts.items()}
    trav = o.pop("traversal", "packets")
    return {"api": api, "scene": scene, "spp": spp, "opts": o, "traversal": trav, "also": tuple(also)}


def wf_configurations():
    """the staged rows by configuration: the thirteen rows share eight (scene, options); {first row's key: every key that shares it}"""
    seen = {}
    for key, row in CASES.items():
        if row["api"] == "wf":
            seen.setdefault((row["scene"], tuple(sorted(row["opts"].items()))), []).append(key)
    return {keys[0]: keys for keys in seen.values()}


def tiled_rows():
    """the rows whose call takes a tile list (render / paths / aov, and one staged row per configuration): what
    tests/test_gpu_dispatch_matrix.py runs again on every geometry of tests/tile_geometries.py"""
    first = set(wf_configurations())
    return [k for k, row in CASES.items() if row["api"] in ("render", "paths", "aov") or k in first]


CASES = {}

# ---- launch_render_tiles, packets: <S, LDS_STACK, W>; automatic S from the pass's samples, mask cache off ------------------------
for _s, _spp in ((1, 1), (2, 3), (4, 5), (8, 9), (16, 17), (32, 33)):
    CASES[f"render_tiles_packet_kernel<{_s}, false, 7>"] = _row("render", "teapot", _spp, cache=0)
    CASES[f"render_tiles_packet_kernel<{_s}, true, 7>"] = _row("render", "teapot", _spp, cache=0, regs=LDS_REGS["teapot"])
# 64 in flight only on request
CASES["render_tiles_packet_kernel<64, false, 7>"] = _row("render", "teapot", 70, cache=0, samples=64)
CASES["render_tiles_packet_kernel<64, true, 7>"] = _row("render", "teapot", 70, cache=0, samples=64, regs=LDS_REGS["teapot"])
# big scene: eight waves per SIMD
CASES["render_tiles_packet_kernel<16, false, 8>"] = _row("render", "atrium", 17, cache=0)
CASES["render_tiles_packet_kernel<16, true, 8>"] = _row("render", "atrium", 17, cache=0, regs=LDS_REGS["atrium"])
CASES["render_tiles_packet_kernel<32, false, 8>"] = _row("render", "atrium", 33, cache=0)
CASES["render_tiles_packet_kernel<32, true, 8>"] = _row("render", "atrium", 33, cache=0, regs=LDS_REGS["atrium"])
# mask cache (default on): S follows the sample count, units of at least four passes
CASES["render_tiles_packet_kernel<4, false, 8, false, true>"] = _row("render", "teapot", 16)
CASES["render_tiles_packet_kernel<8, false, 8, false, true>"] = _row("render", "teapot", 33)
CASES["render_tiles_packet_kernel<16, false, 8, false, true>"] = _row("render", "teapot", 64)
CASES["render_tiles_packet_kernel<32, false, 8, false, true>"] = _row("render", "teapot", 128)
# object group: 16 in flight from 16 samples on, else one
CASES["render_tiles_packet_kernel<16, false, 6, true>"] = _row("render", "group", 17)
CASES["render_tiles_packet_kernel<16, true, 6, true>"] = _row("render", "group", 17, regs=LDS_REGS["group"])
CASES["render_tiles_packet_kernel<1, false, 6, true>"] = _row("render", "group", 3)
CASES["render_tiles_packet_kernel<1, true, 6, true>"] = _row("render", "group", 3, regs=LDS_REGS["group"])
# two rays per lane: 16 in flight, stack in registers
CASES["render_tiles_packet2_kernel<6>"] = _row("render", "teapot", 17, cache=0, lanes=2)
# ---- launch_render_tiles, 8-lane groups ------------------------------------------------------------------------------------------
CASES["render_tiles_kernel<1, false>"] = _row("render", "teapot", 5, traversal="groups")
CASES["render_tiles_kernel<1, true>"] = _row("render", "group", 5, traversal="groups")
# ---- launch_render_tiles, paths: <S, OBJ, RGB>, S from the pass's samples: 1, 2-3, 4-7, >= 8 ------------------------------------
for _s, _spp in ((1, 1), (2, 3), (4, 6), (8, 9)):
    for _obj in (False, True):
        for _rgb in (False, True):
            _scene = ("group" if _obj else "teapot") + ("+rgb" if _rgb else "")
            CASES[f"render_paths_kernel<{_s}, {str(_obj).lower()}, {str(_rgb).lower()}>"] = _row("paths", _scene, _spp)
# camera pass on the cached packet walk: 32 samples or more, plain scene, stack in registers
CASES["render_paths_kernel<8, false, false, true>"] = _row("paths", "teapot", 32)
CASES["render_paths_kernel<8, false, true, true>"] = _row("paths", "teapot+rgb", 32)
CASES["render_paths_pooled_kernel<2>"] = _row("paths", "teapot", 16, pooled=2)
CASES["render_paths_pooled_kernel<4>"] = _row("paths", "teapot", 32, pooled=3)
# ---- launch_render_aov: <S, LDS_STACK, W[, OBJ[, MCACHE]]> -----------------------------------------------------------------------
CASES["render_aov_packet_kernel<16, false, 8, false, true>"] = _row("aov", "teapot", 64)
CASES["render_aov_packet_kernel<4, false, 8, false, true>"] = _row("aov", "teapot", 16)
CASES["render_aov_packet_kernel<16, true, 6, true>"] = _row("aov", "group+rgb", 16, regs=LDS_REGS["group"])
CASES["render_aov_packet_kernel<16, false, 6, true>"] = _row("aov", "group+rgb", 16)
CASES["render_aov_packet_kernel<1, true, 6, true>"] = _row("aov", "group+rgb", 3, regs=LDS_REGS["group"])
CASES["render_aov_packet_kernel<1, false, 6, true>"] = _row("aov", "group+rgb", 3)
CASES["render_aov_packet_kernel<16, true, 8>"] = _row("aov", "teapot", 16, regs=LDS_REGS["teapot"])
CASES["render_aov_packet_kernel<1, true, 8>"] = _row("aov", "teapot", 3, regs=LDS_REGS["teapot"])
CASES["render_aov_packet_kernel<16, false, 8>"] = _row("aov", "teapot", 16, cache=0)
CASES["render_aov_packet_kernel<4, false, 8>"] = _row("aov", "teapot", 5)
CASES["render_aov_packet_kernel<1, false, 8>"] = _row("aov", "teapot", 3)
# ---- launch_render_paths_wavefront: camera <LDS_STACK, OBJ>, vertex <NCHAN, OBJ>, trace <OBJ>, scan / scatter / accumulate -------


def _wf(obj, lds, rgb):
    """(scene, options, every kernel the staged pipeline launches for it)"""
    b = lambda x: str(bool(x)).lower()  # noqa: E731
    scene = ("group" if obj else "teapot") + ("+rgb" if rgb else "")
    names = [f"wf_camera_kernel<{b(lds)}, {b(obj)}>", f"wf_vertex_kernel<{3 if rgb else 1}, {b(obj)}>", "wf_scan_kernel", "wf_scatter_kernel",
             f"wf_trace_groups_kernel<{b(obj)}>", "wf_accumulate_kernel"]
    return scene, ({"regs": LDS_REGS["group" if obj else "teapot"]} if lds else {}), names


for _key, _cfg in (("wf_camera_kernel<false, false>", (0, 0, 0)), ("wf_camera_kernel<true, false>", (0, 1, 0)),
                   ("wf_camera_kernel<false, true>", (1, 0, 0)), ("wf_camera_kernel<true, true>", (1, 1, 0)),
                   ("wf_vertex_kernel<1, false>", (0, 1, 0)), ("wf_vertex_kernel<1, true>", (1, 1, 0)),
                   ("wf_vertex_kernel<3, false>", (0, 0, 1)), ("wf_vertex_kernel<3, true>", (1, 0, 1)),
                   ("wf_trace_groups_kernel<false>", (0, 0, 0)), ("wf_trace_groups_kernel<true>", (1, 0, 1)),
                   ("wf_scan_kernel", (0, 1, 1)), ("wf_scatter_kernel", (1, 1, 1)), ("wf_accumulate_kernel", (1, 0, 0))):
    _scene, _o, _names = _wf(*_cfg)
    assert _key in _names
    CASES[_key] = _row("wf", _scene, 5, also=[n for n in _names if n != _key], **_o)
# ---- ray queries -----------------------------------------------------------------------------------------------------------------
CASES["trace_rays_kernel<false>"] = _row("trace", "teapot", 0)
CASES["trace_rays_kernel<true>"] = _row("trace", "group", 0)
CASES["query_rays_kernel<false, kBounded>"] = _row("bounded", "teapot", 0)
CASES["query_rays_kernel<true, kBounded>"] = _row("bounded", "group", 0)
CASES["query_rays_kernel<false, kAnyHit>"] = _row("occluded", "teapot", 0)
CASES["query_rays_kernel<true, kAnyHit>"] = _row("occluded", "group", 0)
# ---- the rest of the C ABI's kernels ---------------------------------------------------------------------------------------------
CASES["generate_rays_kernel"] = _row("rays", "teapot", 16)
CASES["untile_kernel"] = _row("untile", "teapot", 5)
CASES["quantise_kernel"] = _row("async", "teapot", 5, also=["render_tiles_packet_kernel<4, false, 7>"])

# ---- gate cases: the mask cache is on and the sample count asks for it, one guard refuses: the UNCACHED name must be reported -----
GATES = {
    "triangle coordinates beyond 2^30 (tris_bounded)": ("render_tiles_packet_kernel<32, false, 8>", _row("render", "atrium*2^27", 64)),
    "a sphere (kind != 0)": ("render_tiles_packet_kernel<32, false, 7>", _row("render", "sphere", 64)),
    "an object group": ("render_tiles_packet_kernel<16, false, 6, true>", _row("render", "group", 64)),
    "the stack beyond the registers": ("render_tiles_packet_kernel<32, true, 7>", _row("render", "teapot", 64, regs=LDS_REGS["teapot"])),
    "15 samples against 16": ("render_tiles_packet_kernel<8, false, 7>", _row("render", "teapot", 15)),
    "a pass of 4 S - 1 samples": ("render_tiles_packet_kernel<16, false, 7>", _row("render", "teapot", 63, samples=16)),
    "the option off": ("render_tiles_packet_kernel<32, false, 7>", _row("render", "teapot", 64, cache=0)),
}

# ---- ragged MP_FLAG_ACCUMULATE passes: selection follows the samples of the PASS; 70 samples per pixel in all --------------------
RAGGED = {
    "packets": (_row("render", "teapot", 70), [
        (40, "render_tiles_packet_kernel<8, false, 8, false, true>"), (17, "render_tiles_packet_kernel<4, false, 8, false, true>"),
        (8, "render_tiles_packet_kernel<8, false, 7>"), (4, "render_tiles_packet_kernel<4, false, 7>"), (1, "render_tiles_packet_kernel<1, false, 7>")]),
    "paths": (_row("paths", "teapot", 70), [
        (40, "render_paths_kernel<8, false, false, true>"), (17, "render_paths_kernel<8, false, false>"), (6, "render_paths_kernel<4, false, false>"),
        (4, "render_paths_kernel<4, false, false>"), (2, "render_paths_kernel<2, false, false>"), (1, "render_paths_kernel<1, false, false>")]),
}

# ---- the staged pipeline over several tile batches and sample chunks (tile_geometries "ragged26": 26 tiles in 64 x 64 slots) -----
# launch_render_paths_wavefront walks the tile list in batches of tb = 2^21 / (tile_size^2 * min(samples of the pass, 64)) tiles and
# every batch in chunks of 64 samples; at 64 samples or more tb = 8: batches of 8, 8, 8 and 2 tiles, chunks 64 + 6 at 70 samples.
# (scene, samples per pixel, the MP_FLAG_ACCUMULATE passes (one = a single launch), MP_FLAG_CHUNKED_SUM)
def staged_names(scene):
    """every kernel the staged pipeline launches for `scene` under the default options (the stack in registers)"""
    return set(_wf(scene.startswith("group"), False, scene.endswith("+rgb"))[2])


STAGED_TILES = 26
STAGED_BATCHES = {
    "teapot": ("teapot", 70, (70,), False),
    "teapot+rgb": ("teapot+rgb", 70, (70,), False),
    "group+rgb": ("group+rgb", 70, (70,), False),
    "teapot, passes 40 + 30": ("teapot", 70, (40, 30), False),
    "teapot+rgb, passes 40 + 30": ("teapot+rgb", 70, (40, 30), False),
    # sample chunks 64 + 36, 64 + 64 + 29 and 43 per batch; the flush of the first 256-sample chunk of the sum falls inside the second
    # pass (its last sample chunk); the {chunk sum, count, f64 total} slot is carried per tile across batches and passes
    "teapot, chunked sum, passes 100 + 157 + 43": ("teapot", 300, (100, 157, 43), True),
}
