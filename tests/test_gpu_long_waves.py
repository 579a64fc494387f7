"""GPU tests (-m gpu) of the render kernels on waves that run many work units each: the cases of tests/long_waves.py, rendered with
the context option blocks_per_cu = 1 -- the launchers then see cu_count / 8 CUs, 1 024 waves on an MI355X, and every wave draws
eight or more units in a row from the work queues -- and compared with the oracle's frame of the same input: f32 bit patterns,
the u8 image, the ray segments, the kernels by name.  What a wave keeps between two units (the mask cache's header, tables and
list arena, the empty-leaf marks, the parked feature sums, the LDS stack and ray queue, the pooled path kernel's slab) is thereby
held on every kernel family; the frames that the other tests compare whole with the oracle give a wave one unit.

Every test recomputes the units per wave of its case from the live cu_count through the launch plans (tests/plan_probe.py), prints
them, and FAILS if the case falls below its floor on the card it runs on: a case that does not loop tests nothing new.  On a
mismatch the number of differing words and the first differing tile are reported.  The option is set on contexts of this module's
own and goes back to 0 in a `finally` (tests/walk_frames.py set_options).  Oracle frames are cached per (scene, frame, spp, depth)."""
import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib, scenes
from tests import graft_model as gm
from tests import long_waves as lw
from tests.conftest import TEAPOT
from tests.dispatch_cases import launched
from tests.test_gpu_dispatch_matrix import World  # the matrix's scenes (teapot, group, atrium, "+rgb") with their oracle twins
from tests.walk_frames import Counters, bits, frame, make_contexts, named, planes, run_in_variant, set_options

pytestmark = pytest.mark.gpu
LEVER = {"blocks_per_cu": 1}


class Rig:
    """the module's contexts (one for the matrix's scenes, one per tree format), the scenes on them, the oracle's frames"""

    def __init__(self, oracle):
        self.oracle = oracle
        self.world = World(oracle)
        self.ctxs = make_contexts()
        self._objects, self._twins, self._frames = {}, {}, {}

    def contexts(self):
        return [self.world.ctx, *self.ctxs.values()]

    def mesh(self, key):
        return gm.evict_mesh() if key == "evict" else scenes.atrium(1, lw.SCENES[key])

    def camera(self, key):
        return self.world.scene(key)["cam"] if lw.SCENES[key] == "matrix" else scenes.atrium_camera()

    def object(self, key, slots=None):
        """(context, device object) of a scene: on the context of a tree format, or on the matrix's"""
        if slots is None and lw.SCENES[key] == "matrix":
            return self.world.ctx, self.world.scene(key)["gpu"]
        ctx = self.world.ctx if slots is None else self.ctxs[slots]
        if (key, slots) not in self._objects:
            assert "+" not in key
            obj = mp.TriangleBvh.with_obj(TEAPOT, ctx) if key == "teapot" else mp.TriangleBvh.build(*self.mesh(key), ctx)
            if slots is not None:
                assert obj.device_tree(packet=True)[0].shape[1] == slots
            self._objects[key, slots] = obj
        return ctx, self._objects[key, slots]

    def twin(self, key):
        if lw.SCENES[key] == "matrix":
            return self.world.scene(key)["orc"]
        if key not in self._twins:
            self._twins[key] = gm.evict_oracle(self.oracle) if key == "evict" else self.oracle.Bvh.build(*self.mesh(key))
        return self._twins[key]

    def expected(self, key, res, spp, depth):
        """the oracle's frame, on 16 threads, once: (f32, u8, ray segments)"""
        k = (key, res, spp, depth)
        if k not in self._frames:
            smp = self.oracle.sampler_from_array(self.camera(key).build_sampler(res).as_array())
            if depth:
                f, u8, _, seg = self.twin(key).render_image_paths_mt(smp, *res, spp, lw.SEED, depth, lw.TS, 16)
            else:
                f, u8, *_ = self.twin(key).render_image_mt(smp, *res, spp, lw.SEED, lw.TS, 16)
                seg = res[0] * res[1] * spp
            assert 0 < np.count_nonzero(f[..., 3]), "the view holds hits"
            self._frames[k] = (f, u8, seg)
        return self._frames[k]


@pytest.fixture(scope="module")
def rig(oracle):
    r = Rig(oracle)
    yield r
    for c in r.contexts():
        set_options(c)


def loops(key, ctx):
    """the case's launches at the CUs the launchers see under the lever on this card; fails if a wave gets fewer units than the floor"""
    case = lw.CASES[key]
    cus = max(1, ctx.cu_count // 8)  # mp_ctx::launch_cus at blocks_per_cu = 1
    plans = lw.planned(case, cus)
    for i, p in enumerate(plans):
        print(f"{key}: {p['names'][0]}: {p['units']} units on {4 * p['grid']} waves ({ctx.cu_count} CUs, {cus} under the lever): "
              f"{p['per_wave']:.2f} units per wave")
        floor = case["floor"] if i == 0 else lw.HALVED
        assert p["per_wave"] >= floor, f"{key}: {p['per_wave']:.2f} units per wave on this card, the case needs {floor}"
    return plans


def assert_frame(got, want, ts, what):
    """f32 bit patterns (or an int32 plane's); on a mismatch the differing words and the first differing tile"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = bits(got) != bits(want)
    if diff.any():
        ys, xs = np.nonzero(diff.any(axis=-1))
        y, x = int(ys[0]), int(xs[0])
        tiles = np.unique(ys // ts * (want.shape[1] // ts) + xs // ts)
        pytest.fail(f"{what}: {int(diff.sum())} of {diff.size} words differ in {len(tiles)} tiles; the first at pixel ({x}, {y}) "
                    f"of tile ({x // ts}, {y // ts}): got {got[y, x].tolist()}, want {want[y, x].tolist()}")


def same_names(names, case):
    if case["api"] == "wf":
        assert set(names) == set(case["kernels"]) and len(names) == len(case["kernels"]), names
    else:
        assert names == list(case["kernels"]), names


def settings(case):
    return mp.RenderSettings(case["ts"], case["spp"], case["res"], seed=lw.SEED, traversal=case["traversal"], max_depth=case["depth"],
                             wavefront=case["api"] == "wf", shuffle_tiles=case["shuffle"])


def check_scene_facts(rig, key, obj):
    """the live scene reports what the plans were given (long_waves.FACTS; the matrix's own scenes: test_scene_facts there)"""
    if lw.SCENES[key] != "matrix":
        want, info = lw.FACTS[key], obj.info()
        assert (info.stack_bound, len(obj.device_tree()[0]), info.packet_count) == (want["stack_bound"], want["nodes"], want["packets"])


def run_case(rig, key):
    """a "render" / "paths" / "wf" case in one launch: per context the names, the frame, the u8 image and the segments"""
    case = lw.CASES[key]
    assert case["passes"] is None and case["api"] in ("render", "paths", "wf")
    of, ou8, oseg = rig.expected(case["scene"], case["res"], case["spp"], case["depth"])
    got = {}
    for slots in (16, 8) if case["formats"] else (None,):
        ctx, obj = rig.object(case["scene"], slots)
        check_scene_facts(rig, case["scene"], obj)
        loops(key, ctx)
        f, u8, names, seg = frame(ctx, obj, rig.camera(case["scene"]), settings(case), **case["opts"], **LEVER)
        same_names(names, case)
        assert_frame(f, of, case["ts"], (key, slots))
        assert np.array_equal(u8, ou8), (key, slots)
        assert seg == oseg, (key, slots, seg, oseg)
        if case["depth"]:
            assert seg > case["res"][0] * case["res"][1] * case["spp"], "paths bounce: more segments than camera rays"
        got[slots] = f
        assert ctx.options["blocks_per_cu"] == 0, "the lever is back at its default"
    if case["formats"]:
        assert np.array_equal(bits(got[16]), bits(got[8]))


ONE_LAUNCH = [k for k, c in lw.CASES.items() if c["api"] in ("render", "paths", "wf") and c["passes"] is None]


@pytest.mark.parametrize("key", [k for k in ONE_LAUNCH if lw.CASES[k]["formats"]])
def test_cached_walk(rig, key):
    """The cached packet walk at 4, 8, 16 and 32 samples in flight, under both tree formats, on the teapot view -- units that miss,
    units on the silhouette and interior units alternate inside one wave -- and on the eviction scene from inside: the header,
    the tables, the list arena and the empty-leaf marks of a unit meet the next unit of the same wave eight times over."""
    run_case(rig, key)


def test_cached_walk_ragged_accumulate_passes(rig):
    """The 16-in-flight teapot frame as MP_FLAG_ACCUMULATE passes of 64 + 32 samples in shuffled tile order, against the oracle's
    96-spp frame: the passes select the 16- and the 8-in-flight cached kernels; the second runs four units per wave (8-pixel units
    of the same frame)."""
    import torch

    key = "cached walk, teapot, ragged passes 64 + 32"
    case = lw.CASES[key]
    of, ou8, oseg = rig.expected(case["scene"], case["res"], case["spp"], 0)
    got = {}
    for slots in (16, 8):
        ctx, obj = rig.object(case["scene"], slots)
        loops(key, ctx)
        set_options(ctx, **case["opts"], **LEVER)
        try:
            fr = mp.FrameRenderer(mp.Scene(obj), rig.camera(case["scene"]), settings(case))
            nxt, seen, seg = 0, [], 0
            for n, _, _ in case["passes"]:
                nxt = fr.render_pass(nxt, n)
                seen += launched(ctx)
                seg += int(fr.segments.item())
            img, img8 = fr.untile()
            torch.cuda.synchronize()
        finally:
            set_options(ctx)
        assert nxt == case["spp"] and seen == list(case["kernels"]), seen
        got[slots] = img.cpu().numpy()
        assert_frame(got[slots], of, case["ts"], (key, slots))
        assert np.array_equal(img8.cpu().numpy(), ou8) and seg == oseg, (slots, seg, oseg)
    assert np.array_equal(bits(got[16]), bits(got[8]))


def render_tiny():
    """in a process that loaded the `lists_tiny` build: the case's frame under both tree formats with the lever set, and the
    build's counters after each"""
    import torch

    case = lw.CASES["cached walk, lists_tiny build, evict, 16 in flight"]
    prof = Counters(_lib.lib())
    out = {}
    for slots in (16, 8):
        ctx = mp.Context(0)
        ctx.set_option("packet_tree_slots", slots)
        obj = mp.TriangleBvh.build(*gm.evict_mesh(), ctx)
        assert obj.device_tree(packet=True)[0].shape[1] == slots
        set_options(ctx, **case["opts"], **LEVER)
        try:
            fr = mp.FrameRenderer(mp.Scene(obj), scenes.atrium_camera(), settings(case))
            prof.reset()
            fr.render()
            names = launched(ctx)
            img, _ = fr.untile()
            torch.cuda.synchronize()
        finally:
            set_options(ctx)
        assert names == list(case["kernels"]), names
        out[f"image{slots}"] = img.cpu().numpy()
        out[f"counters{slots}"] = np.array(list(prof.read().values()), np.uint64)
        out["cu_count"] = np.array([ctx.cu_count])
    return out


def test_cached_walk_with_a_tiny_table_and_arena(rig, tmp_path):
    """The eviction scene at 16 in flight in the `lists_tiny` build (four table slots, 32 arena entries), one child process for both
    formats: the frame is the oracle's, and the build's counters show evictions and arena resets -- lists die in mid-unit, and the
    next unit of the same wave starts on what they left."""
    key = "cached walk, lists_tiny build, evict, 16 in flight"
    case = lw.CASES[key]
    loops(key, rig.world.ctx)
    of, _, _ = rig.expected(case["scene"], case["res"], case["spp"], 0)
    got = run_in_variant("lists_tiny", "tests.test_gpu_long_waves:render_tiny", tmp_path, timeout=600)
    assert int(got["cu_count"][0]) == rig.world.ctx.cu_count
    n_units = lw.units(case)
    for slots in (16, 8):
        c = named(got[f"counters{slots}"])
        print(f"lists_tiny, {slots} slots: {n_units} units, {c['list_builds']} list builds, {c['evictions']} evictions, {c['arena_resets']} arena resets, "
              f"{c['passes_left_uncached']} passes left to the uncached walk")
        assert_frame(got[f"image{slots}"], of, case["ts"], (key, slots))
        assert c["evictions"] > 0 and c["arena_resets"] > 0 and c["list_builds"] >= n_units, c


@pytest.mark.parametrize("key", [k for k in ONE_LAUNCH if lw.CASES[k]["api"] == "render" and not lw.CASES[k]["formats"]])
def test_uncached_and_other_tile_kernels(rig, key):
    """The uncached packet walk with its stack in registers and in LDS, the big-scene form, two rays per lane, an object group and
    the 8-lane-group kernel (its LDS ray queue and stacks)."""
    run_case(rig, key)


@pytest.mark.parametrize("key", [k for k in ONE_LAUNCH if lw.CASES[k]["api"] == "paths"])
def test_path_kernels(rig, key):
    """The fused path kernels with and without the cached camera pass, and the pooled kernels with two and four sub-passes, whose
    pool slab in global memory outlives the unit -- once more on the interior scene, where every path survives, the queue stays
    full and all of the slab is rewritten per unit.  Frames and segment counts."""
    run_case(rig, key)


def test_staged_pipeline(rig):
    """wf_camera_kernel at sixteen units per wave; the flat kernels (vertex, scan, scatter, accumulate) beyond the first step of
    their grid-stride loops; all six kernels named."""
    key = "staged pipeline"
    p = loops(key, rig.world.ctx)[0]
    assert p["paths"] > p["flat_grid"] * 256, "the flat kernels' grid-stride loops take a second step"
    run_case(rig, key)


@pytest.mark.parametrize("key", [k for k, c in lw.CASES.items() if c["api"] == "aov"])
def test_feature_planes(rig, key):
    """The feature-plane kernel's parked sums.  tests/aov_model.py costs one ctypes call per ray and cannot hold two million rays, so
    every plane under blocks_per_cu = 1 must equal, bit for bit, the plane of the same call under blocks_per_cu = 0: a comparison
    between two runs of the same kernel, the weaker of the two made here -- it holds the many-unit regime against the
    one-unit-per-wave regime that the model verifies at small sizes.  The stronger: the "shade" plane is the plain render's image
    (tests/test_gpu_aov.py, test_shade_equals_the_render), so it is also compared with the oracle's frame."""
    case = lw.CASES[key]
    ctx, obj = rig.object(case["scene"])
    loops(key, ctx)
    st, cam = settings(case), rig.camera(case["scene"])
    looped, names = planes(ctx, obj, cam, st, lw.PLANES, **LEVER)
    assert names == list(case["kernels"]), names
    assert ctx.options["blocks_per_cu"] == 0
    single, names = planes(ctx, obj, cam, st, lw.PLANES)
    assert names == list(case["kernels"]), names
    of, _, _ = rig.expected(case["scene"], case["res"], case["spp"], 0)
    assert_frame(looped["shade"], of, case["ts"], (key, "shade against the oracle"))
    for k in lw.PLANES:
        assert_frame(looped[k], single[k], case["ts"], (key, k, "blocks_per_cu 1 against 0"))
    hit = looped["ids"][..., 3]
    assert 0 < hit.sum() < hit.size, "the view holds hits and misses"
