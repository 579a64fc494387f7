"""The long-wave cases (tests/long_waves.py) do what they claim, shown on the CPU through the launch plans (tests/plan_probe.py):
at the 32 CUs that an MI355X's launchers see under the context option blocks_per_cu = 1, every case plans to its kernel, its
grid is the cap (the cu_count term of the plan's min binds) and every wave gets at least the case's floor of work units; at the
card's 256 CUs the same frames give a wave one unit -- the regime the rest of the suite renders in."""
import pytest

import minipath_amd as mp
from minipath_amd import scenes
from tests import dispatch_cases as dc
from tests import graft_model as gm
from tests import long_waves as lw
from tests import plan_probe as pp


def test_the_table_of_pixels_per_unit_is_the_kernels():
    """the case data restates BW x BH of the kernels; the kernels' own lines, read out of the sources"""
    import os
    import re

    from tests.conftest import ROOT

    def src(name):
        return open(os.path.join(ROOT, "minipath_amd", "csrc", name)).read()

    packet = "constexpr int BW = (S <= 2) ? 8 : (S <= 8) ? 4 : (S <= 32) ? 2 : 1;  // pixel block = BW x BH, BW*BH*S == 64"
    assert src("kernels_tiles.hip").count(packet) == 1 and src("kernels_aov.hip").count(packet) == 1
    assert "const uint32_t bx = (ts + 3) / 4, by = (ts + 1) / 2, upt = bx * by, total = P.n_tiles * upt;" in src("kernels_tiles.hip")  # packet2
    groups = r"constexpr int BW = \(S == 1\) \? 8 : \(S == 2\) \? 8 : \(S == 4\) \? 4 : 4;\s*\n\s*constexpr int BH = 64 / S / BW;"
    assert re.search(groups, src("kernels_tiles.hip"))  # render_tiles_kernel
    assert "constexpr int BW = (S <= 2) ? 8 : (S <= 8) ? 4 : 2;" in src("kernels_paths.hip")
    assert "constexpr int S = 8, BW = 4, BH = 2, QN = 64 * NSUB;" in src("kernels_paths.hip")  # pooled
    assert "constexpr int S = 16, BW = 2, BH = 2;" in src("kernels_staged.hip")
    for s in (1, 2, 4, 8, 16, 32, 64):
        assert lw.pixels_per_unit(f"{lw.PK}<{s}, false, 7>") == 64 // s == lw.pixels_per_unit(lw.cached(s, lw.AOV))
    assert lw.PIXELS_PER_UNIT == {"render_tiles_packet2_kernel": 4 * 2, "render_paths_kernel": 4 * 2, "render_paths_pooled_kernel": 4 * 2,
                                  "wf_camera_kernel": 2 * 2, "render_tiles_kernel": 8 * 8}  # render_tiles_kernel<1, *>: S == 1, 8 x (64 / 1 / 8)
    for case in lw.CASES.values():
        assert case["ppu"] == lw.pixels_per_unit(case["kernels"][0])


@pytest.mark.parametrize("key, mesh", [("evict", gm.evict_mesh), ("interior", lambda: scenes.atrium(1, lw.SCENES["interior"]))])
def test_the_facts_of_the_added_scenes(key, mesh):
    """what long_waves.FACTS adds to dispatch_cases.FACTS is what the host builder exports for those meshes"""
    assert lw.SCENES["evict"] == gm.EVICT_DETAIL
    assert gm.plan_facts(mp.TriangleBvh.build(*mesh())) == lw.FACTS[key]
    assert all(lw.FACTS[k] == v for k, v in dc.FACTS.items())


def test_the_cases_are_the_issue_list():
    """about two million primary rays per packet case; one oracle frame per (scene, S) serves both formats"""
    for s, (res, spp) in lw.CACHED_FRAMES.items():
        assert res[0] * res[1] * spp == 1 << 21 and spp == 4 * s, s
    assert sum(c["formats"] for c in lw.CASES.values()) == 10
    assert {c["api"] for c in lw.CASES.values()} == {"render", "variant", "paths", "wf", "aov"}
    assert {k for c in lw.CASES.values() for k in c["kernels"]} <= set(pp.table())
    assert all(c["floor"] in (lw.FLOOR, lw.HALVED) and (c["floor"] == lw.FLOOR or c["api"] == "paths") for c in lw.CASES.values()), "only a path case may halve"


@pytest.mark.parametrize("key", list(lw.CASES))
def test_a_case_loops_under_the_lever(key):
    case = lw.CASES[key]
    cus = lw.CUS_LEVER
    assert cus == max(1, lw.CUS_FULL * 1 // 8)  # mp_ctx::launch_cus at blocks_per_cu = 1
    plans = lw.planned(case, cus)
    assert [n for p in plans for n in p["names"]] == list(case["kernels"]), "the plans name the case's kernels, in launch order"
    for i, p in enumerate(plans):
        # the grid is the cap: a whole number (1 .. 8) of resident blocks per CU, and below one unit per wave
        assert p["grid"] % cus == 0 and 1 <= p["grid"] // cus <= 8 and p["grid"] < (p["units"] + 3) // 4, (key, p["grid"], p["units"])
        floor = case["floor"] if i == 0 else lw.HALVED  # a later pass of the ragged frame: 8-pixel units of the same frame
        assert p["per_wave"] >= floor, (key, i, p["per_wave"])
    if case["kernels"][0].startswith("render_tiles_packet2_kernel"):
        assert plans[0]["units"] == plans[0]["out"].units2
    if case["api"] == "wf":  # the flat kernels take their grid-stride loops beyond the first step
        p = plans[0]
        assert p["flat_grid"] == cus * 16 and p["paths"] == 327680 and p["paths"] > 2 * p["flat_grid"] * 256


def test_no_case_loops_at_the_full_cu_count():
    """The gap the cases close: without the lever these very frames give a wave one work unit.  (The staged pipeline's camera
    kernel, 2 x 2-pixel units against the same cap of 8 192 waves, gets two -- still nothing like the sixteen of the lever.)"""
    per_wave = {key: max(p["per_wave"] for p in lw.planned(case, lw.CUS_FULL)) for key, case in lw.CASES.items()}
    assert per_wave.pop("staged pipeline") == 2
    assert max(per_wave.values()) <= 1, per_wave
