"""GPU tests (-m gpu) of the cached packet walk's per-unit child lists (mask_cache.h unit_list_build; packet_walk.h trace_packet_cached).

A. The list builder itself, through the probe (mask_probe.hip, mp_mask_probe_list: the function the walk calls, behind a real call
   as in the walk), dword for dword against the numpy model (tests/unit_list_model.py build_list): the returned table value, the
   arena's fill, the tag and value of the node's slot and every entry.  The teapot: every node of both trees under the bounds of a
   handful of units.  atrium(1, 0.5): nodes on the hit chains of two dozen units under their own bounds, with the arena empty, nearly
   full (absorbing stops for want of room) and too full (the reset), and the top of the tree under bounds so wide that nothing is
   rejected -- the longest lists.

B. Frames, bit-equal to the oracle, with the kernels named: the teapot at 16 and 64 spp on the packet kernel, the feature-plane kernel
   and the path kernel's cached camera pass, and the eviction frame of tests/graft_model.py, under both tree formats; and the
   eviction frame again in the `lists_tiny` build of the library (minipath_amd/csrc/Makefile: four table slots, 32 arena entries),
   which counts its evictions, arena resets and the passes it leaves to the uncached walk.  The floors are a quarter of the rates
   the model counts on 38 units of that frame (tests/test_unit_lists_cpu.py: 0.21 evictions, 0.53 resets and 0.53 such passes per
   unit; the frame has 1 536 units of four passes).  That build once more for the counters themselves: the fused tiles, the feature
   planes and the fused paths are translation units with a copy of the counters each, and what the library reports is their sum.

The variant's frames are rendered in a process of its own (tests/walk_frames.py, run_in_variant): render_variant renders that frame
under both formats and returns the images and the counters; count_families one teapot frame from each of the three units and
the counters after each."""
import ctypes as C
import os

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib, scenes
from tests import aov_model
from tests import graft_model as gm
from tests import unit_list_model as ul
from tests.conftest import TEAPOT
from tests.dispatch_cases import launched
from tests.walk_frames import (CSRC, PROF_SLOTS, Counters, assert_same_bits, bits, check_formats, evict_oracle_image, frame, make_contexts, named, planes,
                               run_in_variant, set_options, teapot_oracle)

pytestmark = pytest.mark.gpu
F = np.float32


def render_variant():
    import torch

    prof = Counters(_lib.lib())
    out = {}
    for slots in (16, 8):
        ctx = mp.Context(0)
        ctx.set_option("packet_tree_slots", slots)
        obj = mp.TriangleBvh.build(*gm.evict_mesh(), ctx)
        assert obj.device_tree(packet=True)[0].shape[1] == slots
        fr = mp.FrameRenderer(mp.Scene(obj), scenes.atrium_camera(), mp.RenderSettings(gm.EVICT_TS, 64, gm.EVICT_RES, seed=gm.EVICT_SEED))
        prof.reset()
        fr.render()
        names = launched(ctx)
        assert names == ["render_tiles_packet_kernel<16, false, 8, false, true>"], names
        img, _ = fr.untile()
        torch.cuda.synchronize()
        out[f"image{slots}"] = img.cpu().numpy()
        out[f"counters{slots}"] = np.array(list(prof.read().values()), np.uint64)
    return out


def count_families():
    """a counted build: one teapot frame from each unit that runs the cached walk (fused tiles, feature planes, fused paths), the
    counters read -- summed over the units' copies -- after a reset and after every frame, then read with a reset and once more"""
    prof = Counters(_lib.lib())

    def read(reset=False):
        return list(prof.read(reset).values())

    ctx = mp.Context(0)
    obj = mp.TriangleBvh.with_obj(TEAPOT, ctx)
    cam, res, seed, ts = mp.Camera.teapot_view(), (64, 48), 21, 32
    prof.reset()
    rows, names = [read()], []
    names.append(frame(ctx, obj, cam, mp.RenderSettings(ts, 16, res, seed=seed))[2])
    rows.append(read())
    names.append(planes(ctx, obj, cam, mp.RenderSettings(ts, 16, res, seed=seed), ("ids", "albedo", "normal"))[1])
    rows.append(read())
    names.append(frame(ctx, obj, cam, mp.RenderSettings(ts, 32, res, seed=seed, max_depth=2))[2])
    rows.append(read())
    return dict(names=np.array(["\n".join(n) for n in names]), counters=np.array(rows, np.uint64), with_reset=np.array(read(True), np.uint64),
                after_reset=np.array(read(), np.uint64))


# ---- A ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def probe():
    so = os.path.join(CSRC, "libmp_mask_probe.so")
    if not os.path.exists(so):
        pytest.fail(f"{so} missing: run build() first")
    import torch

    # (the renderer's HIP runtime is initialised before the probe's copy loads, the order the whole suite has)
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    torch.zeros(1, device="cuda")
    L = C.CDLL(so)
    L.mp_mask_probe_list.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def _header_words(header):
    ab = gm._analytic_bounds()
    lo, hi, neg = header
    w = np.zeros(32, np.uint32)
    w[:19] = ab.header_words(0x100 | int(neg[0]) | int(neg[1]) << 1 | int(neg[2]) << 2, lo, hi)
    return w


def _run_probe(probe, nodes, cases):
    """cases: [(header, node, arena entries in use)] -> per case (value, fill afterwards, tag, slot value, arena dwords)"""
    info = np.zeros(3, np.uint32)
    stride = probe.mp_mask_probe_list_dwords()
    recs = np.ascontiguousarray(nodes, np.uint32)
    hdr = np.ascontiguousarray(np.stack([_header_words(h) for h, _, _ in cases]))
    cs = np.ascontiguousarray(np.array([[n, t] for _, n, t in cases], np.uint32))
    out = np.zeros((len(cases), stride), np.uint32)
    rc = probe.mp_mask_probe_list(recs.ctypes.data, nodes.shape[0], nodes.shape[1], hdr.ctypes.data, cs.ctypes.data, len(cases), out.ctypes.data,
                                  info.ctypes.data)
    assert rc == 0, rc
    entries, arena = ul.header_sizes()
    assert (int(info[0]), int(info[1])) == (arena, entries), "the probe was built with the header's sizes"
    return out, int(info[2])


def _compare(probe, nodes, cases):
    """every case against the model; returns what the cases covered"""
    out, arena_base = _run_probe(probe, nodes, cases)
    _, arena = ul.header_sizes()
    seen = {"lists": 0, "longest": 0, "overflows": 0, "room_stops": 0, "absorbed": 0, "not_nested": 0, "two_level_entries": 0, "empty": 0}
    for (header, node, top0), row in zip(cases, out):
        st = ul.new_stats()
        want = ul.build_list(nodes, node, header, arena - top0, st)
        val, fill, tag, slot_val = (int(v) for v in row[:4])
        if want is None:
            assert (val, fill, tag) == (0xFFFFFFFF, 0, 0xFFFFFFFF), (node, top0, hex(val), fill, hex(tag))
            seen["overflows"] += 1
            continue
        assert val == ((arena_base + top0) << 16 | len(want)), (node, top0, hex(val), len(want))
        assert (fill, tag, slot_val) == (top0 + len(want), node, val), (node, top0)
        got = row[4 + top0:4 + top0 + len(want)]
        assert np.array_equal(got, np.array(want, np.uint32)), (node, top0, got.tolist(), want)
        # nothing outside the list was written
        rest = np.concatenate([row[4:4 + top0], row[4 + top0 + len(want):]])
        assert ((rest & 0xFFFF0000) == 0xDEAD0000).all(), (node, top0)
        seen["lists"] += 1
        seen["longest"] = max(seen["longest"], len(want))
        seen["empty"] += not want
        for k in ("room_stops", "absorbed", "not_nested", "two_level_entries"):
            seen[k] += st[k]
    return seen


def _wide_header():
    """bounds under which no box can be rejected: origins anywhere around the scene, inverse directions from nearly axis-parallel
    to steep, all positive"""
    lo = np.array([[-1e3] * 3, [1e-3] * 3, [0.0] * 3], F)
    hi = np.array([[1e3] * 3, [1e3] * 3, [1.0] * 3], F)
    return lo, hi, np.zeros(3, bool)


@pytest.mark.parametrize("kind", ["packet", "wide"])
def test_teapot_lists_match_the_model(probe, oracle, kind):
    host = mp.TriangleBvh.with_obj(TEAPOT)
    nodes = (host.device_tree(packet=True) if kind == "packet" else host.device_tree())[0]
    assert nodes.shape[:2] == ((18, 16) if kind == "packet" else (27, 8))
    sarr = mp.Camera.teapot_view().build_sampler((64, 48)).as_array()
    headers = [up[0] for up in (ul.unit_passes(oracle, sarr, (64, 48), 64, 21, u, ul.shipped_margin()) for u in (5, 170, 400, 421, 700)) if up]
    assert len(headers) >= 4
    cases = [(h, n, 0) for h in headers + [_wide_header()] for n in range(nodes.shape[0])]
    seen = _compare(probe, nodes, cases)
    print(kind, seen)
    assert seen["lists"] == len(cases) and seen["absorbed"] > 0 and seen["longest"] >= 8


def atrium_cases(oracle, kind):
    """(nodes, cases) of the eviction scene's tree of one format"""
    host = gm.evict_host()
    nodes, root = (host.device_tree(packet=True) if kind == "packet" else host.device_tree())[:2]
    _, arena = ul.header_sizes()
    chains = gm.Chains(nodes, root, host.info().packet_count)
    sarr = scenes.atrium_camera().build_sampler(gm.EVICT_RES).as_array()
    orc = gm.evict_oracle(oracle)
    cases = []
    for u in range(7, 1536, 61):  # 26 units
        up = ul.unit_passes(oracle, sarr, gm.EVICT_RES, 64, gm.EVICT_SEED, u, ul.shipped_margin())
        if up is None:
            continue
        header, passes = up
        prim = orc.trace(passes[0][0], passes[0][1])[1]
        hit = sorted({int(p) >> 3 for p in prim if p != oracle.NO_PRIM})
        on_chain = sorted({n for p in hit[:4] for n in chains.chain(int(chains.node_of[p]))})
        picked = [root >> 6] + on_chain[:6]
        for i, n in enumerate(picked):
            cases.append((header, n, (0, arena - 20, arena - 3)[(u + i) % 3] if i else 0))
    wide = _wide_header()
    cases += [(wide, n, t) for n in [root >> 6] + list(range(0, nodes.shape[0], max(1, nodes.shape[0] // 12))) for t in (0, arena - 24)]
    return nodes, cases


@pytest.mark.parametrize("kind", ["packet", "wide"])
def test_atrium_lists_match_the_model(probe, oracle, kind):
    nodes, cases = atrium_cases(oracle, kind)
    assert 150 <= len(cases) <= 260, len(cases)
    seen = _compare(probe, nodes, cases)
    print(kind, len(cases), seen)
    # counted on the model, packet / wide: 161 / 191 cases, 9 / 8 lists that do not fit, 117 / 117 absorptions refused for want of
    # room, 28 / 47 kept inner children with a kept child that sticks out, 1 664 / 1 673 entries two or more levels down, the longest
    # list the whole arena (384).  Floors: a quarter.
    assert seen["overflows"] >= 2 and seen["room_stops"] >= 29 and seen["not_nested"] >= 7 and seen["two_level_entries"] >= 416, seen
    assert seen["longest"] >= 96, seen


@pytest.fixture(scope="module")
def ctxs():
    """one context per tree format, the launch options back at their defaults afterwards"""
    out = make_contexts()
    yield out
    for c in out.values():
        set_options(c)


# ---- B ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spp,s_in_flight", [(16, 4), (64, 16)])
def test_teapot_packet_kernel(ctxs, oracle, spp, s_in_flight):
    res, seed, ts = (64, 48), 21, 32
    of, ou8, _ = teapot_oracle(oracle, res, spp, seed, ts)
    assert 0.0 < of[..., 3].mean() < 1.0, "hits and misses in view"
    check_formats(ctxs, lambda c: mp.TriangleBvh.with_obj(TEAPOT, c), mp.Camera.teapot_view(), mp.RenderSettings(ts, spp, res, seed=seed),
                   (of, ou8), rf"render_tiles_packet_kernel<{s_in_flight}, false, 8, false, true>")


@pytest.mark.parametrize("spp,s_in_flight", [(16, 4), (64, 16)])
def test_teapot_feature_plane_kernel(ctxs, oracle, spp, s_in_flight):
    res, seed, ts = (64, 48), 21, 32
    smp = oracle.sampler_from_array(mp.Camera.teapot_view().build_sampler(res).as_array())
    want = aov_model.planes(oracle, oracle.Bvh.from_obj(TEAPOT).intersect, smp, res[0], spp, seed, (0, 0, *res))
    which = ("ids", "albedo", "normal")
    got = {}
    for slots, ctx in ctxs.items():
        img, names = planes(ctx, mp.TriangleBvh.with_obj(TEAPOT, ctx), mp.Camera.teapot_view(), mp.RenderSettings(ts, spp, res, seed=seed), which)
        assert names == [f"render_aov_packet_kernel<{s_in_flight}, false, 8, false, true>"], (slots, names)
        for k in which:
            assert_same_bits(img[k], want[k], (slots, k))
        got[slots] = img
    for k in which:
        assert np.array_equal(bits(got[16][k]), bits(got[8][k]))


@pytest.mark.parametrize("spp,cached", [(16, False), (32, True), (64, True)])
def test_teapot_path_kernel_cached_camera_pass(ctxs, oracle, spp, cached):
    """depth 2: the fused path kernel, whose camera pass runs the cached walk in units of spp / 8 passes -- from 32 spp on; at 16 the
    plan names the kernel without a cache (launch_plan.cpp), and the case checks that frame all the same"""
    res, seed, ts, depth = (64, 48), 21, 32, 2
    of, ou8, oseg = teapot_oracle(oracle, res, spp, seed, ts, depth)
    got = {}
    for slots, ctx in ctxs.items():
        f, u8, names, seg = frame(ctx, mp.TriangleBvh.with_obj(TEAPOT, ctx), mp.Camera.teapot_view(), mp.RenderSettings(ts, spp, res, seed=seed, max_depth=depth))
        assert names == ["render_paths_kernel<8, false, false, true>" if cached else "render_paths_kernel<8, false, false>"], (slots, names)
        assert_same_bits(f, of, slots)
        assert np.array_equal(u8, ou8) and seg == oseg, slots
        got[slots] = f
    assert np.array_equal(bits(got[16]), bits(got[8]))


def test_atrium_frame_both_formats(ctxs, oracle):
    of, ou8 = evict_oracle_image(oracle, 64)
    assert np.count_nonzero(of[..., 3]) > of.shape[0] * of.shape[1] // 2
    check_formats(ctxs, lambda c: mp.TriangleBvh.build(*gm.evict_mesh(), c), scenes.atrium_camera(),
                   mp.RenderSettings(gm.EVICT_TS, 64, gm.EVICT_RES, seed=gm.EVICT_SEED), (of, ou8), r"render_tiles_packet_kernel<16, false, 8, false, true>")


def test_atrium_frame_with_a_tiny_table_and_arena(oracle, tmp_path):
    got = run_in_variant("lists_tiny", "tests.test_unit_lists_gpu:render_variant", tmp_path, timeout=600)
    of, _ = evict_oracle_image(oracle, 64)
    units = gm.EVICT_RES[0] * gm.EVICT_RES[1] // 4
    for slots in (16, 8):
        c = named(got[f"counters{slots}"])
        builds, evictions, resets, left = c["list_builds"], c["evictions"], c["arena_resets"], c["passes_left_uncached"]
        print(f"lists_tiny, {slots} slots: per unit {builds / units:.2f} list builds, {evictions / units:.2f} evictions, {resets / units:.2f} arena resets, "
              f"{left / units:.2f} passes left to the uncached walk; {c['inner_links'] / (4 * units):.2f} inner links per pass")
        assert_same_bits(got[f"image{slots}"], of, slots)
        assert evictions >= units * 0.21 / 4 and resets >= units * 0.53 / 4 and left >= units * 0.53 / 4, (slots, evictions, resets, left)
        assert builds >= units and left <= resets


def test_counters_are_summed_over_the_units_that_run_the_cached_walk(tmp_path):
    """The fused tiles, the feature planes and the fused paths are translation units of their own, each with its own copy of the
    counted build's counters; mp_prof_read_n reports their sum and resets them all.  The teapot at (64, 48), one frame per unit: the
    packet kernel and the feature planes at 16 spp, and a depth-2 path frame at 32 spp -- the fewest samples at which the plan names
    the path kernel's cached row (launch_plan.cpp; at 16 it names the row without a cache, which counts nothing).  Slot 0, list
    builds, grows with every frame: no unit's counters are lost.  Exact counts are the business of the tests above."""
    got = run_in_variant("lists_tiny", "tests.test_unit_lists_gpu:count_families", tmp_path, timeout=600)
    names = [n.split("\n") for n in got["names"]]
    counters, with_reset, after_reset = got["counters"], got["with_reset"], got["after_reset"]
    builds = counters[:, PROF_SLOTS.index("list_builds")]
    print("list builds after the reset and after each frame:", builds.tolist())
    assert names == [["render_tiles_packet_kernel<4, false, 8, false, true>"], ["render_aov_packet_kernel<4, false, 8, false, true>"],
                     ["render_paths_kernel<8, false, false, true>"]], names
    assert counters.shape == (4, len(PROF_SLOTS)) and not counters[0].any(), "all the counters are zero after a reset"
    assert builds[0] < builds[1] < builds[2] < builds[3], builds
    assert np.array_equal(with_reset, counters[3]), "a read with reset = 1 still reports what was counted"
    assert not after_reset.any(), "... and leaves every unit's copy at zero"
