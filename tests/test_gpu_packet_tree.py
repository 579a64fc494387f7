"""GPU tests (-m gpu) of the cached packet walk on its two trees: the 16-slot PACKET tree (Context option "packet_tree_slots" = 16,
the default: frame words and cache entries node << 16 | 16-bit mask, 16 records per node) and the wide tree it falls back to
("packet_tree_slots" = 8: node << 8 | 8-bit mask; also what a scene with 2^16 packet-tree nodes or more gets).  Every case
renders on two contexts, one per format, names the cached kernel it ran (Context.last_kernels) and compares f32 bit patterns with
the oracle -- and therefore the two formats with each other.  The frames are small: the walk goes wrong in the format, not in the size.
The oracle's images are computed once per case and shared."""
import functools
import os
import re
import sys

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import scenes
from tests import aov_model
from tests import dispatch_cases as dc
from tests import tie_model as tm
from tests.conftest import TEAPOT

pytestmark = pytest.mark.gpu

SLOTS = (16, 8)
DETAIL = 0.1  # the stand-in of tests/test_packet_tree_cpu.py: thin top, non-nestable nodes, 212 packet-tree nodes against 280


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def ctxs():
    """one context per tree format; the scenes made on each take its format at upload"""
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    out = {}
    for s in SLOTS:
        c = mp.Context(0)
        c.set_option("packet_tree_slots", s)
        out[s] = c
    yield out
    for c in out.values():
        for k, v in dc.DEFAULTS.items():
            c.set_option(k, v)


def _options(ctx, **opts):
    for k, v in {**dc.DEFAULTS, **opts}.items():
        ctx.set_option(k, v)


def _frame(ctx, obj, cam, st, **opts):
    """one frame through FrameRenderer: (f32 image, u8 image, kernels reported, ray segments)"""
    import torch

    _options(ctx, **opts)
    try:
        fr = mp.FrameRenderer(mp.Scene(obj), cam, st)
        fr.render()
        names = dc.launched(ctx)
        img, img8 = fr.untile()
        torch.cuda.synchronize()
        return img.cpu().numpy(), img8.cpu().numpy(), names, int(fr.segments.item())
    finally:
        _options(ctx)


def _check_export(obj, slots):
    """the scene holds the format of its context: under "packet_tree_slots" = 8 the walk's tree is the wide tree byte for byte
    (with the root's record behind it), under 16 a 16-slot tree with at most as many nodes"""
    pk, proot, pbound, pabs, rec = obj.device_tree(packet=True)
    wide, wroot, wbound, wabs = obj.device_tree()
    assert pk.shape[1] == slots
    if slots == 8:
        assert pk.tobytes() == wide.tobytes() and (proot, pbound, pabs) == (wroot, wbound, wabs)
    else:
        assert pk.shape[0] <= wide.shape[0] and pabs >= wabs
    assert np.array_equal(rec[:6].view(np.float32), np.array([-np.inf] * 3 + [np.inf] * 3, np.float32)) and int(rec[6]) == proot


def _check_formats(ctxs, make_obj, cam, st, want, name_re, **opts):
    of, ou8 = want
    got = {}
    for slots, ctx in ctxs.items():
        obj = make_obj(ctx)
        _check_export(obj, slots)
        f, u8, names, _ = _frame(ctx, obj, cam, st, **opts)
        assert len(names) == 1 and re.fullmatch(name_re, names[0]), (slots, names)
        diff = int(np.sum(bits(f) != bits(of)))
        assert diff == 0, (slots, names, diff)
        assert np.array_equal(u8, ou8), slots
        got[slots] = f
    assert np.array_equal(bits(got[16]), bits(got[8]))


@functools.lru_cache(maxsize=None)
def _teapot_oracle(oracle, res, spp, seed, ts, depth=0):
    orc = oracle.Bvh.from_obj(TEAPOT)
    smp = oracle.sampler_from_array(mp.Camera.teapot_view().build_sampler(res).as_array())
    if depth:
        f, u8, _, seg = orc.render_image_paths_mt(smp, *res, spp, seed, depth, ts, 16)
        return f, u8, seg
    f, u8, *_ = orc.render_image_mt(smp, *res, spp, seed, ts, 16)
    return f, u8, None


@pytest.mark.parametrize("spp,s_in_flight", [(16, 4), (64, 16)])
def test_teapot_ragged_tiles(ctxs, oracle, spp, s_in_flight):
    """128 x 96 in tiles of 64: the bottom row of tiles is 32 high.  16 spp: units of four passes at 4 in flight; 64 spp: 16 in flight."""
    res, seed, ts = (128, 96), 21, 64
    of, ou8, _ = _teapot_oracle(oracle, res, spp, seed, ts)
    assert 0.0 < of[..., 3].mean() < 1.0, "hits and misses in view"
    _check_formats(ctxs, lambda c: mp.TriangleBvh.with_obj(TEAPOT, c), mp.Camera.teapot_view(), mp.RenderSettings(ts, spp, res, seed=seed),
                   (of, ou8), rf"render_tiles_packet_kernel<{s_in_flight}, false, 8, false, true>")


@functools.lru_cache(maxsize=None)
def _atrium():
    return scenes.atrium(1, DETAIL)


@functools.lru_cache(maxsize=None)
def _atrium_oracle(oracle, res, spp, seed, ts, fnum):
    orc = oracle.Bvh.build(*_atrium())
    cam = scenes.atrium_camera() if fnum is None else scenes.atrium_camera().f_number(fnum)
    smp = oracle.sampler_from_array(cam.build_sampler(res).as_array())
    f, u8, *_ = orc.render_image_mt(smp, *res, spp, seed, ts, 16)
    return f, u8


def test_stand_in_from_inside(ctxs, oracle):
    """The small-detail stand-in from the benchmark's interior view: every ray hits, the walk crosses the absorbed thin top of the tree
    in every pass and visits nodes with more than eight children (slots 8..15 of the mask, the high half of the record stride)."""
    res, spp, seed, ts = (96, 64), 64, 5, 32
    want = _atrium_oracle(oracle, res, spp, seed, ts, None)
    assert np.count_nonzero(want[0][..., 3]) > res[0] * res[1] // 2
    _check_formats(ctxs, lambda c: mp.TriangleBvh.build(*_atrium(), c), scenes.atrium_camera(), mp.RenderSettings(ts, spp, res, seed=seed),
                   want, r"render_tiles_packet_kernel<\d+, false, 8, false, true>")


def test_wide_lens_frame(ctxs, oracle):
    """A wide lens (f/1.2), 256 spp at 16 in flight: units of 16 passes whose origins spread over the lens and whose directions fan
    out, under bounds that mask_cache_begin_unit takes from the unit's corner rays.  Those bounds hold every pass of such a unit
    (counted on the model of tools/analytic_bounds.py for this very frame: no pass escapes, at any f-number down to 0.02), so this
    case is the packet kernel's parity under the widest bounds; the clear in the middle of a unit is the next case's."""
    res, spp, seed, ts = (96, 64), 256, 29, 32
    want = _atrium_oracle(oracle, res, spp, seed, ts, 1.2)
    assert np.count_nonzero(want[0][..., 3]) > res[0] * res[1] // 2
    _check_formats(ctxs, lambda c: mp.TriangleBvh.build(*_atrium(), c), scenes.atrium_camera().f_number(1.2),
                   mp.RenderSettings(ts, spp, res, seed=seed), want, r"render_tiles_packet_kernel<16, false, 8, false, true>",
                   packet_samples_in_flight=16)


def _units_with_escaping_passes(oracle, cam, res, spp, seed):
    """The fused path kernel's cached camera pass on the numpy model of the cache's bound-keeping (tools/analytic_bounds.py, Cache
    without corner bounds: the first cached pass of a unit sets the bounds, widened by a quarter): units of 4 x 2 pixels x 8
    samples per pass (render_paths_kernel<8>: lane = pixel * 8 + sample, passes at sample 0, 8, 16, ...); a pass whose rays may
    all use the cached walk with one sign pattern enters the cache.  Returns (units, units with a pass that left the bounds set
    before it -- a widen-and-clear of every tag in the middle of the unit)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import analytic_bounds as ab

    smp = oracle.sampler_from_array(cam.build_sampler(res).as_array())
    units = escaped = 0
    for y0 in range(0, res[1], 2):
        for x0 in range(0, res[0], 4):
            cache = ab.Cache(None, None, None, None)
            for s0 in range(0, spp, 8):
                rays = [oracle.sample_ray(smp, x0 + (l // 8) % 4, y0 + (l // 8) // 4,
                                          oracle.lib().mpo_sample_key(seed, res[0], spp, x0 + (l // 8) % 4, y0 + (l // 8) // 4, s0 + l % 8))
                        for l in range(64)]
                o, d, inv = (np.array([list(getattr(r, k)) for r in rays], np.float32) for k in ("o", "d", "inv"))
                neg = inv < 0
                if ab.ray_ok(o, d, inv).all() and (neg.all(0) | ~neg.any(0)).all():
                    cache.begin_pass(o, d, inv)
            units += 1
            escaped += cache.escapes > 0
    return units, escaped


def test_wide_lens_passes_leave_the_unit_bounds(ctxs, oracle):
    """Passes that leave the unit's bounds: the bounds widen and every node entry -- tags in the upper 16 bits under the packet
    tree's format -- is cleared to all-ones in the middle of a unit and refilled; a stale or mis-tagged entry would cull a child
    and lose hits.  The packet kernel's corner bounds are never left (above), so the case runs where a unit's first pass sets the
    bounds: the fused path kernel's cached camera pass, through a wide lens (f/1.2), depth 2, 32 spp = four passes per unit.  The
    premise is asserted on the model: the frame is 72 x 40 in tiles of 32, so every 4 x 2 unit lies inside one tile and the frame."""
    res, spp, seed, ts, depth = dc.RES, 32, 9, dc.TS, 2
    cam = mp.Camera.teapot_view().f_number(1.2)
    units, escaped = _units_with_escaping_passes(oracle, cam, res, spp, seed)
    assert units == 360 and escaped >= 10, (units, escaped)  # (counted: 35; 46 at the view's own f/4.8)
    orc = oracle.Bvh.from_obj(TEAPOT)
    smp = oracle.sampler_from_array(cam.build_sampler(res).as_array())
    of, ou8, _, oseg = orc.render_image_paths_mt(smp, *res, spp, seed, depth, ts, 16)
    assert 0.0 < of[..., 3].mean() < 1.0, "hits and misses in view"
    got = {}
    for slots, ctx in ctxs.items():
        obj = mp.TriangleBvh.with_obj(TEAPOT, ctx)
        f, u8, names, seg = _frame(ctx, obj, cam, mp.RenderSettings(ts, spp, res, seed=seed, max_depth=depth))
        assert names == ["render_paths_kernel<8, false, false, true>"], (slots, names)
        diff = int(np.sum(bits(f) != bits(of)))
        assert diff == 0 and np.array_equal(u8, ou8) and seg == oseg, (slots, diff)
        got[slots] = f
    assert np.array_equal(bits(got[16]), bits(got[8]))


def test_path_kernel_cached_camera_pass(ctxs, oracle):
    """The teapot at depth 2, 32 spp: the fused path kernel's camera pass runs the cached walk (units of four passes of 8)."""
    res, spp, seed, ts, depth = dc.RES, 32, 9, dc.TS, 2
    of, ou8, oseg = _teapot_oracle(oracle, res, spp, seed, ts, depth)
    got = {}
    for slots, ctx in ctxs.items():
        obj = mp.TriangleBvh.with_obj(TEAPOT, ctx)
        f, u8, names, seg = _frame(ctx, obj, mp.Camera.teapot_view(), mp.RenderSettings(ts, spp, res, seed=seed, max_depth=depth))
        assert names == ["render_paths_kernel<8, false, false, true>"], (slots, names)
        diff = int(np.sum(bits(f) != bits(of)))
        assert diff == 0 and np.array_equal(u8, ou8), (slots, diff)
        assert seg == oseg and seg > res[0] * res[1] * spp
        got[slots] = f
    assert np.array_equal(bits(got[16]), bits(got[8]))


def test_tie_scene_feature_planes(ctxs, oracle):
    """meshes.doubled("grid_40"): every triangle twice, the copies under different materials, so the ids and albedo planes show which
    of two triangles with the same t won (the lower lane).  16 spp: the cached feature-plane kernel, units of four passes."""
    import torch

    mesh, key = "grid_40", "render_aov_packet_kernel<4, false, 8, false, true>"
    row = tm.AOV_CASES[key]
    pos, nrm, tex, tri, *_ = tm.arrays(mesh)
    mat = tm.material_ids(mesh, "copy")
    orc = tm.oracle_scene(oracle, mesh, "copy")
    orc.set_materials(tm.RGB, tm.SKY)
    want = aov_model.planes(oracle, orc.intersect, tm.sampler(oracle), tm.RES[0], row["spp"], tm.SEED, (0, 0, *tm.RES), tm.RGB)
    ids = want["ids"].reshape(-1, 4)
    hit = ids[:, 3] == 1
    assert 0 < hit.sum() < hit.size and len(np.unique(ids[hit, 2])) == 2, "hits and misses, winners of both materials"
    got = {}
    for slots, ctx in ctxs.items():
        gpu = mp.TriangleBvh.build(pos, nrm, tex, tri, ctx, tri_material=mat)
        gpu.set_materials(tm.RGB, tm.SKY)
        _options(ctx, **row["opts"])
        try:
            fr = mp.FrameRenderer(mp.Scene(gpu), tm.camera(), mp.RenderSettings(tm.TS, row["spp"], tm.RES, seed=tm.SEED))
            out = fr.render_aov()
            names = dc.launched(ctx)
            img = {k: fr.untile_plane(out[k]).cpu().numpy() for k in ("ids", "albedo")}
            torch.cuda.synchronize()
        finally:
            _options(ctx)
        assert names == [key], (slots, names)
        for k in ("ids", "albedo"):
            diff = int(np.sum(bits(img[k]) != bits(want[k])))
            assert diff == 0, (slots, k, diff)
        got[slots] = img
    for k in ("ids", "albedo"):
        assert np.array_equal(bits(got[16][k]), bits(got[8][k]))
