"""Every render kernel family over the camera matrix (-m gpu): each case of tests/camera_cases.py (tests/test_camera_cases_cpu.py
shows what each is) through each route of camera_cases.ROUTES -- the cached packet walk and the same frame with the cache off at 64
samples per pixel, the 8-lane groups, the fused path kernel and its pooled form, the staged pipeline, the feature planes -- and
through mp_generate_rays and the mask cache's mask_cache_begin_unit (libmp_mask_probe.so).  Every comparison is on bit patterns
against the oracle at the same 15 floats: the f32 frame, the u8 image, the ray segments; the planes against tests/aov_model.py and
tests/aov_pass_model.py; the rays against mpo_sample_ray; the unit headers against tools/analytic_bounds.py.  Every test asserts
the kernel names its call reported, so the route named is the route run.  Two metamorphic checks stay on the GPU: the film scaled
by 2^-32 and 2^46 gives the GPU's own unscaled frame, and a cached-walk frame in two passes is the single launch.

The scene, the oracle's results per (case, kind, samples) and the GPU's frames per (case, route) are made once per module.
focus_zero and scaled_flush (camera_cases.NON_FINITE) send NaN or infinite directions through every walk; their test ids carry
their names, so `-k "focus_zero or scaled_flush"` and its negation split the file."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib
from tests import aov_model, aov_pass_model, camera_cases as cc
from tests import dispatch_cases as dc
from tests.conftest import TEAPOT
from tests.test_unit_bounds_cpu import _model, check_invariants, shipped_margin
from tests.test_unit_bounds_gpu import probe_units

pytestmark = pytest.mark.gpu

F = np.float32
FRAME_ROUTES = [r for r, row in cc.ROUTES.items() if row["api"] != "aov"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class World:
    """the context, the teapot on the GPU and in the oracle, the oracle's frames and the GPU's, each made once"""

    def __init__(self, oracle, bvh):
        import torch

        assert torch.cuda.is_available(), "gpu tests need a GPU"
        self.oracle, self.bvh, self.ctx = oracle, bvh, mp.Context(0)
        self.scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, self.ctx))
        self._expected, self._rendered = {}, {}

    def options(self, row=None):
        for k, v in {**dc.DEFAULTS, **(row["opts"] if row else {})}.items():
            self.ctx.set_option(k, v)

    def settings(self, case, row):
        paths = row["api"] in ("paths", "wf")
        return mp.RenderSettings(cc.TILE, row["spp"], case["res"], seed=cc.SEED, traversal=row.get("traversal", "packets"),
                                 max_depth=cc.DEPTH if paths else 0, wavefront=row["api"] == "wf")

    def expected(self, name, route):
        """the oracle's (f32, u8, ray segments) for the case at the route's kind and samples"""
        row, c = cc.ROUTES[route], cc.cases()[name]
        paths = row["api"] in ("paths", "wf")
        key = (name, paths, row["spp"])
        if key not in self._expected:
            w, h = c["res"]
            with np.errstate(all="ignore"):
                if paths:
                    f, u8, _, seg = self.bvh.render_image_paths_mt(c["sampler"], w, h, row["spp"], cc.SEED, cc.DEPTH, cc.TILE, 8)
                else:
                    f, u8, *_ = self.bvh.render_image_mt(c["sampler"], w, h, row["spp"], cc.SEED, cc.TILE, 8)
                    seg = w * h * row["spp"]
            self._expected[key] = (f, u8, seg)
        return self._expected[key]

    def rendered(self, name, route):
        """the GPU's (f32, u8, ray segments, kernel names) of the case through the route, one launch"""
        import torch

        if (name, route) not in self._rendered:
            row, c = cc.ROUTES[route], cc.cases()[name]
            self.options(row)
            try:
                fr = mp.FrameRenderer(self.scene, c["camera"], self.settings(c, row))
                fr.render()
                names = dc.launched(self.ctx)
                img, img8 = fr.untile()
                torch.cuda.synchronize()
                self._rendered[(name, route)] = (img.cpu().numpy(), img8.cpu().numpy(), int(fr.segments.item()), names)
            finally:
                self.options()
        return self._rendered[(name, route)]


@pytest.fixture(scope="module")
def world(oracle, teapot_oracle_bvh):
    w = World(oracle, teapot_oracle_bvh)
    yield w
    w.options()


def assert_names(names, expect):
    if isinstance(expect, set):
        assert set(names) == expect and len(names) == len(expect), names
    else:
        assert names == expect, names


@pytest.mark.parametrize("route", FRAME_ROUTES)
@pytest.mark.parametrize("name", cc.NAMES)
def test_frame(world, name, route):
    """the f32 frame, the u8 image and the segment count against the oracle at the same sampler; the kernels by name"""
    row = cc.ROUTES[route]
    of, ou8, oseg = world.expected(name, route)
    hit = int((of[..., 3] > 0).sum())
    # (the 100 / 100 condition of test_camera_cases_cpu.py is on the 16-spp frame: at 64 spp near_focus leaves fewer misses)
    # (a miss of the path extension carries the sky's radiance: only the reference-semantics frame of a non-finite case is all zero)
    paths = row["api"] in ("paths", "wf")
    assert (hit == 0 and not np.isnan(of).any() and (paths or not of.any())) if name in cc.NON_FINITE else 0 < hit < of[..., 3].size
    img, img8, seg, names = world.rendered(name, route)
    assert_names(names, row["names"])
    differing = int(np.sum(bits(img) != bits(of)))
    print(f"{name} / {route}: {differing} f32 values differ, {seg} segments")
    assert differing == 0, f"{name} / {route}: {differing} f32 values differ from the oracle's frame"
    assert np.array_equal(img8, ou8)
    assert seg == oseg
    if row["api"] in ("paths", "wf") and name not in cc.NON_FINITE:
        assert seg > of[..., 3].size * row["spp"], "paths bounce: more segments than camera rays"


@pytest.mark.parametrize("route", cc.SCALE_INVARIANT_ROUTES)
@pytest.mark.parametrize("name", ["scaled_mixed", "scaled_high"])
def test_film_scale_leaves_the_gpu_frame_unchanged(world, name, route):
    """a power of two is exact while nothing underflows: part of the scaled frame's waves take ray_dir's plain sqrtf and /, part the
    short sequences, and the frame is the GPU's own wide_pinhole frame, whose waves all take the short ones"""
    a, b = world.rendered(name, route), world.rendered("wide_pinhole", route)
    assert_names(a[3], cc.ROUTES[route]["names"])
    assert_names(b[3], cc.ROUTES[route]["names"])
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_two_passes_are_the_single_launch(world):
    """inf_focus_open on the cached walk as passes of 24 + 40 samples: each pass on the cached kernel its own count selects, the
    finished frame the single launch's and the oracle's"""
    import torch

    name, passes = cc.TWO_PASS
    row, c = cc.ROUTES["cached"], cc.cases()[name]
    single = world.rendered(name, "cached")
    world.options(row)
    try:
        fr = mp.FrameRenderer(world.scene, c["camera"], world.settings(c, row))
        nxt, seg = 0, 0
        for n, kernel in passes:
            nxt = fr.render_pass(nxt, n)
            assert dc.launched(world.ctx) == [kernel]
            seg += int(fr.segments.item())
        assert nxt == row["spp"]
        img, img8 = fr.untile()
        torch.cuda.synchronize()
    finally:
        world.options()
    of, ou8, oseg = world.expected(name, "cached")
    got = img.cpu().numpy()
    assert np.array_equal(bits(got), bits(single[0])) and np.array_equal(img8.cpu().numpy(), single[1]) and seg == single[2] == oseg
    assert np.array_equal(bits(got), bits(of)) and np.array_equal(img8.cpu().numpy(), ou8)


@pytest.mark.parametrize("name", cc.NAMES)
def test_feature_planes(world, name):
    """render_aov at 16 spp: shade, normal, albedo and ids against tests/aov_model.py; the same frame through render_aov_pass with
    the position plane against tests/aov_pass_model.py"""
    import torch

    row, c = cc.ROUTES["aov"], cc.cases()[name]
    w, h = c["res"]
    with np.errstate(all="ignore"):
        want = aov_model.planes(world.oracle, world.bvh.intersect, c["sampler"], w, row["spp"], cc.SEED, (0, 0, w, h))
        want6 = aov_pass_model.planes(world.oracle, world.bvh.intersect, c["sampler"], w, row["spp"], cc.SEED, (0, 0, w, h))
    hits = int(want["ids"][..., 3].sum())
    assert hits == 0 if name in cc.NON_FINITE else 0 < hits < w * h
    for k in want:
        assert np.array_equal(bits(want[k]), bits(want6[k])), "the two models agree on the planes they share"
    world.options(row)
    try:
        fr = mp.FrameRenderer(world.scene, c["camera"], world.settings(c, row))
        out = fr.render_aov()
        assert_names(dc.launched(world.ctx), row["names"])
        img = {k: fr.untile_plane(v) for k, v in out.items()}
        planes = fr.new_aov_planes(position=True)
        assert fr.render_aov_pass(planes) == row["spp"]
        assert_names(dc.launched(world.ctx), row["names"])
        img6 = {k: fr.untile_plane(v) for k, v in planes.items()}
        torch.cuda.synchronize()
    finally:
        world.options()
    for k in ("shade", "normal", "albedo", "ids"):
        got = img[k].cpu().numpy()
        assert np.array_equal(bits(got), bits(want[k])), (name, k, int(np.sum(bits(got) != bits(want[k]))))
    for k in ("position", "shade", "normal", "albedo", "ids"):
        got = img6[k].cpu().numpy()
        assert np.array_equal(bits(got), bits(want6[k])), (name, "pass", k, int(np.sum(bits(got) != bits(want6[k]))))


@pytest.mark.parametrize("name", cc.NAMES)
def test_generated_rays(world, name):
    """mp_generate_rays on one 16 x 16 block, samples 0-3: origin and direction bits against mpo_sample_ray"""
    import torch

    c, o = cc.cases()[name], world.oracle
    st = mp.RenderSettings(cc.TILE, 16, c["res"], seed=cc.SEED)
    blk = mp.ScreenBlock(*cc.RAYS_BLOCK)
    bufs = [torch.empty(blk.area(), dtype=torch.float32, device="cuda") for _ in range(6)]
    s, ss = c["camera"].build_sampler(c["res"]).as_struct(), st.as_struct()
    for sample in cc.RAYS_SAMPLES:
        _lib.check(_lib.lib().mp_generate_rays(world.ctx.handle, C.byref(s), C.byref(ss), blk.as_struct(), sample, *[b.data_ptr() for b in bufs], None))
        names = dc.launched(world.ctx)
        torch.cuda.synchronize()
        assert names == ["generate_rays_kernel"], names
        g = np.stack([b.cpu().numpy() for b in bufs], axis=1)
        exp = np.zeros_like(g)
        for i, (x, y) in enumerate(blk.internal_points()):
            r = o.sample_ray(c["sampler"], x, y, o.lib().mpo_sample_key(C.c_uint64(cc.SEED), c["res"][0], 16, x, y, sample))
            exp[i] = list(r.o) + list(r.d)
        bad = bits(g) != bits(exp)
        if bad.any():
            i, k = np.argwhere(bad)[0]
            print(f"{name}, sample {sample}: {int(bad.sum())} values differ, {int((bad & np.isnan(g) & np.isnan(exp)).sum())} of them NaN on both sides; "
                  f"first: ray {i} component {k}: {bits(g)[i, k]:#010x} against {bits(exp)[i, k]:#010x}")
        assert not bad.any(), (name, sample, int(bad.sum()))
        finite = np.isfinite(exp[:, 3:]).all()
        assert finite == (name not in cc.NON_FINITE)


@pytest.mark.parametrize("name", cc.NAMES)
def test_unit_headers(name):
    """mask_cache_begin_unit over all 384 units of the frame: the header equals analytic_bounds.header_words bit for bit where the
    unit adopts, with every tag cleared; a declined unit has state 0xFFFFFFFF and its tags untouched"""
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    ab = _model()
    c = cc.cases()[name]
    js = ab.jitter_scale()
    blocks = [(x, x + 1, y, y + 1) for y in range(0, c["res"][1], 2) for x in range(0, c["res"][0], 2)]
    got, ntags, margin = probe_units(c["values"], js, blocks)
    assert margin == np.float32(shipped_margin()) and got.shape[0] == 384
    adopted = 0
    with np.errstate(all="ignore"):
        for blk, g in zip(blocks, got):
            state, lo, hi = ab.corner_header(c["values"], js, *blk, margin)
            if state == 0xFFFFFFFF:
                assert g[12] == 0xFFFFFFFF and g[19] == 0, (name, blk)
                continue
            adopted += 1
            check_invariants(state, lo, hi)
            assert np.array_equal(g[:19], ab.header_words(state, lo, hi)), (name, blk, g[:19], ab.header_words(state, lo, hi))
            assert g[19] == ntags, (name, blk)
    print(f"{name}: {adopted} of 384 units adopted")
    if name in ("near_focus",) + cc.NON_FINITE:
        assert adopted == 0
    if name in ("inf_focus_open", "wide", "tele"):
        assert adopted >= 300
