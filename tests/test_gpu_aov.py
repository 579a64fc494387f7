"""GPU tests of the first-hit feature planes (mp_render_aov_device, include/minipath_hip.h; FrameRenderer.render_aov).  Every
comparison is on bit patterns with zero differences allowed: against the numpy model over the oracle (tests/aov_model.py), against
mp_render_tiles_device of the same settings, against mp_generate_rays + mp_trace_rays, and of the launch against itself under
other launch options, plane subsets and tile orders."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib, scenes
from tests import aov_model, meshes
from tests import dispatch_cases as dc
from tests.aov_model import bits
from tests.conftest import TEAPOT

pytestmark = pytest.mark.gpu

F = np.float32
NO = 0xFFFFFFFF
PLANES = ("shade", "normal", "albedo", "ids")
TABLE = [{"albedo": (0.9, 0.85, 0.8), "albedo2": (0.1, 0.15, 0.7), "checker": 6.0},
         ((0.7, 0.2, 0.3), (0.0, 0.0, 0.0)),
         {"albedo": 0.4, "emission": (1.5, 0.5, 0.0), "albedo2": (0.2, 0.9, 0.2), "checker": 0.75}]


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return mp.Context(0)


def _options(ctx, samples=0, cache=1, regs=64):
    ctx.set_option("packet_samples_in_flight", samples)
    ctx.set_option("packet_mask_cache", cache)
    ctx.set_option("packet_stack_registers", regs)


def _images(obj, cam, st, tiles=None, names=None, **which):
    """render_aov + untile_plane of every plane asked for: {name: [h, w, 4] numpy}; ids as uint32.  names: a list that receives the
    kernels the feature-plane launch reported"""
    import torch

    fr = mp.FrameRenderer(mp.Scene(obj), cam, st, tiles=tiles)
    out = fr.render_aov(**which)
    if names is not None:
        names += dc.launched(obj.ctx)
    img = {k: fr.untile_plane(v) for k, v in out.items()}
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if k == "ids" else v.cpu().numpy()) for k, v in img.items()}


def _same(got, want, what):
    for k in want:
        if k in got:
            diff = int(np.sum(bits(got[k]) != bits(want[k])))
            assert diff == 0, (what, k, diff)


def _look(eye, at=(0.0, 0.0, 0.0)):
    return mp.Camera.default().look_at(eye, at, (0, 1, 0))


def _scene(name, ctx, oracle):
    """(GPU object, camera, intersect(ray) -> oracle.Hit, material table or None)"""
    if name == "teapot":
        orc = oracle.Bvh.from_obj(TEAPOT)
        return mp.TriangleBvh.with_obj(TEAPOT, ctx), mp.Camera.teapot_view(), orc.intersect, None
    if name in ("soup_300", "grid_40", "sphere_24", "two_clusters"):
        pos, nrm, tex, tri = meshes.make(name)
        gpu, orc = mp.TriangleBvh.build(pos, nrm, tex, tri, ctx), oracle.Bvh.build(pos, nrm, tex, tri)
        return gpu, _look((0.4, 5.0, 4.5)), orc.intersect, None
    if name == "checker":  # a material per triangle, two of them checkers over the grid's texture coordinates
        pos, nrm, tex, tri = meshes.make("grid_40")
        mat = (np.arange(tri.shape[0]) % 3).astype(np.uint32)
        gpu = mp.TriangleBvh.build(pos, nrm, tex, tri, ctx, tri_material=mat)
        orc = oracle.Bvh.build(pos, nrm, tex, tri, tri_material=mat)
        gpu.set_materials(TABLE, 0.6)
        orc.set_materials(TABLE, 0.6)
        return gpu, _look((0.4, 5.0, 4.5)), orc.intersect, TABLE
    if name == "sphere":
        c, r = (0.2, 0.5, -0.3), 1.5
        return mp.Sphere(c, r, ctx), _look((0.4, 5.0, 4.5)), (lambda ray: oracle.sphere_intersect(c, r, ray)), None
    if name == "group":  # {teapot, soup x 2 rotated, sphere} under a coloured + checker table
        pos, nrm, tex, tri = meshes.make("soup_300")
        mat = (np.arange(tri.shape[0]) % 3).astype(np.uint32)
        teapot, ball = mp.TriangleBvh.with_obj(TEAPOT, ctx), mp.Sphere((0.4, 0, 0), 1.0, ctx)
        soup = mp.TriangleBvh.build(pos, nrm, tex, tri, ctx, tri_material=mat)
        o_teapot, o_soup = oracle.Bvh.from_obj(TEAPOT), oracle.Bvh.build(pos, nrm, tex, tri, tri_material=mat)
        tr = np.array([[0, 0, 0], [4.0, 1.5, -1.0], [-3.5, 2.0, 1.0], [0.0, 4.0, -1.0]], F)
        s = F(np.sqrt(0.5))
        q = np.array([[0, 0, 0, 1], [s, 0, 0, s], [0, 0.6, 0, 0.8], [0, 0, 0, 1]], F)
        gpu = mp.ObjectGroup([teapot, soup, soup, ball], tr, rotations=q)
        gpu.set_materials(TABLE, 0.5)
        box = oracle.Bvh.from_obj(TEAPOT)
        box.set_materials(TABLE, 0.5)
        box.set_group([o_teapot, o_soup, o_soup, ((0.4, 0.0, 0.0), 1.0)], tr, rotations=q)
        gpu._keep = (teapot, soup, ball, box, o_teapot, o_soup)
        return gpu, _look((1.0, 6.0, 13.0), (0.0, 2.0, 0.0)), box.intersect, TABLE
    if name == "instances":
        base = mp.TriangleBvh.with_obj(TEAPOT, ctx)
        tr = np.array([[0, 0, 0], [7.5, 0, -3], [-7.0, 0.5, -6], [0.25, 3.4, -1.0]], F)
        gpu = mp.Instances(base, tr)
        orc = oracle.Bvh.from_obj(TEAPOT)
        orc.set_instances(tr)
        gpu._keep = (base, orc)
        return gpu, _look((1.0, 6.0, 16.0), (0.0, 2.0, -2.0)), orc.intersect, None
    raise KeyError(name)


def _model(oracle, cam, isect, res, spp, seed, table):
    smp = oracle.sampler_from_array(cam.build_sampler(res).as_array())
    return aov_model.planes(oracle, isect, smp, res[0], spp, seed, (0, 0, res[0], res[1]), table)


# 5. all four planes equal the model, every scene kind; tiles 64 and 17 (clipped), a non-square frame
@pytest.mark.parametrize("name", ["teapot", "soup_300", "grid_40", "sphere_24", "two_clusters", "checker", "sphere", "group", "instances"])
def test_planes_equal_the_model(ctx, oracle, name):
    _options(ctx)
    gpu, cam, isect, table = _scene(name, ctx, oracle)
    res, spp, seed = (44, 36), 5, 9
    want = _model(oracle, cam, isect, res, spp, seed, table)
    hits = want["ids"][..., 3]
    assert 0 < hits.sum() < hits.size, "the case must hold hits and misses"
    if table is not None:
        assert len(np.unique(want["ids"][..., 2][hits == 1])) >= 2, "several materials in view"
    if name in ("group", "instances"):
        assert len(np.unique(want["ids"][..., 1][hits == 1])) >= 2, "several members in view"
    for ts in (64, 17):
        _same(_images(gpu, cam, mp.RenderSettings(ts, spp, res, seed=seed)), want, (name, ts))
    if name in ("teapot", "group"):  # the stack beyond 4 registers entries in LDS: the LDS-stack instantiations
        for spp2 in ((spp, 16) if name == "group" else (spp,)):
            w2 = want if spp2 == spp else _model(oracle, cam, isect, (24, 20), spp2, seed, table)
            r2 = res if spp2 == spp else (24, 20)
            _options(ctx, regs=4)
            _same(_images(gpu, cam, mp.RenderSettings(17, spp2, r2, seed=seed)), w2, (name, "lds stack", spp2))
            _options(ctx)
            _same(_images(gpu, cam, mp.RenderSettings(17, spp2, r2, seed=seed)), w2, (name, spp2))


# 6. sample counts that reach every S the launcher selects, with and without the mask cache: the template arguments of
# render_aov_packet_kernel each count must report (mask cache on, off, stack in LDS), and together they are every form of the
# kernel that a scene without members can select
AOV_FORMS = {1: ("1, false, 8", "1, false, 8", "1, true, 8"), 2: ("1, false, 8", "1, false, 8", "1, true, 8"),
             3: ("1, false, 8", "1, false, 8", "1, true, 8"), 10: ("4, false, 8", "4, false, 8", "1, true, 8"),
             16: ("4, false, 8, false, true", "16, false, 8", "16, true, 8"), 33: ("4, false, 8, false, true", "16, false, 8", "16, true, 8"),
             64: ("16, false, 8, false, true", "16, false, 8", "16, true, 8"), 100: ("16, false, 8, false, true", "16, false, 8", "16, true, 8")}
assert {f"render_aov_packet_kernel<{f}>" for forms in AOV_FORMS.values() for f in forms} == \
    {k for k, row in dc.CASES.items() if row["api"] == "aov" and not row["scene"].startswith("group")}


@pytest.mark.parametrize("spp", [1, 2, 3, 10, 16, 33, 64, 100])
def test_sample_counts_equal_the_model(ctx, oracle, spp):
    gpu, cam, isect, table = _scene("checker" if spp in (3, 33) else "teapot", ctx, oracle)
    res = (16, 12)
    want = _model(oracle, cam, isect, res, spp, 4, table)
    names = []
    for cache in (1, 0):
        _options(ctx, cache=cache)
        _same(_images(gpu, cam, mp.RenderSettings(16, spp, res, seed=4), names=names), want, (spp, cache))
    _options(ctx, regs=4)
    _same(_images(gpu, cam, mp.RenderSettings(16, spp, res, seed=4), names=names), want, (spp, "lds stack"))
    _options(ctx)
    assert names == [f"render_aov_packet_kernel<{f}>" for f in AOV_FORMS[spp]], names


def test_planes_do_not_depend_on_launch_options(ctx):
    gpu = mp.TriangleBvh.with_obj(TEAPOT, ctx)
    cam, st = mp.Camera.teapot_view(), mp.RenderSettings(32, 70, (96, 80), seed=2)
    _options(ctx)
    want = _images(gpu, cam, st)
    try:
        for samples in (1, 2, 4, 8, 16, 32, 64):
            for cache in (0, 1):
                _options(ctx, samples=samples, cache=cache)
                _same(_images(gpu, cam, st), want, (samples, cache))
    finally:
        _options(ctx)


def _atrium(ctx):
    pos, nrm, tex, tri = scenes.atrium(1, 0.05)
    return (pos, nrm, tex, tri), mp.TriangleBvh.build(pos, nrm, tex, tri, ctx)


def test_stand_in_tiles_equal_the_model(ctx, oracle):
    """The Sponza stand-in at reduced detail: a deep tree (the big-scene launch); a few tiles, with the stack in registers and in LDS."""
    (pos, nrm, tex, tri), gpu = _atrium(ctx)
    orc = oracle.Bvh.build(pos, nrm, tex, tri)
    cam, res, spp = scenes.atrium_camera(), (64, 48), 16
    tiles = [mp.ScreenBlock(16, 16, 32, 32), mp.ScreenBlock(48, 32, 64, 48)]
    smp = oracle.sampler_from_array(cam.build_sampler(res).as_array())
    st = mp.RenderSettings(16, spp, res, seed=13)
    for regs in (64, 8):
        _options(ctx, regs=regs)
        got = _images(gpu, cam, st, tiles=tiles)
        for t in tiles:
            blk = (t.min_x, t.min_y, t.max_x, t.max_y)
            want = aov_model.planes(oracle, orc.intersect, smp, res[0], spp, 13, blk)
            _same({k: v[blk[1]:blk[3], blk[0]:blk[2]] for k, v in got.items()}, want, (regs, blk))
    _options(ctx)


# 7. d_shade == mp_render_tiles_device, GPU against GPU, with and without MP_FLAG_PATHS in the AOV call's settings
@pytest.mark.parametrize("case", ["teapot", "atrium"])
def test_shade_equals_the_render(ctx, case):
    import torch

    _options(ctx)
    if case == "teapot":
        gpu, cam, res, tiles = mp.TriangleBvh.with_obj(TEAPOT, ctx), mp.Camera.teapot_view(), (256, 256), None
    else:
        gpu, cam, res = _atrium(ctx)[1], scenes.atrium_camera(), (256, 160)
        tiles = [mp.ScreenBlock(64, 32, 128, 96), mp.ScreenBlock(192, 96, 256, 160), mp.ScreenBlock(0, 0, 64, 64)]
    for spp in (16, 64):
        fr = mp.FrameRenderer(mp.Scene(gpu), cam, mp.RenderSettings(64, spp, res, seed=3), tiles=tiles)
        ref = fr.render().clone()
        for depth in (0, 4):
            fa = mp.FrameRenderer(mp.Scene(gpu), cam, mp.RenderSettings(64, spp, res, seed=3, max_depth=depth), tiles=tiles)
            out = fa.render_aov(normal=False, albedo=False, ids=False)
            torch.cuda.synchronize()
            assert list(out) == ["shade"]
            n = len(fr.tiles)
            diff = int((out["shade"][:n].view(torch.int32) != ref[:n].view(torch.int32)).sum().item())
            assert diff == 0, (case, spp, depth, diff)
            assert int(fa.segments.item()) == fa.samples_per_frame
        assert float(ref[..., 3].sum().item()) > 0


# 8. any subset of planes gives the same bits; tile_order permutations do not change them
def test_plane_subsets_and_tile_order(ctx):
    import torch

    _options(ctx)
    gpu = mp.TriangleBvh.with_obj(TEAPOT, ctx)
    gpu.set_materials([((0.2, 0.5, 0.9), 0.0)], 1.0)
    cam, st = mp.Camera.teapot_view(), mp.RenderSettings(17, 20, (100, 70), seed=6)
    want = _images(gpu, cam, st)
    for mask in range(1, 15):
        which = {k: bool(mask >> i & 1) for i, k in enumerate(PLANES)}
        got = _images(gpu, cam, st, **which)
        assert sorted(got) == sorted(k for k in PLANES if which[k])
        _same(got, want, which)
    fr = mp.FrameRenderer(mp.Scene(gpu), cam, st)
    n = len(fr.tiles)
    order = list(np.random.default_rng(3).permutation(n))
    fr._order_c = (C.c_uint32 * n)(*[int(i) for i in order])
    fr._extras.tile_order = C.cast(fr._order_c, C.POINTER(C.c_uint32))
    out = fr.render_aov()
    img = {k: fr.untile_plane(v) for k, v in out.items()}
    torch.cuda.synchronize()
    _same({k: (v.cpu().numpy().view(np.uint32) if k == "ids" else v.cpu().numpy()) for k, v in img.items()}, want, "tile order")
    assert int(fr.tile_cost[:n].min().item()) > 0  # d_tile_cost as in mp_render_tiles_device_ex


# 9. ids through mp_untile keep every bit; the id of sample 0 equals TriangleBvh.intersect of mp_generate_rays(sample=0)'s rays
def test_ids_survive_untile_and_equal_trace_rays(ctx):
    import torch

    _options(ctx)
    gpu = mp.TriangleBvh.with_obj(TEAPOT, ctx)
    cam, res = mp.Camera.teapot_view(), (96, 64)
    st = mp.RenderSettings(32, 7, res, seed=8)
    fr = mp.FrameRenderer(mp.Scene(gpu), cam, st)
    out = fr.render_aov(shade=False, normal=False, albedo=False)
    ids_t = out["ids"]
    img = fr.untile_plane(ids_t)
    torch.cuda.synchronize()
    assert img.dtype == torch.int32
    ids = img.cpu().numpy().view(np.uint32)
    tile_major = ids_t.cpu().numpy().view(np.uint32)
    for i, t in enumerate(fr.tiles):  # the scatter moved the bit patterns untouched
        assert np.array_equal(ids[t.min_y:t.max_y, t.min_x:t.max_x], tile_major[i, : t.max_y - t.min_y, : t.max_x - t.min_x])
    miss = ids[..., 3] == 0
    assert miss.any() and (~miss).any()
    assert np.all(ids[miss] == np.array([NO, 0, 0, 0], np.uint32))  # 0xFFFFFFFF (a NaN pattern as float) survives
    # sample 0's rays, traced by the ray API
    n = res[0] * res[1]
    rays = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(6)]
    smp, sts = cam.build_sampler(res).as_struct(), st.as_struct()
    _lib.check(_lib.lib().mp_generate_rays(ctx.handle, C.byref(smp), C.byref(sts), _lib.Block(0, 0, res[0], res[1]), 0,
                                           *[r.data_ptr() for r in rays], None))
    torch.cuda.synchronize()
    o, d = torch.stack(rays[:3], 1), torch.stack(rays[3:], 1)
    hit = gpu.intersect(o, d, full=True)
    torch.cuda.synchronize()
    prim = hit["prim"].cpu().numpy().view(np.uint32).reshape(res[1], res[0])
    assert np.array_equal(ids[..., 0], prim)
    assert np.array_equal(ids[..., 3], (prim != NO).astype(np.uint32))
    assert np.array_equal(ids[..., 2], np.where(prim != NO, hit["material"].cpu().numpy().view(np.uint32).reshape(res[1], res[0]), 0))


# 10. refusals and no-ops
def test_refusals_and_no_ops(ctx):
    import torch

    _options(ctx)
    L = _lib.lib()
    gpu = mp.TriangleBvh.with_obj(TEAPOT, ctx)
    cam, res = mp.Camera.teapot_view(), (32, 32)
    smp = cam.build_sampler(res).as_struct()
    tiles = (_lib.Block * 1)(_lib.Block(0, 0, 32, 32))
    buf = torch.full((32, 32, 4), 7.0, dtype=torch.float32, device="cuda")
    planes = _lib.AovPlanes(buf.data_ptr(), None, None, None)

    def call(st, n=1, pl=planes):
        return L.mp_render_aov_device(ctx.handle, gpu.handle, C.byref(smp), C.byref(st), tiles, n, C.byref(pl), None, None)

    base = mp.RenderSettings(32, 4, res, seed=1).as_struct()
    for flags, extra in ((_lib.MP_FLAG_ACCUMULATE, {}), (_lib.MP_FLAG_CHUNKED_SUM, {}),
                         (_lib.MP_FLAG_WAVEFRONT | _lib.MP_FLAG_PATHS, {"max_depth": 3}), (_lib.MP_FLAG_TRAVERSAL_GROUPS, {})):
        st = _lib.SettingsStruct.from_buffer_copy(base)
        st.flags |= flags
        for k, v in extra.items():
            setattr(st, k, v)
        assert call(st) == 5, flags  # MP_ERR_UNSUPPORTED
        assert L.mp_last_error()
    torch.cuda.synchronize()
    assert float(buf.min().item()) == 7.0  # nothing was launched
    assert call(base, n=0) == 0 and call(base, pl=_lib.AovPlanes()) == 0  # no-ops
    torch.cuda.synchronize()
    assert float(buf.min().item()) == 7.0
    bad = (_lib.Block * 1)(_lib.Block(0, 0, 40, 32))  # outside the resolution
    assert L.mp_render_aov_device(ctx.handle, gpu.handle, C.byref(smp), C.byref(base), bad, 1, C.byref(planes), None, None) == 1
    assert call(base) == 0
    torch.cuda.synchronize()
    assert float(buf[..., 3].max().item()) <= 1.0 and float(buf[..., 3].sum().item()) > 0
