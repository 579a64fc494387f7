"""GPU tests of the feature planes in progressive passes (mp_render_aov_pass_device, include/minipath_hip.h;
FrameRenderer.new_aov_planes / render_aov_pass).  Every comparison is on f32 / u32 bit patterns with zero differences allowed:
the six planes against the numpy model over the oracle (tests/aov_pass_model.py), the four old planes against
mp_render_aov_device (the code as it was), any split into passes against the single launch, the state between passes against
mp_render_tiles_device's own MP_FLAG_ACCUMULATE state and against the model's state_after(k), previews against the host's
state * (1 / k), and every instantiation of render_aov_packet_kernel through the new entry point."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib, io
from tests import aov_pass_model
from tests import dispatch_cases as dc
from tests.aov_pass_model import FLOAT_PLANES, PLANES, bits
from tests.conftest import TEAPOT
from tests.test_aov_passes_cpu import SPLITS
from tests.test_gpu_aov import _options, _scene
from tests.test_gpu_dispatch_matrix import SEED, World

pytestmark = pytest.mark.gpu

F = np.float32
OLD = ("shade", "normal", "albedo", "ids")
ALL = {k: True for k in PLANES}
A = "render_aov_packet_kernel"
SENTINEL = 0x5A5A5A5A
SMALL = dict(res=(24, 16), ts=16, spp=5, seed=9)   # 1 920 rays: the model's size; the right column of tiles is clipped
BIG = dict(res=(72, 40), ts=32, spp=70, seed=2)    # 201 600 rays: 3 x 2 tiles, right column and bottom row clipped


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    c = mp.Context(0)
    yield c
    _options(c)


def _renderer(gpu, cam, case, **kw):
    return mp.FrameRenderer(mp.Scene(gpu), cam, mp.RenderSettings(case["ts"], case["spp"], case["res"], seed=case["seed"], **kw))


def _host(planes):
    """tile-major tensors -> {name: numpy}, synchronising"""
    import torch

    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in planes.items()}


def _scatter(fr, a):
    """mp_untile on the host: tile-major [n, ts, ts, 4] -> image-major [h, w, 4], bit patterns untouched"""
    w, h = fr.settings.resolution
    img = np.zeros((h, w, 4), a.dtype)
    for i, t in enumerate(fr.tiles):
        img[t.min_y:t.max_y, t.min_x:t.max_x] = a[i, : t.max_y - t.min_y, : t.max_x - t.min_x]
    return img


def _passes(fr, split, which=ALL, planes=None, names=None, begin=0):
    """the passes of `split` from `begin` on, on fresh planes unless given; names receives the kernels each pass reported"""
    planes = fr.new_aov_planes(**which) if planes is None else planes
    for count in split:
        nxt = fr.render_aov_pass(planes, begin, count)
        assert nxt == (begin + count if count else int(fr.settings.sample_count))
        if names is not None:
            names.append(dc.launched(fr.ctx))
        begin = nxt
    return planes


def _same(got, want, what, keys=None):
    for k in (keys or want):
        diff = int(np.sum(bits(got[k]) != bits(want[k])))
        assert diff == 0, (what, k, diff)


@pytest.fixture(scope="module")
def big(ctx):
    """the teapot at 72 x 40 x 70: the renderer, one whole-frame launch of the six planes, mp_render_aov_device's four"""
    _options(ctx)
    gpu = mp.TriangleBvh.with_obj(TEAPOT, ctx)
    fr = _renderer(gpu, mp.Camera.teapot_view(), BIG)
    names = []
    whole = _host(_passes(fr, (70,), names=names))
    assert names == [[A + "<16, false, 8, false, true>"]]
    assert int(fr.segments.item()) == fr.samples_per_frame
    old = _host(fr.render_aov())
    hit = whole["ids"].view(np.uint32)[..., 3]
    assert 0 < hit.sum() < 72 * 40, "the view must hold hits and misses"
    return {"gpu": gpu, "fr": fr, "whole": whole, "old": old}


_frames = {}


def _small_case(name, ctx, oracle):
    """(GPU object, camera, aov_pass_model.Frame) of a scene of tests/test_gpu_aov.py at 24 x 16 x 5; the model is computed once"""
    gpu, cam, isect, table = _scene(name, ctx, oracle)
    if name not in _frames:
        smp = oracle.sampler_from_array(cam.build_sampler(SMALL["res"]).as_array())
        _frames[name] = aov_pass_model.Frame(oracle, isect, smp, SMALL["res"][0], SMALL["spp"], SMALL["seed"], (0, 0, *SMALL["res"]), table)
    return gpu, cam, _frames[name]


# 1. the six planes equal the model; the four old ones also equal mp_render_aov_device.  group / instances: rotated and translated
# members, so that the point must be the world ray's
@pytest.mark.parametrize("name", ["teapot", "checker", "sphere", "group", "instances"])
def test_new_planes_equal_the_model(ctx, oracle, name):
    _options(ctx)
    gpu, cam, frame = _small_case(name, ctx, oracle)
    want = frame.planes()
    assert 0 < frame.hit.sum() < frame.hit.size, "the case must hold hits and misses"
    if name in ("group", "instances"):
        assert len(np.unique(want["ids"][..., 1][want["ids"][..., 3] == 1])) >= 2, "several members in view"
    assert np.any(want["position"][..., :3] != 0) and np.any(want["shade_sq"][..., 0] != want["shade"][..., 0])
    fr = _renderer(gpu, cam, SMALL)
    got = _host(_passes(fr, (0,)))
    assert sorted(got) == sorted(PLANES)
    img = {k: _scatter(fr, v) for k, v in got.items()}
    _same(img, want, name, PLANES)
    _same(got, _host(fr.render_aov()), (name, "mp_render_aov_device"), OLD)
    # the scatter on the device moves the same bits, the new planes included
    two = _passes(fr, (0,), {k: k in ("position", "shade_sq") for k in PLANES})
    _same(_host({k: fr.untile_plane(v) for k, v in two.items()}), want, (name, "untile_plane"), ("position", "shade_sq"))


# 2. any split equals the single launch, and the kernels follow the pass
@pytest.mark.parametrize("split", [(40, 17, 8, 4, 1), (64, 6), (1, 69)])
def test_any_split_equals_the_single_launch(ctx, big, split):
    _options(ctx)
    names = []
    got = _host(_passes(big["fr"], split, names=names))
    assert names == [[A + n] for n in SPLITS[split]], names
    _same(got, big["old"], (split, "mp_render_aov_device"), OLD)
    _same(got, big["whole"], (split, "whole frame"), PLANES)


# 3. state and previews between passes
def test_state_and_previews_between_passes(ctx, big):
    import torch

    _options(ctx)
    fr = big["fr"]
    beauty = _renderer(big["gpu"], mp.Camera.teapot_view(), BIG)
    planes, begin, names = fr.new_aov_planes(**ALL), 0, []
    for count in (40, 17, 13):
        _passes(fr, (count,), planes=planes, names=names, begin=begin)
        assert int(fr.segments.item()) == sum(t.area() for t in fr.tiles) * count  # pixels x samples of the pass
        assert beauty.render_pass(begin, count) == begin + count
        begin += count
        torch.cuda.synchronize()
        state = _host(planes)
        assert np.array_equal(bits(state["shade"]), bits(beauty.tile_buf.cpu().numpy())), ("render_pass state", begin)
        if begin < 70:
            cnt = state["shade"][..., 3]
            assert np.array_equal(cnt, np.round(cnt)) and cnt.max() == begin, "hit counts, not means"
            for k in FLOAT_PLANES:
                if k != "normal":
                    assert np.array_equal(bits(state[k][..., 3]), bits(cnt)), k
                img = fr.untile_plane(planes[k], preview_samples=begin)
                torch.cuda.synchronize()
                want = (_scatter(fr, state[k]) * (F(1) / F(begin))).astype(F)
                assert np.array_equal(bits(img.cpu().numpy()), bits(want)), ("preview", k, begin)
                assert np.array_equal(bits(planes[k].cpu().numpy()), bits(state[k])), "the preview only reads"
    assert names == [[A + n] for n in SPLITS[(40, 17, 13)]], names
    _same(_host(planes), big["whole"], "(40, 17, 13)", PLANES)


def test_state_equals_the_model_and_ids_are_written_once(ctx, oracle):
    _options(ctx)
    gpu, cam, frame = _small_case("teapot", ctx, oracle)
    fr = _renderer(gpu, cam, SMALL)
    planes = _passes(fr, (2,))
    state = {k: _scatter(fr, v) for k, v in _host(planes).items()}
    _same(state, frame.state_after(2), "state after (2) of (2, 3)", PLANES)
    _passes(fr, (3,), planes=planes, begin=2)
    final = {k: _scatter(fr, v) for k, v in _host(planes).items()}
    _same(final, frame.planes(), "(2, 3)", PLANES)
    assert np.array_equal(bits(state["ids"]), bits(final["ids"])), "ids after pass one are the final ids"
    # a later pass does not touch the plane: a sentinel stays
    p2 = _passes(fr, (2,))
    p2["ids"].fill_(SENTINEL)
    _passes(fr, (3,), planes=p2, begin=2)
    got = _host(p2)
    assert np.all(got["ids"].view(np.uint32) == SENTINEL)
    _same({k: _scatter(fr, v) for k, v in got.items()}, final, "sentinel run", FLOAT_PLANES)


# 4. every instantiation through the new entry point, whole and as two ragged passes
@pytest.fixture(scope="module")
def world(oracle):
    w = World(oracle)
    yield w
    w.options()


@pytest.mark.parametrize("name", [k for k, row in dc.CASES.items() if row["api"] == "aov"])
def test_every_instantiation_through_the_new_entry(world, name):
    row = dc.CASES[name]
    world.options(row)
    s = world.scene(row["scene"])
    spp = row["spp"]
    fr = mp.FrameRenderer(mp.Scene(s["gpu"]), s["cam"], mp.RenderSettings(dc.AOV_TS, spp, dc.AOV_RES, seed=SEED))
    names = []
    whole = _host(_passes(fr, (0,), names=names))
    assert names == [[name]], names
    old = _host(fr.render_aov())
    assert world.kernels() == [name]
    hit = old["ids"].view(np.uint32)[..., 3]
    assert 0 < hit.sum() < dc.AOV_RES[0] * dc.AOV_RES[1], "the view must hold hits and misses"
    _same(whole, old, (name, "mp_render_aov_device"), OLD)
    cut = spp // 2 + 1
    two = _host(_passes(fr, (cut, spp - cut)))
    _same(two, whole, (name, "two ragged passes"), PLANES)
    world.options()


# 5. plane subsets and tile order
def test_plane_subsets_and_tile_order(ctx):
    _options(ctx)
    gpu = mp.TriangleBvh.with_obj(TEAPOT, ctx)
    gpu.set_materials([((0.2, 0.5, 0.9), 0.0)], 1.0)
    case = dict(res=(40, 24), ts=16, spp=20, seed=6)
    fr = _renderer(gpu, mp.Camera.teapot_view(), case)
    want = _host(_passes(fr, (0,)))
    split = (7, 13)
    for names in (("normal",), ("position",), ("shade_sq", "ids"), ("normal", "ids"), ("albedo", "position"), PLANES):
        which = {k: k in names for k in PLANES}
        got = _host(_passes(fr, split, which))
        assert sorted(got) == sorted(names)
        _same(got, want, names, names)
    n = len(fr.tiles)
    order = list(np.random.default_rng(3).permutation(n))
    fr._order_c = (C.c_uint32 * n)(*[int(i) for i in order])
    fr._extras.tile_order = C.cast(fr._order_c, C.POINTER(C.c_uint32))
    _same(_host(_passes(fr, split)), want, "tile order", PLANES)


# 6. checkpoint and resume
def test_checkpoint_and_resume(ctx, big, tmp_path):
    _options(ctx)
    fr = big["fr"]
    planes = _passes(fr, (10, 7))
    ck = str(tmp_path / "planes.npz")
    io.save_checkpoint(ck, fr, 17, planes=planes)
    resumed = _renderer(big["gpu"], mp.Camera.teapot_view(), BIG)
    fresh = resumed.new_aov_planes(**ALL)
    nxt = io.load_checkpoint(ck, resumed, planes=fresh)
    assert nxt == 17
    _passes(resumed, (30, 23), planes=fresh, begin=nxt)
    _same(_host(fresh), big["whole"], "resumed", PLANES)
    other = _renderer(big["gpu"], mp.Camera.teapot_view(), {**BIG, "spp": 71})
    with pytest.raises(ValueError, match="other settings"):
        io.load_checkpoint(ck, other, planes=other.new_aov_planes(**ALL))


# 7. refusals and no-ops
def test_refusals_and_no_ops(ctx):
    import torch

    _options(ctx)
    L = _lib.lib()
    gpu = mp.TriangleBvh.with_obj(TEAPOT, ctx)
    cam, res = mp.Camera.teapot_view(), (32, 32)
    smp = cam.build_sampler(res).as_struct()
    tiles = (_lib.Block * 1)(_lib.Block(0, 0, 32, 32))
    bufs = [torch.full((32, 32, 4), 7.0, dtype=torch.float32, device="cuda") for _ in range(6)]
    size = C.sizeof(_lib.AovPlanesEx)
    planes = _lib.AovPlanesEx(size, *[b.data_ptr() for b in bufs])

    def call(st, n=1, pl=planes):
        return L.mp_render_aov_pass_device(ctx.handle, gpu.handle, C.byref(smp), C.byref(st), tiles, n, C.byref(pl), None, None)

    def untouched():
        torch.cuda.synchronize()
        return all(float(b.min().item()) == 7.0 and float(b.max().item()) == 7.0 for b in bufs)

    def settings(flags=0, **extra):
        st = _lib.SettingsStruct.from_buffer_copy(mp.RenderSettings(32, 4, res, seed=1).as_struct())
        st.flags |= flags
        for k, v in extra.items():
            setattr(st, k, v)
        return st

    ACC = _lib.MP_FLAG_ACCUMULATE
    for st in (settings(_lib.MP_FLAG_CHUNKED_SUM), settings(_lib.MP_FLAG_CHUNKED_SUM | ACC, pass_count=2),
               settings(_lib.MP_FLAG_WAVEFRONT | _lib.MP_FLAG_PATHS, max_depth=3), settings(_lib.MP_FLAG_TRAVERSAL_GROUPS)):
        assert call(st) == 5, st.flags  # MP_ERR_UNSUPPORTED
        assert L.mp_last_error()
    assert untouched()
    for st in (settings(ACC, pass_begin=4), settings(ACC, pass_begin=9), settings(ACC, pass_begin=2, pass_count=3)):
        assert call(st) == 1, (st.pass_begin, st.pass_count)  # MP_ERR_INVALID: a pass outside [0, sample_count)
    assert call(settings(), pl=_lib.AovPlanesEx(4, *[b.data_ptr() for b in bufs])) == 1  # struct_size
    assert call(settings(), pl=_lib.AovPlanesEx(size - 8, *[b.data_ptr() for b in bufs])) == 1
    assert untouched()
    assert call(settings(), n=0) == 0 and call(settings(), pl=_lib.AovPlanesEx(size)) == 0  # no-ops
    assert call(settings(ACC, pass_begin=1, pass_count=2), pl=_lib.AovPlanesEx(size)) == 0
    assert untouched()
    # the old entry point keeps its refusal of passes
    old = _lib.AovPlanes(bufs[0].data_ptr(), None, None, None)
    assert L.mp_render_aov_device(ctx.handle, gpu.handle, C.byref(smp), C.byref(settings(ACC)), tiles, 1, C.byref(old), None, None) == 5
    assert untouched()
    # and the same arguments without a reason to refuse render: a first pass leaves sums, MP_FLAG_PATHS is ignored
    assert call(settings(ACC | _lib.MP_FLAG_PATHS, pass_count=3, max_depth=4)) == 0
    torch.cuda.synchronize()
    cnt = bufs[0][..., 3]
    assert float(cnt.max().item()) == 3.0 and float(cnt.min().item()) == 0.0
    assert call(settings(ACC, pass_begin=3)) == 0
    torch.cuda.synchronize()
    assert float(bufs[0][..., 3].max().item()) == 1.0 and all(float(b[..., 3].sum().item()) > 0 for b in bufs[:3] + bufs[4:])
