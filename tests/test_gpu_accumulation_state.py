"""GPU tests (-m gpu) of the running accumulation state between progressive passes, all bit for bit: the three-channel path
kernels against the oracle (cached and uncached camera pass, every samples-in-flight width, staged pipeline, pooled fall-back,
coloured object group), rgb previews of unfinished passes (mp_untile_preview, mp_render_pass_multi gathers), multi-device passes
that are all or nothing, and the host-staged gather ("multi_gather_staged").  Contexts share this box's GPU."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from tests import meshes
from tests.conftest import TEAPOT

pytestmark = pytest.mark.gpu
SEED = 0x5EED
RES, TS = (96, 64), 32
# one material, coloured and checkered (the teapot has no texture coordinates: the checker reads the origin's cell)
RGB_TABLE = [{"albedo": (0.9, 0.45, 0.2), "emission": (0.05, 0.0, 0.1), "albedo2": (0.2, 0.6, 0.9), "checker": 3.0}]
GREY_TABLE = [(0.75, 0.0)]  # the default material: grey 0.75, no emission
SKY = 0.8
RAGGED = (1, 2, 3, 5, 9, 0)  # 1, 2, 2, 4, 8 samples in flight, then the rest (8)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def sync():
    import torch

    torch.cuda.synchronize()


def host(t):
    sync()
    return t.cpu().numpy()


def teapot_rgb(ctx):
    bvh = mp.TriangleBvh.with_obj(TEAPOT, ctx)
    bvh.set_materials(RGB_TABLE, SKY)
    return bvh


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"


@pytest.fixture(scope="module")
def orc_rgb(oracle):
    b = oracle.Bvh.from_obj(TEAPOT)
    b.set_materials(RGB_TABLE, SKY)
    return b


@pytest.fixture(scope="module")
def rgb_frame(oracle, orc_rgb):
    """(spp, depth) -> the oracle's (f32, u8, segments) of the coloured teapot view"""
    memo = {}

    def get(spp, depth, res=RES):
        key = (spp, depth, res)
        if key not in memo:
            of, ou8, _, seg = orc_rgb.render_image_paths_mt(oracle.build_sampler(oracle.teapot_camera(), *res), res[0], res[1], spp, SEED,
                                                            depth, TS, 8)
            memo[key] = (of, ou8, seg)
        return memo[key]

    return get


def oracle_u8(oracle, img):
    """mpo_color_to_image of every pixel of an image-major f32 frame"""
    flat = np.ascontiguousarray(img, np.float32).reshape(-1, 4)
    out = np.zeros(flat.shape, np.uint8)
    f, o = flat.ctypes.data, out.ctypes.data
    fn, fp, up = oracle.lib().mpo_color_to_image, C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    for i in range(flat.shape[0]):
        fn(C.cast(f + 16 * i, fp), C.cast(o + 4 * i, up))
    return out.reshape(img.shape)


def expected_preview(state, tiles, k, res):
    """mp_untile_preview's definition in numpy f32: every channel of the running state times 1.0f / k"""
    w, h = res
    img = np.zeros((h, w, 4), np.float32)
    inv = np.float32(1.0) / np.float32(k)
    for i, t in enumerate(tiles):
        img[t.min_y:t.max_y, t.min_x:t.max_x] = state[i, :t.height(), :t.width()] * inv
    return img


def check_preview(oracle, fr, k):
    """FrameRenderer.untile(preview_samples=k) of a coloured render against the definition and the oracle's quantisation"""
    img, u8 = fr.untile(preview_samples=k)
    got, got8 = host(img), host(u8)
    exp = expected_preview(host(fr.tile_buf), fr.tiles, k, fr.settings.resolution)
    for c in range(4):
        assert np.array_equal(bits(got[..., c]), bits(exp[..., c])), (k, "rgba"[c], int(np.sum(bits(got[..., c]) != bits(exp[..., c]))))
    assert np.any(got[..., 0] != got[..., 2]), k  # the preview really is coloured
    assert np.array_equal(got8, oracle_u8(oracle, got)), k
    return got, got8


# ---- A. three-channel kernels against the oracle ------------------------------------------------------------------

@pytest.mark.parametrize("spp,depth", [(40, 4), (70, 3), (33, 5)])
@pytest.mark.parametrize("mask_cache", [1, 0])
def test_rgb_teapot_frame(gpu, rgb_frame, spp, depth, mask_cache):
    """The coloured teapot at 32 or more samples per launch: render_paths_kernel<8, false, true, true> (mask cache on) and
    <8, false, true, false> (off) against the oracle: f32, u8 and segment count."""
    c = mp.Context(0)
    c.set_option("packet_mask_cache", mask_cache)
    fr = mp.FrameRenderer(mp.Scene(teapot_rgb(c)), mp.Camera.teapot_view(), mp.RenderSettings(TS, spp, RES, seed=SEED, max_depth=depth))
    fr.render()
    img, u8 = fr.untile()
    of, ou8, seg = rgb_frame(spp, depth)
    assert np.any(of[..., 0] != of[..., 2])
    got = host(img)
    assert np.array_equal(bits(got), bits(of)), (spp, depth, mask_cache, int(np.sum(bits(got) != bits(of))))
    assert np.array_equal(host(u8), ou8) and int(fr.segments.item()) == seg


@pytest.mark.parametrize("wavefront", [False, True])
def test_rgb_ragged_passes_and_previews(gpu, oracle, rgb_frame, wavefront):
    """Ragged passes (1, 2, 3, 5, 9 samples, then the rest) carry {sum r, sum g, sum b, hits} through every samples-in-flight
    width of the fused kernel and through wf_accumulate_kernel's three-channel branch; the preview after every unfinished pass
    scales each channel on its own; the last pass gives the oracle's frame and segment count."""
    spp, depth = 40, 4
    c = mp.Context(0)
    fr = mp.FrameRenderer(mp.Scene(teapot_rgb(c)), mp.Camera.teapot_view(),
                          mp.RenderSettings(TS, spp, RES, seed=SEED, max_depth=depth, wavefront=wavefront))
    nxt, segs = 0, 0
    for count in RAGGED:
        nxt = fr.render_pass(nxt, count)
        segs += int(fr.segments.item())
        if nxt < spp:
            check_preview(oracle, fr, nxt)
    assert nxt == spp
    img, u8 = fr.untile()
    of, ou8, seg = rgb_frame(spp, depth)
    assert np.array_equal(bits(host(img)), bits(of)) and np.array_equal(host(u8), ou8)
    assert segs == seg


@pytest.mark.parametrize("mode", [2, 3])
def test_rgb_table_under_paths_pooled(gpu, rgb_frame, mode):
    """paths_pooled 2 / 3 ask for the pooled kernel, which carries one channel: a coloured table must fall back to the one-pass
    kernel and give the oracle's frame, whole and in passes of 16 and more."""
    spp, depth = 40, 4
    c = mp.Context(0)
    c.set_option("paths_pooled", mode)
    scene = mp.Scene(teapot_rgb(c))
    st = mp.RenderSettings(TS, spp, RES, seed=SEED, max_depth=depth)
    of, ou8, seg = rgb_frame(spp, depth)
    fr = mp.FrameRenderer(scene, mp.Camera.teapot_view(), st)
    fr.render()
    img, u8 = fr.untile()
    assert np.array_equal(bits(host(img)), bits(of)) and np.array_equal(host(u8), ou8) and int(fr.segments.item()) == seg
    fp = mp.FrameRenderer(scene, mp.Camera.teapot_view(), st)
    fp.render_pass(fp.render_pass(0, 17))
    img, _ = fp.untile()
    assert np.array_equal(bits(host(img)), bits(of))


def test_coloured_object_group_fused_wavefront_ragged(gpu, oracle):
    """The coloured object group of test_coloured_and_checker_materials (a grid twice, one turned, and a Sphere) fused and staged,
    whole and in ragged passes with previews: render_paths_kernel<S, true, true> for S = 1 .. 8 and the staged object walk."""
    ctx = mp.Context(0)
    pos, nrm, tex, tri = meshes.make("grid_40")
    mat = (np.arange(tri.shape[0]) % 3).astype(np.uint32)
    bvh = mp.TriangleBvh.build(pos, nrm, tex, tri, ctx, tri_material=mat)
    orc = oracle.Bvh.build(pos, nrm, tex, tri, tri_material=mat)
    table = [{"albedo": (0.9, 0.85, 0.8), "albedo2": (0.1, 0.15, 0.7), "checker": 6.0},
             ((0.7, 0.2, 0.3), (0.0, 0.0, 0.0)),
             {"albedo": 0.4, "emission": (1.5, 0.5, 0.0), "albedo2": (0.2, 0.9, 0.2), "checker": 0.75}]
    eye, at = (0.4, 5.0, 4.5), (0.0, 0.0, 0.0)
    cam = mp.Camera.default().look_at(eye, at, (0, 1, 0))
    oc = oracle.Camera()
    oracle.lib().mpo_camera_default(C.byref(oc))
    oracle.lib().mpo_camera_look_at(C.byref(oc), oracle.vec3(*eye), oracle.vec3(*at), oracle.vec3(0, 1, 0))
    res, spp, depth, ts = (96, 80), 24, 4, 32
    ball_def = ((0.3, 1.4, 0.2), 0.8)
    tr = np.array([[0, 0, 0], [0.5, 2.5, -0.5], [0, 0, 0]], np.float32)
    rot = np.array([[0, 0, 0, 1], [np.sqrt(0.5), 0, 0, np.sqrt(0.5)], [0, 0, 0, 1]], np.float32)
    grp = mp.ObjectGroup([bvh, bvh, mp.Sphere(*ball_def, ctx)], tr, rotations=rot)
    grp.set_materials(table, 0.5)
    orc.set_materials(table, 0.5)
    orc.set_group([orc, orc, ball_def], tr, rotations=rot)
    og, ou8, _, gseg = orc.render_image_paths_mt(oracle.build_sampler(oc, *res), res[0], res[1], spp, 5, depth, ts, 8)
    assert np.any(og[..., 0] != og[..., 2])
    for wavefront in (False, True):
        st = mp.RenderSettings(ts, spp, res, seed=5, max_depth=depth, wavefront=wavefront)
        fr = mp.FrameRenderer(mp.Scene(grp), cam, st)
        fr.render()
        img, u8 = fr.untile()
        got = host(img)
        assert np.array_equal(bits(got), bits(og)), (wavefront, int(np.sum(bits(got) != bits(og))))
        assert np.array_equal(host(u8), ou8) and int(fr.segments.item()) == gseg
        fp = mp.FrameRenderer(mp.Scene(grp), cam, st)
        nxt, segs = 0, 0
        for count in RAGGED:
            nxt = fp.render_pass(nxt, count)
            segs += int(fp.segments.item())
            if nxt < spp:
                check_preview(oracle, fp, nxt)
        img, _ = fp.untile()
        assert np.array_equal(bits(host(img)), bits(og)) and segs == gseg, wavefront


# ---- B. rgb previews over several contexts; D. the staged gather ---------------------------------------------------

@pytest.mark.parametrize("staged", [0, 1])
def test_rgb_previews_over_two_contexts(gpu, oracle, rgb_frame, staged):
    """mp_render_pass_multi over two contexts on one GPU with a coloured table: every gathered preview equals the one-device
    FrameRenderer's preview of the same passes (itself pinned to the definition), the last gather the oracle's frame; with
    multi_gather_staged = 1 rank 1's shard travels through pinned host memory and the frames are the same bits."""
    spp, depth = 40, 4
    ctxs = [mp.Context(0) for _ in range(2)]
    if staged:
        ctxs[0].set_option("multi_gather_staged", staged)
    scenes = [mp.Scene(teapot_rgb(c)) for c in ctxs]
    cam = mp.Camera.teapot_view()
    st = mp.RenderSettings(TS // 2, spp, RES, seed=SEED, max_depth=depth)
    ref = mp.FrameRenderer(scenes[0], cam, st)
    mf = mp.MultiDeviceFrame(scenes, cam, st)
    nxt = 0
    for count in (3, 9, 0):
        assert ref.render_pass(nxt, count) == (nxt + count if count else spp)
        nxt, img, img8 = mf.render_pass(nxt, count)
        got, got8 = host(img), host(img8)
        if nxt < spp:
            exp, exp8 = check_preview(oracle, ref, nxt)
        else:
            of, exp8, _ = rgb_frame(spp, depth)
            exp = of
        assert np.array_equal(bits(got), bits(exp)), (nxt, int(np.sum(bits(got) != bits(exp))))
        assert np.array_equal(got8, exp8), nxt
        assert ctxs[0].query("multi_staged_ranks") == staged


def test_staged_gather_whole_frames_and_chunked_passes(gpu, oracle, teapot_oracle_bvh):
    """multi_gather_staged on the gathering context: whole frames, grey previews of chunked passes and their final frame equal the
    direct path and the oracle; a larger frame after a smaller one (the staging buffer grows) still matches; switching the option
    off again between frames changes nothing; values outside 0..1 are refused."""
    ctxs = [mp.Context(0) for _ in range(4)]
    for v in (-1, 2):
        with pytest.raises(mp.MinipathError):
            ctxs[0].set_option("multi_gather_staged", v)
    scenes = [mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, c)) for c in ctxs]
    cam = mp.Camera.teapot_view()
    osmp = lambda res: oracle.build_sampler(oracle.teapot_camera(), *res)  # noqa: E731
    for res, spp in (((64, 48), 6), ((150, 110), 4)):  # the second frame is larger: every rank's staging buffer grows
        st = mp.RenderSettings(16, spp, res, seed=SEED, max_depth=3)
        of, ou8, _, _ = teapot_oracle_bvh.render_image_paths_mt(osmp(res), res[0], res[1], spp, SEED, 3, 16, 8)
        for staged in (1, 0, 1):
            ctxs[0].set_option("multi_gather_staged", staged)
            img, u8 = mp.MultiDeviceFrame(scenes[:3], cam, st).render()
            assert ctxs[0].query("multi_staged_ranks") == 2 * staged
            assert np.array_equal(bits(host(img)), bits(of)) and np.array_equal(host(u8), ou8), (res, staged)
    # chunked progressive passes, gathered previews through host memory against the direct path's
    res, spp = (80, 48), 300
    oracle.lib().mpo_set_chunked_sum(1)
    try:
        of, ou8, _, _ = teapot_oracle_bvh.render_image_paths_mt(osmp(res), res[0], res[1], spp, SEED, 2, 16, 8)
    finally:
        oracle.lib().mpo_set_chunked_sum(0)
    st = mp.RenderSettings(16, spp, res, seed=SEED, max_depth=2, chunked_sum=True)
    direct = mp.MultiDeviceFrame([scenes[1], scenes[3]], cam, st)  # gathers on ctxs[1], option off
    staged = mp.MultiDeviceFrame([scenes[0], scenes[2]], cam, st)  # gathers on ctxs[0], option on (a rank's shard is its context's)
    ctxs[0].set_option("multi_gather_staged", 1)
    ctxs[1].set_option("multi_gather_staged", 0)
    nd = ns = 0
    for count in (200, 70, 0):  # the first preview falls inside a 256-sample chunk, the second after one
        nd, dimg, du8 = direct.render_pass(nd, count)
        a, a8 = host(dimg), host(du8)
        ns, simg, su8 = staged.render_pass(ns, count)
        assert ctxs[0].query("multi_staged_ranks") == 1 and ctxs[1].query("multi_staged_ranks") == 0
        assert nd == ns
        assert np.array_equal(bits(host(simg)), bits(a)) and np.array_equal(host(su8), a8), ns
    assert np.array_equal(bits(a), bits(of)) and np.array_equal(a8, ou8)


# ---- C. multi-device passes are all or nothing ------------------------------------------------------------------

def _grey_multi(oracle, teapot_oracle_bvh, n, spp, chunked=False):
    ctxs = [mp.Context(0) for _ in range(n)]
    bvhs = [mp.TriangleBvh.with_obj(TEAPOT, c) for c in ctxs]
    res, depth = (64, 48), 3
    st = mp.RenderSettings(16, spp, res, seed=SEED, max_depth=depth, chunked_sum=chunked)
    oracle.lib().mpo_set_chunked_sum(1 if chunked else 0)
    try:
        of, ou8, _, _ = teapot_oracle_bvh.render_image_paths_mt(oracle.build_sampler(oracle.teapot_camera(), *res), res[0], res[1], spp,
                                                                SEED, depth, 16, 8)
    finally:
        oracle.lib().mpo_set_chunked_sum(0)
    return ctxs, bvhs, [mp.Scene(b) for b in bvhs], st, of, ou8


def _finish_and_check(mf, begin, of, ou8):
    nxt, img, u8 = mf.render_pass(begin, 0)
    assert nxt == mf.settings.sample_count
    got = host(img)
    assert np.array_equal(bits(got), bits(of)), int(np.sum(bits(got) != bits(of)))
    assert np.array_equal(host(u8), ou8)


def test_refused_rank_leaves_every_shard_as_it_was(gpu, oracle, teapot_oracle_bvh):
    """Ranks [A, B] render pass (0, 5); [A, C] at 5 is refused (C's shard holds no state) and must not have added the pass to A's
    shard; the continuation on [A, B] then gives the oracle's frame.  The same with a fresh context as the last of three ranks."""
    cam = mp.Camera.teapot_view()
    ctxs, _, scenes, st, of, ou8 = _grey_multi(oracle, teapot_oracle_bvh, 3, 12)
    a, b, c = scenes
    mf = mp.MultiDeviceFrame([a, b], cam, st)
    assert mf.render_pass(0, 5, gather=False) == 5
    with pytest.raises(mp.MinipathError):
        mp.MultiDeviceFrame([a, c], cam, st).render_pass(5, 0)
    _finish_and_check(mf, 5, of, ou8)
    # three ranks, the last one refused
    d = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, mp.Context(0)))
    mf3 = mp.MultiDeviceFrame([a, b, c], cam, st)
    assert mf3.render_pass(0, 4, gather=False) == 4
    with pytest.raises(mp.MinipathError):
        mp.MultiDeviceFrame([a, b, d], cam, st).render_pass(4, 3)
    assert mf3.render_pass(4, 3, gather=False) == 7
    _finish_and_check(mf3, 7, of, ou8)


def test_launch_refusal_on_rank_one_leaves_rank_zero_as_it_was(gpu, oracle, teapot_oracle_bvh):
    """Between chunked passes rank 1's scene gets a coloured table (refused under the chunked rule, which the launcher used to find
    only when it reached rank 1, after rank 0 had rendered); after the grey table is back, the continuation gives the oracle's
    frame."""
    cam = mp.Camera.teapot_view()
    ctxs, bvhs, scenes, st, of, ou8 = _grey_multi(oracle, teapot_oracle_bvh, 2, 40, chunked=True)
    mf = mp.MultiDeviceFrame(scenes, cam, st)
    assert mf.render_pass(0, 10, gather=False) == 10
    sync()
    bvhs[1].set_materials(RGB_TABLE, 1.0)
    with pytest.raises(mp.MinipathError):
        mf.render_pass(10, 0)
    sync()
    bvhs[1].set_materials(GREY_TABLE, 1.0)
    _finish_and_check(mf, 10, of, ou8)
