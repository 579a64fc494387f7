"""GPU parity tests (-m gpu) of the round-3 features, all through the C ABI, bit-exact: progressive passes over several devices
(mp_render_pass_multi, mp_untile_preview), object groups that outlive their members' handles."""
import os

import numpy as np
import pytest

import minipath_amd as mp
from tests import meshes
from tests.dispatch_cases import launched
from tests.conftest import TEAPOT

pytestmark = pytest.mark.gpu
SEED = 0x5EED


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return mp.Context(0)


@pytest.mark.parametrize("n,chunked", [(2, False), (3, True)])
def test_progressive_passes_over_several_devices(oracle, teapot_oracle_bvh, n, chunked):
    """BASELINE configs[4]'s real shape (VERDICT r2 #4b; SURVEY 8e: "accumulators stay sharded; gather only per displayed pass /
    at end"): mp_render_pass_multi adds ragged passes to the shards that stay on their devices; a gather after the last pass is
    the single-launch frame bit for bit (= the oracle's), a gather before it is the preview mp_untile_preview defines -- checked
    against the same formula applied to a one-device FrameRenderer's running state; passes that do not continue the state are
    refused.  The n contexts share this box's GPU."""
    import torch

    ctxs = [mp.Context(0) for _ in range(n)]
    scenes = [mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, c)) for c in ctxs]
    cam = mp.Camera.teapot_view()
    res, spp, ts = (200, 136), 600 if chunked else 24, 16
    depth = 3
    st = mp.RenderSettings(ts, spp, res, seed=SEED, max_depth=depth, chunked_sum=chunked)
    passes = (300, 13, 0) if chunked else (5, 12, 0)   # the chunked case cuts a 256-sample chunk in the middle
    # the expected frame: one launch on one device (itself pinned against the oracle in the round-1/2 suites; and here)
    one = mp.FrameRenderer(scenes[0], cam, st)
    one.render()
    full, _ = one.untile()
    torch.cuda.synchronize()
    full = full.cpu().numpy()
    if not chunked:
        of, _, _, _ = teapot_oracle_bvh.render_image_paths_mt(oracle.build_sampler(oracle.teapot_camera(), *res), res[0], res[1], spp, SEED, depth, ts, 8)
        assert np.array_equal(bits(full), bits(of))
    # the running state after each pass on one device -> expected previews
    ref = mp.FrameRenderer(scenes[0], cam, st)
    mf = mp.MultiDeviceFrame(scenes, cam, st)
    nxt = 0
    for k, count in enumerate(passes):
        nxt_ref = ref.render_pass(nxt, count)
        torch.cuda.synchronize()
        if k == 1:  # a pass that stays on the devices: nothing gathered
            assert mf.render_pass(nxt, count, gather=False) == nxt_ref
            nxt = nxt_ref
            continue
        nxt2, img, img8 = mf.render_pass(nxt, count)
        torch.cuda.synchronize()
        assert nxt2 == nxt_ref
        nxt = nxt2
        got = img.cpu().numpy()
        if nxt == spp:
            assert np.array_equal(bits(got), bits(full))
            ref_img, ref_u8 = ref.untile()
        else:
            ref_img, ref_u8 = ref.untile(preview_samples=nxt)
            state = ref.tile_buf.cpu().numpy()  # [tile, y, x, 4] running state of the one-device render
            torch.cuda.synchronize()
            t0 = ref.tiles[0]
            s = state[0, :t0.height(), :t0.width()]
            if chunked:
                tot = np.ascontiguousarray(s[..., 2:4]).view(np.float64)[..., 0] + s[..., 0].astype(np.float64)
                exp = (tot * (1.0 / np.float64(nxt))).astype(np.float32)
                exp_a = (s[..., 1].astype(np.float64) * (1.0 / np.float64(nxt))).astype(np.float32)
            else:
                inv = np.float32(1.0) / np.float32(nxt)
                exp, exp_a = s[..., 0] * inv, s[..., 3] * inv
            blk = got[t0.min_y:t0.max_y, t0.min_x:t0.max_x]
            assert np.array_equal(bits(blk[..., 0]), bits(exp)) and np.array_equal(bits(blk[..., 3]), bits(exp_a))
            assert np.array_equal(bits(blk[..., 1]), bits(exp)) and np.array_equal(bits(blk[..., 2]), bits(exp))
        torch.cuda.synchronize()
        assert np.array_equal(bits(got), bits(ref_img.cpu().numpy())) and np.array_equal(img8.cpu().numpy(), ref_u8.cpu().numpy())
    assert nxt == spp
    # a pass that does not continue the shards' state is refused; a pass from 0 starts over
    with pytest.raises(mp.MinipathError):
        mf.render_pass(7, 3)
    assert mf.render_pass(0, 4, gather=False) == 4
    with pytest.raises(mp.MinipathError):
        mf.render_pass(5, 3)
    with pytest.raises(mp.MinipathError):
        mp.MultiDeviceFrame(list(reversed(scenes)), cam, st).render_pass(4, 3)   # other ranks: not the state those shards hold
    assert mf.render_pass(4, 0)[0] == spp
    torch.cuda.synchronize()
    assert np.array_equal(bits(mf.image.cpu().numpy()), bits(full))
    # whole frames through the same buffers afterwards
    img, _ = mf.render()
    torch.cuda.synchronize()
    assert np.array_equal(bits(img.cpu().numpy()), bits(full))


def test_group_outlives_its_members_handles(ctx):
    """an object group borrows its members' device arrays; it now holds a reference on each member, so closing the
    members first must leave the group renderable (before: kernels read freed device memory)."""
    import torch

    base = mp.TriangleBvh.with_obj(TEAPOT, ctx)
    tr = np.array([[0, 0, 0], [7.5, 0, -3]], np.float32)
    inst = mp.Instances(base, tr)
    cam = mp.Camera.teapot_view()
    st = mp.RenderSettings(32, 4, (160, 96), seed=SEED)
    fr = mp.FrameRenderer(mp.Scene(inst), cam, st)
    fr.render()
    before, _ = fr.untile()
    torch.cuda.synchronize()
    before = before.cpu().numpy()
    base.close()                       # the caller's handle on the member goes first
    junk = [torch.full((1 << 20,), float("nan"), device="cuda") for _ in range(16)]  # churn the allocator over whatever was freed
    del junk
    fr2 = mp.FrameRenderer(mp.Scene(inst), cam, st)
    fr2.render()
    after, _ = fr2.untile()
    torch.cuda.synchronize()
    assert np.array_equal(bits(after.cpu().numpy()), bits(before))
    assert inst.info().triangle_count == 2256  # info() reads the member's host tree: still there
    inst.close()


def test_coloured_and_checker_materials(ctx, oracle):
    """SURVEY 8 f4 finished: rgb albedo / emission and a checkerboard material that reads
    HitRecord.texture_coords (geometry/mod.rs:78-79).  Oracle definition: tests/test_golden_cpu.py; here GPU == oracle bit for bit
    for the fused kernel, the staged pipeline, an object group with a Sphere member (texture coordinates = origin), progressive
    passes; the chunked rule refuses such tables."""
    import ctypes as C

    import torch

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
    res, spp, depth, ts = (160, 112), 9, 5, 32
    smp = oracle.build_sampler(oc, *res)
    for sky in (0.6, 0.0):
        bvh.set_materials(table, sky)
        orc.set_materials(table, sky)
        of, ou8, _, seg = orc.render_image_paths_mt(smp, res[0], res[1], spp, 21, depth, ts, 8)
        assert not np.array_equal(of[..., 0], of[..., 2])  # really coloured
        for wavefront in (False, True):
            fr = mp.FrameRenderer(mp.Scene(bvh), cam, mp.RenderSettings(ts, spp, res, seed=21, max_depth=depth, wavefront=wavefront))
            fr.render()
            img, u8 = fr.untile()
            torch.cuda.synchronize()
            assert np.array_equal(bits(img.cpu().numpy()), bits(of)), (sky, wavefront, int(np.sum(bits(img.cpu().numpy()) != bits(of))))
            assert np.array_equal(u8.cpu().numpy(), ou8) and int(fr.segments.item()) == seg
            # ragged progressive passes carry {sum r, sum g, sum b, hits}
            fp = mp.FrameRenderer(mp.Scene(bvh), cam, mp.RenderSettings(ts, spp, res, seed=21, max_depth=depth, wavefront=wavefront))
            nxt = fp.render_pass(0, 4); nxt = fp.render_pass(nxt, 1); fp.render_pass(nxt)
            img2, _ = fp.untile()
            torch.cuda.synchronize()
            assert np.array_equal(bits(img2.cpu().numpy()), bits(of))
    with pytest.raises(mp.MinipathError):   # one channel of state per pixel under the chunked rule
        mp.FrameRenderer(mp.Scene(bvh), cam, mp.RenderSettings(ts, 300, res, seed=21, max_depth=depth, chunked_sum=True)).render()
    # the reference semantics ignore the table altogether
    of1, _, _, _, _ = orc.render_image_mt(smp, res[0], res[1], 4, 21, ts, 8)
    fr = mp.FrameRenderer(mp.Scene(bvh), cam, mp.RenderSettings(ts, 4, res, seed=21))
    fr.render()
    img, _ = fr.untile()
    torch.cuda.synchronize()
    assert np.array_equal(bits(img.cpu().numpy()), bits(of1))
    # object group: the grid twice (one turned) and a Sphere; the group's table
    ball_def = ((0.3, 1.4, 0.2), 0.8)
    tr = np.array([[0, 0, 0], [0.5, 2.5, -0.5], [0, 0, 0]], np.float32)
    rot = np.array([[0, 0, 0, 1], [np.sqrt(0.5), 0, 0, np.sqrt(0.5)], [0, 0, 0, 1]], np.float32)
    grp = mp.ObjectGroup([bvh, bvh, mp.Sphere(*ball_def, ctx)], tr, rotations=rot)
    grp.set_materials(table, 0.5)
    orc.set_materials(table, 0.5)
    orc.set_group([orc, orc, ball_def], tr, rotations=rot)
    og, _, _, gseg = orc.render_image_paths_mt(smp, res[0], res[1], spp, 5, depth, ts, 8)
    orc.set_instances(np.zeros((0, 3), np.float32))
    fr = mp.FrameRenderer(mp.Scene(grp), cam, mp.RenderSettings(ts, spp, res, seed=5, max_depth=depth))
    fr.render()
    img, _ = fr.untile()
    torch.cuda.synchronize()
    assert np.array_equal(bits(img.cpu().numpy()), bits(og)) and int(fr.segments.item()) == gseg
    # a grey table on the same scene still takes the one-channel kernels and gives r = g = b
    bvh.set_materials([(0.5, 0.0), (0.8, 0.1), (0.3, 0.0)], 1.0)
    orc.set_materials([(0.5, 0.0), (0.8, 0.1), (0.3, 0.0)], 1.0)
    ogr, _, _, _ = orc.render_image_paths_mt(smp, res[0], res[1], spp, 21, depth, ts, 8)
    fr = mp.FrameRenderer(mp.Scene(bvh), cam, mp.RenderSettings(ts, spp, res, seed=21, max_depth=depth))
    fr.render()
    img, _ = fr.untile()
    torch.cuda.synchronize()
    got = img.cpu().numpy()
    assert np.array_equal(bits(got), bits(ogr)) and np.array_equal(got[..., 0], got[..., 1])


@pytest.mark.parametrize("mode", [0, 2, 3])
def test_pooled_path_kernel_modes(oracle, teapot_oracle_bvh, mode):
    """Round 3: the pooled form of the fused path kernel (several passes of 8 samples share one 8-lane-group walk over a per-wave ray
    queue in global memory, the passes' path state parked beside it) against the one-pass kernel (mode 0): same operations per path,
    same sample order -- the same bits and segment counts as the oracle, on an open scene (most paths end early: thin queues), an
    interior scene (every path survives to max_depth), ragged progressive passes that start and end inside a batch, and the chunked
    accumulation rule (a 256-sample chunk boundary never falls inside a batch)."""
    import ctypes as C

    import torch

    from minipath_amd import scenes

    c = mp.Context(0)
    c.set_option("paths_pooled", mode)
    teapot = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, c))
    cam = mp.Camera.teapot_view()
    for spp, depth, res, tile in ((40, 5, (256, 256), (64, 96, 128, 160)), (17, 3, (250, 130), (192, 64, 250, 128)), (70, 2, (256, 256), (96, 96, 128, 128))):
        st = mp.RenderSettings(64, spp, res, seed=SEED, max_depth=depth)
        fr = mp.FrameRenderer(teapot, cam, st, tiles=[mp.ScreenBlock(*tile)])
        buf = fr.render()
        # the kernel the mode selects: pooled with two passes (mode 2) or four from 32 samples on (mode 3); mode 0 the one-pass kernel,
        # its camera pass on the cached packet walk from 32 samples on
        want = {0: "render_paths_kernel<8, false, false, true>" if spp >= 32 else "render_paths_kernel<8, false, false>",
                2: "render_paths_pooled_kernel<2>", 3: "render_paths_pooled_kernel<4>" if spp >= 32 else "render_paths_pooled_kernel<2>"}[mode]
        assert launched(c) == [want]
        torch.cuda.synchronize()
        tw, th = tile[2] - tile[0], tile[3] - tile[1]
        of, _, seg = teapot_oracle_bvh.render_tile_paths(oracle.build_sampler(oracle.teapot_camera(), *res), res[0], res[1], spp, SEED, depth, *tile)
        assert np.array_equal(bits(buf[0, :th, :tw].cpu().numpy()), bits(of)), (mode, spp, depth)
        assert int(fr.segments.item()) == seg
        # ragged progressive passes: 13 + 9 + the rest start and end inside batches of 16 / 32 samples
        fp = mp.FrameRenderer(teapot, cam, st, tiles=[mp.ScreenBlock(*tile)])
        nxt, segs = 0, 0
        for count in (13, 9, 0) if spp > 22 else (5, 0):
            nxt = fp.render_pass(nxt, count)
            segs += int(fp.segments.item())
        torch.cuda.synchronize()
        assert np.array_equal(bits(fp.tile_buf[0, :th, :tw].cpu().numpy()), bits(of)) and segs == seg
    # interior scene, whole frame, also under the chunked rule
    pos, nrm, tex, tri = scenes.atrium(1, 0.05)
    scene = mp.Scene(mp.TriangleBvh.build(pos, nrm, tex, tri, c))
    orc = oracle.Bvh.build(pos, nrm, tex, tri)
    oc = oracle.Camera()
    oracle.lib().mpo_camera_default(C.byref(oc))
    eye, at, fnum = scenes.ATRIUM_VIEW
    oracle.lib().mpo_camera_look_at(C.byref(oc), oracle.vec3(*eye), oracle.vec3(*at), oracle.vec3(0, 1, 0))
    oc.f_number = fnum
    res = (96, 64)
    smp = oracle.build_sampler(oc, *res)
    for spp, depth, chunked in ((32, 6, False), (300, 3, True)):
        oracle.lib().mpo_set_chunked_sum(1 if chunked else 0)
        try:
            of, _, _, seg = orc.render_image_paths_mt(smp, res[0], res[1], spp, 11, depth, 32, 8)
        finally:
            oracle.lib().mpo_set_chunked_sum(0)
        fr = mp.FrameRenderer(scene, scenes.atrium_camera(), mp.RenderSettings(32, spp, res, seed=11, max_depth=depth, chunked_sum=chunked))
        if chunked:
            nxt = fr.render_pass(0, 100); nxt = fr.render_pass(nxt, 157); fr.render_pass(nxt)
        else:
            fr.render()
        img, _ = fr.untile()
        torch.cuda.synchronize()
        assert np.array_equal(bits(img.cpu().numpy()), bits(of)), (mode, spp, chunked, int(np.sum(bits(img.cpu().numpy()) != bits(of))))
        if not chunked:
            assert int(fr.segments.item()) == seg


@pytest.mark.parametrize("mode", [0, 2])
def test_packet_mask_cache(oracle, teapot_oracle_bvh, mode):
    """Round 3: the packet walk's per-unit mask cache (children that NO ray inside the bounds of the work unit's rays can hit are
    skipped without their per-ray slab tests; bounds widened and masks rebuilt when a pass does not fit).  Exact by interval
    arithmetic on monotone IEEE operations; here: frames with units of 4 to 16 passes, 16 and 32 samples in flight, a pinhole and a
    wide lens (bounds of very different extent), a view along an axis (zero direction components: those passes take the literal
    walk, the others the cache), ragged progressive passes, equal to the oracle bit for bit with the cache forced on and off."""
    import ctypes as C

    import torch

    from minipath_amd import scenes

    c = mp.Context(0)
    c.set_option("packet_mask_cache", mode)
    teapot = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, c))
    res = (96, 64)
    for fnum, spp, sflight in ((4.8, 64, 16), (1e9, 128, 32), (0.7, 70, 16)):
        c.set_option("packet_samples_in_flight", sflight)
        cam = mp.Camera.teapot_view().f_number(fnum)
        oc = oracle.teapot_camera()
        oc.f_number = fnum
        of, ou8, _, seg, _ = teapot_oracle_bvh.render_image_mt(oracle.build_sampler(oc, *res), res[0], res[1], spp, SEED, 32, 8)
        fr = mp.FrameRenderer(teapot, cam, mp.RenderSettings(32, spp, res, seed=SEED))
        fr.render()
        # every one of these frames has units of four passes or more: the cached form with the cache on, the plain one with it off
        assert launched(c) == [f"render_tiles_packet_kernel<{sflight}, false, " + ("8, false, true>" if mode else "7>")]
        img, u8 = fr.untile()
        torch.cuda.synchronize()
        assert np.array_equal(bits(img.cpu().numpy()), bits(of)), (mode, fnum, spp)
        assert np.array_equal(u8.cpu().numpy(), ou8)
    c.set_option("packet_samples_in_flight", 0)
    # interior scene with absorbed nodes in its wide tree; an axis-aligned view through the middle pixel columns; ragged passes
    pos, nrm, tex, tri = scenes.atrium(1, 0.05)
    scene = mp.Scene(mp.TriangleBvh.build(pos, nrm, tex, tri, c))
    orc = oracle.Bvh.build(pos, nrm, tex, tri)
    for eye, at in (((-16.0, 4.2, 0.8), (12.0, 5.5, -0.5)), ((-15.0, 5.0, 0.0), (10.0, 5.0, 0.0))):
        oc = oracle.Camera()
        oracle.lib().mpo_camera_default(C.byref(oc))
        oracle.lib().mpo_camera_look_at(C.byref(oc), oracle.vec3(*eye), oracle.vec3(*at), oracle.vec3(0, 1, 0))
        oc.f_number = 1e9  # pinhole: every ray of the centre column has an exactly zero direction component in the second view
        cam = mp.Camera.default().look_at(eye, at, (0, 1, 0)).f_number(1e9)
        spp = 96
        of, _, _, _, _ = orc.render_image_mt(oracle.build_sampler(oc, *res), res[0], res[1], spp, 3, 32, 8)
        fr = mp.FrameRenderer(scene, cam, mp.RenderSettings(32, spp, res, seed=3))
        # automatic samples in flight: the cache's table gives the pass of 70 samples 16 and the one of 26 four; without the cache
        # these small launches get 32 from 32 samples on, else 16
        nxt = fr.render_pass(0, 70)
        assert launched(c) == ["render_tiles_packet_kernel<16, false, 8, false, true>" if mode else "render_tiles_packet_kernel<32, false, 7>"]
        fr.render_pass(nxt)
        assert launched(c) == ["render_tiles_packet_kernel<4, false, 8, false, true>" if mode else "render_tiles_packet_kernel<16, false, 7>"]
        img, _ = fr.untile()
        torch.cuda.synchronize()
        assert np.array_equal(bits(img.cpu().numpy()), bits(of)), (mode, eye)


def test_packet_triangle_masks(oracle):
    """Round 3: the packet walk's per-unit TRIANGLE masks (tri_may_hit: the Moeller-Trumbore sequence evaluated on intervals over
    the bounds of a work unit's rays; a triangle no ray inside the bounds can hit is skipped for every pass of the unit).  Frames
    of the interior stand-in with 8 and 16 passes per unit through a wide lens and a pinhole, and the magnitude guards of the
    no-overflow argument: a scene scaled beyond 2^30 (DevScene::tris_bounded off: plain walk), a scene within the bound seen from
    beyond 2^30 (those passes take the plain walk) -- all equal to the oracle bit for bit with the cache on and off."""
    import ctypes as C

    import torch

    from minipath_amd import scenes

    res = (96, 64)
    pos, nrm, tex, tri = scenes.atrium(1, 0.08)
    cases = [(1.0, (-14.0, 4.5, 1.0), (10.0, 5.0, -2.0), 1.4, 256), (1.0, (-14.0, 4.5, 1.0), (10.0, 5.0, -2.0), 1e9, 128),
             (2.0 ** 31, (-14.0, 4.5, 1.0), (10.0, 5.0, -2.0), 4.0, 64), (2.0 ** 24, (-120.0, 30.0, 9.0), (10.0, 5.0, -2.0), 4.0, 64)]
    for scale, eye, at, fnum, spp in cases:
        p = (pos * np.float32(scale)).astype(np.float32)
        orc = oracle.Bvh.build(p, nrm, tex, tri)
        oc = oracle.Camera()
        oracle.lib().mpo_camera_default(C.byref(oc))
        e = tuple(float(np.float32(x) * np.float32(scale)) for x in eye)
        a = tuple(float(np.float32(x) * np.float32(scale)) for x in at)
        oracle.lib().mpo_camera_look_at(C.byref(oc), oracle.vec3(*e), oracle.vec3(*a), oracle.vec3(0, 1, 0))
        oc.f_number = fnum
        of, _, _, _, _ = orc.render_image_mt(oracle.build_sampler(oc, *res), res[0], res[1], spp, 21, 32, 8)
        assert np.count_nonzero(of[..., 3]) > 200  # the view does hit the scene
        for mode in (1, 0):
            c = mp.Context(0)
            c.set_option("packet_mask_cache", mode)
            scene = mp.Scene(mp.TriangleBvh.build(p, nrm, tex, tri, c))
            cam = mp.Camera.default().look_at(e, a, (0, 1, 0)).f_number(fnum)
            fr = mp.FrameRenderer(scene, cam, mp.RenderSettings(32, spp, res, seed=21))
            fr.render()
            img, _ = fr.untile()
            torch.cuda.synchronize()
            assert np.array_equal(bits(img.cpu().numpy()), bits(of)), (scale, fnum, mode, int(np.sum(bits(img.cpu().numpy()) != bits(of))))


def test_cpp_mirror_renders_the_same_frame():
    """examples/render_teapot (C++ over include/minipath.hpp: Camera().look_at(..).f_number(..), Scene::with_obj, render(), wait(),
    image()) renders the frame the Python mirror renders through the same C ABI: FNV-1a of the u8 image."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(root, "examples")], check=True, capture_output=True)
    r = subprocess.run([os.path.join(root, "examples", "render_teapot"), TEAPOT, "320", "200", "16", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    line = [l for l in r.stdout.splitlines() if l.startswith("image fnv1a ")]
    assert line, r.stdout
    c = mp.Context(0)
    scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, c))
    prog = mp.render(scene, mp.Camera.teapot_view(), mp.RenderSettings(64, 16, (320, 200), seed=SEED))
    prog.wait()
    u8 = prog.image()
    h = 1469598103934665603
    for b in np.ascontiguousarray(u8).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert line[0].split()[-1] == f"{h:016x}"
    assert "20 / 20 tiles" in r.stdout


def test_render_u8_only_flag():
    """MP_FLAG_IMAGE_U8_ONLY: render() keeps just the reference's u8 RgbaImage on the host -- the same bytes as without the flag --
    and mp_render_image_f32 then says MP_ERR_UNSUPPORTED."""
    c = mp.Context(0)
    scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, c))
    res = (200, 120)
    full = mp.render(scene, mp.Camera.teapot_view(), mp.RenderSettings(32, 24, res, seed=SEED))
    full.wait()
    c.set_option("render_batch_tiles", 5)  # ... and odd batches that taper towards the end of the frame: the same image
    lean = mp.render(scene, mp.Camera.teapot_view(), mp.RenderSettings(32, 24, res, seed=SEED, image_u8_only=True))
    lean.wait()
    c.set_option("render_batch_tiles", 0)
    assert lean.progress().finished == lean.progress().total == 28
    assert np.array_equal(full.image(), lean.image()) and full.image().any()
    assert full.image_f32().shape == (res[1], res[0], 4)
    with pytest.raises(mp.MinipathError) as e:
        lean.image_f32()
    assert e.value.code == 5
