"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI, against the CPU oracle
on identical seeded inputs.  All comparisons are BIT-EXACT on f32 bit patterns (the north-star tolerance is 1e-5
relative on the accumulated radiance; the implementation is written to meet it with zero difference) and exact on
u8 / indices."""
import os
import threading

import numpy as np
import pytest

import minipath_amd as mp
from tests import meshes
from tests.dispatch_cases import launched
from tests.conftest import TEAPOT

pytestmark = pytest.mark.gpu

SEED = 0x5EED
REL_TOL = 1e-5  # BASELINE.json north_star: accumulated f32 radiance within 1e-5 relative


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return mp.Context(0)


@pytest.fixture(scope="module")
def teapot(ctx):
    return mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, ctx))


def _trace_both(scene, orc, o, d, full=False):
    import torch

    to = torch.from_numpy(o).cuda()
    td = torch.from_numpy(d).cuda()
    out = scene.object.intersect(to, td, full=full)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    t, prim, u, v = orc.trace(o, d)
    return got, (t, prim, u, v)


def _assert_hits_equal(got, exp):
    t, prim, u, v = exp
    assert np.array_equal(got["prim"].view(np.uint32), prim), f"{int(np.sum(got['prim'].view(np.uint32) != prim))} prim mismatches"
    assert np.array_equal(bits(got["t"]), bits(t))
    hit = prim != 0xFFFFFFFF
    assert np.array_equal(bits(got["u"])[hit], bits(u)[hit])
    assert np.array_equal(bits(got["v"])[hit], bits(v)[hit])


def test_trace_teapot_camera_rays_bit_exact(teapot, oracle, teapot_oracle_bvh):
    """bit-identical (t, prim, u, v) on seeded teapot rays (K2+K3)."""
    s = oracle.build_sampler(oracle.teapot_camera(), 256, 256)
    rng = np.random.default_rng(1)
    n = 60000
    o = np.zeros((n, 3), np.float32)
    d = np.zeros((n, 3), np.float32)
    xs, ys = rng.integers(0, 256, n), rng.integers(0, 256, n)
    for i in range(n):
        r = oracle.sample_ray(s, int(xs[i]), int(ys[i]), 1000 + i)
        o[i] = list(r.o)
        d[i] = list(r.d)
    got, exp = _trace_both(teapot, teapot_oracle_bvh, o, d)
    _assert_hits_equal(got, exp)
    assert 0.2 < np.mean(exp[1] != 0xFFFFFFFF) < 0.9


def test_trace_random_rays_full_hit_record(teapot, oracle, teapot_oracle_bvh):
    """Random origins incl. inside the model, axis-parallel and zero-component directions (inv = +inf path);
    full HitRecord (point, normal, texture_coords) of ray_bvh_intersection.rs:66-95."""
    bmin, bmax = teapot_oracle_bvh.bbox()
    o, d = meshes.random_rays(20000, 7, bmin, bmax)
    got, exp = _trace_both(teapot, teapot_oracle_bvh, o, d, full=True)
    _assert_hits_equal(got, exp)
    idx = np.nonzero(exp[1] != 0xFFFFFFFF)[0][:3000]
    for i in idx:
        h = teapot_oracle_bvh.intersect(oracle.ray_new(o[i], d[i]))
        assert h.hit == 1
        assert np.array_equal(bits(got["point"][i]), bits(np.array(list(h.point), np.float32)))
        assert np.array_equal(bits(got["normal"][i]), bits(np.array(list(h.normal), np.float32)))
        assert np.array_equal(bits(got["tex"][i]), bits(np.array(list(h.tex), np.float32)))


@pytest.mark.parametrize("name", ["soup_300", "soup_5000", "grid_40", "sphere_24", "flat_plane", "two_clusters", "sliver_fan"])
def test_trace_synthetic_scenes(ctx, oracle, name):
    """Flat-shaded soups, smooth grids, degenerate (zero-extent) boxes, far-apart clusters, shared-edge ties."""
    import torch

    pos, nrm, tex, tri = meshes.make(name)
    scene = mp.Scene(mp.TriangleBvh.build(pos, nrm, tex, tri, ctx))
    orc = oracle.Bvh.build(pos, nrm, tex, tri)
    bmin, bmax = orc.bbox()
    o, d = meshes.random_rays(30000, 21, bmin, np.maximum(bmax, bmin + 1e-3))
    got, exp = _trace_both(scene, orc, o, d, full=True)
    _assert_hits_equal(got, exp)
    idx = np.nonzero(exp[1] != 0xFFFFFFFF)[0][:500]
    for i in idx:
        h = orc.intersect(oracle.ray_new(o[i], d[i]))
        assert np.array_equal(bits(got["normal"][i]), bits(np.array(list(h.normal), np.float32)))
    if name not in ("flat_plane",):
        assert len(idx) > 10
    del scene
    torch.cuda.synchronize()


def test_trace_non_finite_and_extreme_rays(teapot, oracle, teapot_oracle_bvh):
    """Rays no renderer produces but a caller of mp_trace_rays can hand over: zero-length directions (Ray::new divides 0 by 0:
    NaN direction, NaN inverse), NaN / infinite origins and directions, directions of 1e-30 and 1e30 length, origins 1e30 away,
    origins exactly on the scene box, denormal components.  The walk has no special cases for them: every comparison against a NaN
    is false on the GPU as on the CPU, so (t, prim, u, v) still match the oracle bit for bit (and nothing hangs or faults)."""
    rng = np.random.default_rng(99)
    bmin, bmax = [np.asarray(x, np.float32) for x in teapot_oracle_bvh.bbox()]
    o, d = meshes.random_rays(4096, 5, bmin, bmax)
    n = o.shape[0]
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    k = 0
    def block(m):
        nonlocal k
        sl = slice(k, k + m); k += m
        return sl
    d[block(64)] = 0.0                                   # zero-length direction
    d[block(64), rng.integers(0, 3, 64)] = nan           # one NaN component
    o[block(64), rng.integers(0, 3, 64)] = nan
    d[block(64), rng.integers(0, 3, 64)] = inf           # infinite direction component: the unit vector has a NaN and zeros
    o[block(64), rng.integers(0, 3, 64)] = -inf
    sl = block(128); d[sl] = d[sl] * np.float32(1e-30)   # tiny but normal length
    sl = block(128); d[sl] = d[sl] * np.float32(1e-41)   # denormal components (length underflows towards 0)
    sl = block(128); d[sl] = d[sl] * np.float32(1e30)    # the squared length overflows: norm = inf, direction 0 or NaN
    sl = block(128); o[sl] = o[sl] + np.float32(1e30)    # origin far away
    sl = block(128); o[sl, 0] = bmin[0]                  # origin exactly on the box's faces
    sl = block(128); o[sl, 1] = bmax[1]; d[sl, 1] = 0.0  # ... sliding along one
    sl = block(64); o[sl] = np.float32(1e-42)            # denormal origin
    # a direction component small enough that 1/d overflows to +-inf (denormals are kept) with the origin exactly on a
    # child-box plane of the same axis gives 0 * inf = NaN in the slab test, which aabb.rs:262-267 patches to -inf / +inf: these
    # rays must take the walk with the NaN patches (and the literal tree), chosen from the inverse, not from `d == 0`
    lit = teapot.object.device_tree(literal=True)[0]
    boxes = lit[:, :, :6].view(np.float32).reshape(-1, 6)[lit[:, :, 6].reshape(-1) != 0xFFFFFFF8]
    sl = block(256)
    for j, i in enumerate(range(sl.start, sl.stop)):
        b = boxes[rng.integers(0, boxes.shape[0])]
        ax = j % 3
        tgt = b[:3] + (b[3:] - b[:3]) * rng.random(3, dtype=np.float32)
        dd = rng.standard_normal(3).astype(np.float32)
        dd[ax] = np.float32(1e-40) * (1 if (j // 3) % 2 else -1)   # |1/d| = inf after Ray::new's normalisation
        oo = (tgt - dd * np.float32(2.0)).astype(np.float32)
        oo[ax] = b[ax] if (j // 6) % 2 else b[3 + ax]              # exactly on the child box's min / max plane
        o[i], d[i] = oo, dd
    assert k <= n
    got, exp = _trace_both(teapot, teapot_oracle_bvh, o, d, full=True)
    _assert_hits_equal(got, exp)
    hit = exp[1] != 0xFFFFFFFF
    assert 200 < hit.sum() < n  # the ordinary rays among them still hit
    # misses report t = f32::MAX and zeroed records
    assert np.all(got["t"][~hit] == np.finfo(np.float32).max) and not got["normal"][~hit].any() and not got["point"][~hit].any()
    for i in np.flatnonzero(hit)[:300]:
        h = teapot_oracle_bvh.intersect(oracle.ray_new(o[i], d[i]))
        assert np.array_equal(bits(got["point"][i]), bits(np.array(list(h.point), np.float32)))
        assert np.array_equal(bits(got["normal"][i]), bits(np.array(list(h.normal), np.float32)))


def test_trace_edge_sizes(teapot, teapot_oracle_bvh):
    """n = 0, 1, 63, 64, 65 rays (partial wave queues)."""
    import torch

    bmin, bmax = teapot_oracle_bvh.bbox()
    for n in (1, 63, 64, 65, 129):
        o, d = meshes.random_rays(n, 100 + n, bmin, bmax)
        got, exp = _trace_both(teapot, teapot_oracle_bvh, o, d)
        _assert_hits_equal(got, exp)
    out = teapot.object.intersect(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), device="cuda"))
    assert out["t"].numel() == 0


def test_generate_rays_matches_sample_ray(ctx, oracle):
    """K1: CameraSampler::sample_ray (camera.rs:176-191) in seeded mode, bit-exact."""
    import ctypes as C

    import torch

    from minipath_amd import _lib

    cam = mp.Camera.teapot_view()
    st = mp.RenderSettings(64, 16, (256, 256), seed=SEED)
    smp = cam.build_sampler(st.resolution)
    blk = mp.ScreenBlock(40, 50, 72, 70)
    n = blk.area()
    bufs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(6)]
    s, ss = smp.as_struct(), st.as_struct()
    for sample in (0, 5, 15):
        _lib.check(
            _lib.lib().mp_generate_rays(ctx.handle, C.byref(s), C.byref(ss), blk.as_struct(), sample, *[b.data_ptr() for b in bufs], None)
        )
        torch.cuda.synchronize()
        g = [b.cpu().numpy() for b in bufs]
        osmp = oracle.sampler_from_array(smp.as_array())
        for i, (x, y) in enumerate(blk.internal_points()):
            key = oracle.lib().mpo_sample_key(SEED, 256, 16, x, y, sample)
            r = oracle.sample_ray(osmp, x, y, key)
            exp = np.array(list(r.o) + list(r.d), np.float32)
            assert np.array_equal(bits(np.array([g[k][i] for k in range(6)], np.float32)), bits(exp)), (x, y, sample)


@pytest.mark.parametrize("traversal", ["packets", "groups"])
@pytest.mark.parametrize(
    "res,tile_size,spp,tile",
    [
        ((256, 256), 64, 16, (64, 64, 128, 128)),     # SURVEY 8c golden: one 64x64 tile at 16 spp
        ((256, 256), 64, 1, (128, 128, 192, 192)),    # spp = 1
        ((250, 130), 64, 5, (192, 128, 250, 130)),    # clipped corner tile 58 x 2
        ((256, 256), 20, 7, (100, 100, 120, 120)),    # tile size not a multiple of the 8x8 wave block
        ((256, 256), 64, 3, (0, 0, 64, 64)),          # background-only tile
    ],
)
def test_render_tile_bit_exact(teapot, oracle, teapot_oracle_bvh, res, tile_size, spp, tile, traversal):
    """Worker::render_tile (worker.rs:32-49): f32 means bit-exact (<= 1e-5 rel required), u8 exact; both the
    ray-packet and the 8-lane-group traversal."""
    cam = mp.Camera.teapot_view()
    st = mp.RenderSettings(tile_size, spp, res, seed=SEED, traversal=traversal)
    f, u8 = mp.render_tile(teapot, cam.build_sampler(res), st, mp.ScreenBlock(*tile))
    of, ou8 = teapot_oracle_bvh.render_tile(oracle.build_sampler(oracle.teapot_camera(), *res), res[0], res[1], spp, SEED, *tile)
    rel = np.abs(f - of) / np.maximum(np.abs(of), 1e-30)
    assert rel.max() <= REL_TOL
    assert np.array_equal(bits(f), bits(of)), f"{int(np.sum(bits(f) != bits(of)))} f32 values differ (max rel {rel.max()})"
    assert np.array_equal(u8, ou8)


def test_render_tile_empty_and_invalid(teapot):
    cam = mp.Camera.teapot_view()
    st = mp.RenderSettings(64, 2, (256, 256))
    f, u8 = mp.render_tile(teapot, cam.build_sampler((256, 256)), st, mp.ScreenBlock(10, 10, 10, 30))
    assert f.size == 0 and u8.size == 0
    with pytest.raises(mp.MinipathError):  # tile larger than tile_size
        mp.render_tile(teapot, cam.build_sampler((256, 256)), st, mp.ScreenBlock(0, 0, 65, 64))
    with pytest.raises(mp.MinipathError):  # tile outside the resolution
        mp.render_tile(teapot, cam.build_sampler((256, 256)), st, mp.ScreenBlock(224, 224, 288, 288))


@pytest.mark.parametrize("traversal", ["packets", "groups"])
def test_c1_frame_matches_oracle(teapot, oracle, teapot_oracle_bvh, traversal):
    """BASELINE config C1 (teapot 256x256, 16 spp): the whole frame through the one-launch device path + untile,
    against the oracle's threaded render (machinery.rs semantics): f32 bit-exact, u8 exact."""
    import torch

    cam = mp.Camera.teapot_view()
    st = mp.RenderSettings(64, 16, (256, 256), seed=SEED, traversal=traversal)
    fr = mp.FrameRenderer(teapot, cam, st)
    fr.render()
    img, img8 = fr.untile()
    torch.cuda.synchronize()
    of, ou8, _, rays, _ = teapot_oracle_bvh.render_image_mt(oracle.build_sampler(oracle.teapot_camera(), 256, 256), 256, 256, 16, SEED, 64, 8)
    assert rays == 256 * 256 * 16 == fr.rays_per_frame
    assert np.array_equal(bits(img.cpu().numpy()), bits(of))
    assert np.array_equal(img8.cpu().numpy(), ou8)
    cover = (of[..., 3] > 0).mean()
    assert 0.3 < cover < 0.7


def test_render_async_api(teapot, oracle, teapot_oracle_bvh):
    """render()/RenderProgress (machinery.rs:20-178): callbacks once per tile start/end, progress, image, elapsed."""
    cam = mp.Camera.teapot_view()
    st = mp.RenderSettings(32, 4, (160, 96), seed=SEED)
    started, finished, lock = [], [], threading.Lock()

    def on_start(t):
        with lock:
            started.append(t)

    def on_finish(t, snap):
        with lock:
            finished.append((t, snap.finished, snap.total))

    rp = mp.render(teapot, cam, st, on_start, on_finish)
    rp.wait()
    assert rp.is_finished()
    tiles = mp.tile_ordering(mp.ScreenBlock(0, 0, 160, 96), 32)
    assert len(tiles) == 15
    assert sorted(t.as_struct().as_tuple() for t in started) == sorted(t.as_struct().as_tuple() for t in tiles)
    assert sorted(t.as_struct().as_tuple() for t, _, _ in finished) == sorted(t.as_struct().as_tuple() for t in tiles)
    assert sorted(f for _, f, _ in finished) == list(range(1, 16)) and all(tot == 15 for _, _, tot in finished)
    p = rp.progress()
    assert (p.finished, p.total) == (15, 15) and p.percent() == 100.0
    e1 = rp.elapsed()
    assert e1 > 0 and rp.elapsed() == e1  # stops incrementing once finished (machinery.rs:148-157)
    of, ou8, *_ = teapot_oracle_bvh.render_image_mt(oracle.build_sampler(oracle.teapot_camera(), 160, 96), 160, 96, 4, SEED, 32, 4)
    assert np.array_equal(rp.image(), ou8)
    assert np.array_equal(bits(rp.image_f32()), bits(of))
    # shuffled tile order renders the same image
    rp2 = mp.render(teapot, cam, mp.RenderSettings(32, 4, (160, 96), seed=SEED, shuffle_tiles=True))
    rp2.wait()
    assert np.array_equal(rp2.image(), ou8)


def test_render_abort(teapot):
    """RenderProgress::abort (machinery.rs:159-165): in-flight tiles finish, no new ones start.  abort() is called
    from the first `started` callback, i.e. while the first batch of tiles is in flight: exactly that batch completes."""
    cam = mp.Camera.teapot_view()
    st = mp.RenderSettings(8, 2, (2048, 2048), seed=1)  # 65 536 tiles = several launch batches
    box = {}

    def on_start(t):
        if "rp" in box and not box.get("aborted"):
            box["aborted"] = True
            box["rp"].abort()

    import time

    rp = mp.render(teapot, cam, st, on_start)
    box["rp"] = rp
    t0 = time.time()
    while not box.get("aborted") and not rp.is_finished() and time.time() - t0 < 30:
        time.sleep(0.0005)
    rp.wait()
    p = rp.progress()
    assert rp.is_finished() and box.get("aborted")
    assert 0 < p.finished < p.total == 65536
    img = rp.image()
    assert img.shape == (2048, 2048, 4)
    # aborting a finished render is harmless
    rp.abort()
    assert rp.progress().finished == p.finished


def test_untile_color_to_image(ctx, teapot, oracle):
    """K7 + color_to_image (worker.rs:69-76) on the device incl. rounding ties, clamps and NaN."""
    import ctypes as C

    import torch

    from minipath_amd import _lib

    st = mp.RenderSettings(4, 1, (8, 4))
    tiles = mp.tile_ordering(mp.ScreenBlock(0, 0, 8, 4), 4)
    vals = np.array([0.5 / 255, 1.5 / 255, 2.5 / 255, 0.49999 / 255, 1.0, 2.0, -1.0, np.nan, 254.5 / 255, 0.0, 0.999, 127.5 / 255], np.float32)
    buf = np.resize(vals, (2, 4, 4, 4)).astype(np.float32)
    d = torch.from_numpy(buf).cuda()
    img = torch.zeros((4, 8, 4), dtype=torch.float32, device="cuda")
    img8 = torch.zeros((4, 8, 4), dtype=torch.uint8, device="cuda")
    tc = (_lib.Block * 2)(*[t.as_struct() for t in tiles])
    ss = st.as_struct()
    _lib.check(_lib.lib().mp_untile(ctx.handle, C.byref(ss), tc, 2, d.data_ptr(), img.data_ptr(), img8.data_ptr(), None))
    torch.cuda.synchronize()
    exp = np.concatenate([buf[0], buf[1]], axis=1)
    assert np.array_equal(bits(img.cpu().numpy()), bits(exp))
    out = np.zeros(4, np.uint8)
    e8 = np.zeros((4, 8, 4), np.uint8)
    for y in range(4):
        for x in range(8):
            oracle.lib().mpo_color_to_image(exp[y, x].ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_uint8)))
            e8[y, x] = out
    assert np.array_equal(img8.cpu().numpy(), e8)


def test_full_size_properties(teapot):
    """BASELINE config C2 geometry (teapot 1920x1080, tile 64) at reduced spp: size-independent properties.
    idempotence (two launches give identical bits); any subset of tiles reproduces the same pixels (tiles are
    independent units); alpha = hits/spp is a multiple of 1/spp in [0,1]; grey <= alpha."""
    import torch

    cam = mp.Camera.teapot_view()
    spp = 8
    st = mp.RenderSettings(64, spp, (1920, 1080), seed=SEED)
    fr = mp.FrameRenderer(teapot, cam, st)
    assert len(fr.tiles) == 510 and fr.rays_per_frame == 1920 * 1080 * spp
    a = fr.render().clone()
    b = fr.render().clone()
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    img, img8 = fr.untile()
    sub = fr.tiles[3::7]
    fr2 = mp.FrameRenderer(teapot, cam, st, tiles=sub)
    fr2.render()
    img2, _ = fr2.untile()
    torch.cuda.synchronize()
    img, img2 = img.cpu().numpy(), img2.cpu().numpy()
    for t in sub:
        assert np.array_equal(bits(img[t.min_y:t.max_y, t.min_x:t.max_x]), bits(img2[t.min_y:t.max_y, t.min_x:t.max_x]))
    alpha = img[..., 3]
    assert alpha.min() >= 0 and alpha.max() <= 1 and np.allclose(alpha * spp, np.round(alpha * spp), atol=1e-5)
    assert np.all(img[..., 0] <= alpha + 1e-6) and np.array_equal(img[..., 0], img[..., 1]) and np.array_equal(img[..., 0], img[..., 2])
    assert 0.05 < (alpha > 0).mean() < 0.6
    i8 = img8.cpu().numpy()
    assert np.array_equal(i8[..., 3] == 0, alpha < 0.5 / 255)


def test_golden_fixtures(teapot, ctx):
    """tests/golden/teapot_golden.npz (made by tests/golden/make_golden.py from the oracle): 4096 seeded rays and
    one 64x64 tile at 16 spp."""
    import os

    import torch

    from tests.conftest import GOLDEN

    g = np.load(os.path.join(GOLDEN, "teapot_golden.npz"))
    out = teapot.object.intersect(torch.from_numpy(g["ray_o"]).cuda(), torch.from_numpy(g["ray_d"]).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(out["prim"].cpu().numpy().view(np.uint32), g["hit_prim"])
    assert np.array_equal(bits(out["t"].cpu().numpy()), g["hit_t_bits"])
    hit = g["hit_prim"] != 0xFFFFFFFF
    assert np.array_equal(bits(out["u"].cpu().numpy())[hit], g["hit_u_bits"][hit])
    assert np.array_equal(bits(out["v"].cpu().numpy())[hit], g["hit_v_bits"][hit])
    st = mp.RenderSettings(64, 16, (256, 256), seed=int(g["seed"]))
    f, u8 = mp.render_tile(teapot, mp.Camera.teapot_view().build_sampler((256, 256)), st, mp.ScreenBlock(*[int(v) for v in g["tile"]]))
    assert np.array_equal(bits(f), g["tile_f32_bits"])
    assert np.array_equal(u8, g["tile_u8"])


@pytest.mark.parametrize("traversal", ["packets", "groups"])
@pytest.mark.parametrize("name", ["soup_5000", "grid_40", "sphere_24", "sliver_fan", "soup_300"])
def test_render_synthetic_scenes(ctx, oracle, name, traversal):
    """Whole small frames of synthetic scenes (flat shading, deep trees, shared-edge ties) against the oracle,
    with a camera looking at the scene: exercises the packet walk with partially culled lanes."""
    import ctypes as C

    pos, nrm, tex, tri = meshes.make(name)
    scene = mp.Scene(mp.TriangleBvh.build(pos, nrm, tex, tri, ctx))
    orc = oracle.Bvh.build(pos, nrm, tex, tri)
    bmin, bmax = orc.bbox()
    ctr = (bmin + bmax) / 2
    ext = float(np.max(bmax - bmin))
    eye = ctr + np.array([0.9, 0.7, 1.6], np.float32) * ext
    cam = mp.Camera.default().look_at(tuple(eye), tuple(ctr), (0, 1, 0)).f_number(2.0).sensor_height(36e-3)
    oc = oracle.Camera()
    oracle.lib().mpo_camera_default(C.byref(oc))
    oracle.lib().mpo_camera_look_at(C.byref(oc), oracle.vec3(*eye), oracle.vec3(*ctr), oracle.vec3(0, 1, 0))
    oc.f_number = 2.0
    oc.sensor_size = 36e-3
    res = (96, 72)
    st = mp.RenderSettings(32, 3, res, seed=11, traversal=traversal)
    fr = mp.FrameRenderer(scene, cam, st)
    fr.render()
    img, img8 = fr.untile()
    of, ou8, *_ = orc.render_image_mt(oracle.build_sampler(oc, *res), res[0], res[1], 3, 11, 32, 4)
    assert np.array_equal(bits(img.cpu().numpy()), bits(of))
    assert np.array_equal(img8.cpu().numpy(), ou8)
    assert (of[..., 3] > 0).mean() > 0.05


@pytest.mark.parametrize("regs", [64, 3])
def test_packet_stack_in_lds(oracle, teapot_oracle_bvh, regs):
    """The packet walk keeps the first `packet_stack_registers` entries of its shared stack in registers and the rest in
    LDS (HybridStack).  With the exact stack bound the shipped scenes fit in registers, so the knob is lowered to 3 to
    drive the LDS path (incl. the epoch-based lazy cull) on the teapot: the image must not change."""
    c = mp.Context(0)
    c.set_option("packet_stack_registers", regs)
    scene = mp.Scene(mp.TriangleBvh.with_obj(TEAPOT, c))
    assert scene.object.info().stack_bound > 3
    for max_depth in (0, 3):
        st = mp.RenderSettings(64, 8, (256, 256), seed=SEED, max_depth=max_depth)
        fr = mp.FrameRenderer(scene, mp.Camera.teapot_view(), st, tiles=[mp.ScreenBlock(64, 96, 128, 160)])
        got = fr.render()[0].cpu().numpy()
        lds = "true" if regs == 3 else "false"  # 8 samples: 8 in flight, too few passes for the mask cache
        want = "render_paths_kernel<8, false, false>" if max_depth else f"render_tiles_packet_kernel<8, {lds}, 7>"
        assert launched(c) == [want]
        s = oracle.build_sampler(oracle.teapot_camera(), 256, 256)
        if max_depth:
            of, _, _ = teapot_oracle_bvh.render_tile_paths(s, 256, 256, 8, SEED, max_depth, 64, 96, 128, 160)
        else:
            of, _ = teapot_oracle_bvh.render_tile(s, 256, 256, 8, SEED, 64, 96, 128, 160)
        assert np.array_equal(bits(got), bits(of))
    with pytest.raises(mp.MinipathError):
        c.set_option("packet_stack_registers", 65)
    with pytest.raises(mp.MinipathError):
        c.set_option("nope", 1)


@pytest.mark.parametrize("traversal", ["packets", "groups"])
def test_atrium_deep_tree(ctx, oracle, traversal):
    """Sponza stand-in (minipath_amd.scenes.atrium) at 5 % detail: 13 k triangles, 10 inner levels (7*depth+1 = 71, exact
    stack bound far lower); camera inside the hall (every ray hits something)."""
    import ctypes as C

    from minipath_amd import scenes

    pos, nrm, tex, tri = scenes.atrium(1, 0.05)
    bvh = mp.TriangleBvh.build(pos, nrm, tex, tri, ctx)
    assert 7 * bvh.info().depth + 1 > 64 and 1 < bvh.info().stack_bound <= 7 * bvh.info().depth + 1
    scene = mp.Scene(bvh)
    orc = oracle.Bvh.build(pos, nrm, tex, tri)
    cam = scenes.atrium_camera()
    oc = oracle.Camera()
    oracle.lib().mpo_camera_default(C.byref(oc))
    oracle.lib().mpo_camera_look_at(C.byref(oc), oracle.vec3(-16.0, 4.2, 0.8), oracle.vec3(12.0, 5.5, -0.5), oracle.vec3(0, 1, 0))
    oc.f_number = 4.0
    res = (160, 96)
    assert np.array_equal(bits(cam.build_sampler(res).as_array()), bits(oracle.build_sampler(oc, *res).as_array()))
    st = mp.RenderSettings(32, 9, res, seed=3, traversal=traversal)
    fr = mp.FrameRenderer(scene, cam, st)
    fr.render()
    img, img8 = fr.untile()
    of, ou8, *_ = orc.render_image_mt(oracle.build_sampler(oc, *res), res[0], res[1], 9, 3, 32, 8)
    assert np.array_equal(bits(img.cpu().numpy()), bits(of))
    assert np.array_equal(img8.cpu().numpy(), ou8)
    assert (of[..., 3] > 0).mean() > 0.95
    bmin, bmax = orc.bbox()
    o, d = meshes.random_rays(20000, 5, bmin, bmax)
    got, exp = _trace_both(scene, orc, o, d)
    _assert_hits_equal(got, exp)


@pytest.mark.parametrize("wavefront", [False, True])
@pytest.mark.parametrize("max_depth,spp,res,tile", [(8, 16, (256, 256), (64, 96, 128, 160)), (1, 5, (256, 256), (96, 96, 160, 160)),
                                                    (3, 9, (250, 130), (192, 64, 250, 128)), (2, 1, (256, 256), (64, 64, 128, 128)),
                                                    (4, 70, (256, 256), (96, 96, 128, 128))])
def test_path_extension_tile_bit_exact(teapot, oracle, teapot_oracle_bvh, max_depth, spp, res, tile, wavefront):
    """Build-defined path extension (MP_FLAG_PATHS; no reference counterpart): GPU == oracle restatement bit for bit,
    including the number of traced ray segments.  Camera rays on the packet walk, bounce rays compacted into the LDS
    queue and traced by the 8-lane-group traversal."""
    import torch

    cam = mp.Camera.teapot_view()
    st = mp.RenderSettings(64, spp, res, seed=SEED, max_depth=max_depth, wavefront=wavefront)
    fr = mp.FrameRenderer(teapot, cam, st, tiles=[mp.ScreenBlock(*tile)])
    buf = fr.render()
    torch.cuda.synchronize()
    tw, th = tile[2] - tile[0], tile[3] - tile[1]
    got = buf[0, :th, :tw].cpu().numpy()
    of, ou8, seg = teapot_oracle_bvh.render_tile_paths(oracle.build_sampler(oracle.teapot_camera(), *res), res[0], res[1], spp, SEED, max_depth, *tile)
    assert np.array_equal(bits(got), bits(of)), f"{int(np.sum(bits(got) != bits(of)))} differ"
    assert int(fr.segments.item()) == seg
    assert seg >= tw * th * spp
    if max_depth > 1:
        assert seg > tw * th * spp  # some paths bounced


def test_path_extension_atrium_and_frame(ctx, oracle):
    """Interior scene (every path bounces until max_depth or escapes never): deep tree + LDS queue/stack pressure."""
    import ctypes as C

    import torch

    from minipath_amd import scenes

    pos, nrm, tex, tri = scenes.atrium(1, 0.05)
    scene = mp.Scene(mp.TriangleBvh.build(pos, nrm, tex, tri, ctx))
    orc = oracle.Bvh.build(pos, nrm, tex, tri)
    oc = oracle.Camera()
    oracle.lib().mpo_camera_default(C.byref(oc))
    oracle.lib().mpo_camera_look_at(C.byref(oc), oracle.vec3(-16.0, 4.2, 0.8), oracle.vec3(12.0, 5.5, -0.5), oracle.vec3(0, 1, 0))
    oc.f_number = 4.0
    res = (96, 64)
    of, ou8, secs, seg = orc.render_image_paths_mt(oracle.build_sampler(oc, *res), res[0], res[1], 6, 5, 4, 32, 8)
    for wavefront in (False, True):  # fused kernel, then the staged evaluation with direction-sorted bounce packets
        st = mp.RenderSettings(32, 6, res, seed=5, max_depth=4, wavefront=wavefront)
        fr = mp.FrameRenderer(scene, scenes.atrium_camera(), st)
        fr.render()
        img, _ = fr.untile()
        torch.cuda.synchronize()
        assert np.array_equal(bits(img.cpu().numpy()), bits(of)), wavefront
        assert int(fr.segments.item()) == seg
    assert seg > 3 * res[0] * res[1] * 6  # closed hall: almost every path uses all four segments


def test_reference_mode_segment_count(teapot):
    import torch

    st = mp.RenderSettings(64, 3, (256, 256), seed=SEED)
    fr = mp.FrameRenderer(teapot, mp.Camera.teapot_view(), st)
    fr.render()
    torch.cuda.synchronize()
    assert int(fr.segments.item()) == 256 * 256 * 3 == fr.rays_per_frame
    with pytest.raises(ValueError):
        mp.RenderSettings(64, 1, (8, 8), traversal="nope").as_struct()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_sharded_render_reassembles_to_single_gpu_image(teapot, world):
    """SURVEY 8e on one device: every rank's shard rendered by its own launch into the gather layout (equal-size shards,
    empty padding blocks), rank-major concatenation, un-tile with the padded tile list == the one-GPU frame, bit for bit.
    (The RCCL gather itself is the only step not exercised; the same plan is exercised over gloo in test_distributed_cpu.)"""
    import torch

    from minipath_amd import _lib
    from minipath_amd.distributed import plan_shards

    cam = mp.Camera.teapot_view()
    st = mp.RenderSettings(32, 4, (200, 120), seed=SEED)
    ref = mp.FrameRenderer(teapot, cam, st)
    ref.render()
    ref_img, ref_u8 = ref.untile()
    plan = plan_shards(ref.tiles, world)
    ts = st.tile_size
    gather = torch.zeros((world * plan.per_rank, ts, ts, 4), dtype=torch.float32, device="cuda")
    for r in range(world):
        shard = gather[r * plan.per_rank:(r + 1) * plan.per_rank]
        mp.FrameRenderer(teapot, cam, st, tiles=plan.shards[r], tile_buf=shard).render()
    order = plan.gather_order
    order_c = (_lib.Block * len(order))(*[t.as_struct() for t in order])
    img, img8 = ref.untile(gather, (order, order_c), reuse=False)
    torch.cuda.synchronize()
    assert torch.equal(img.view(torch.int32), ref_img.view(torch.int32)) and torch.equal(img8, ref_u8)


def test_sphere_object(ctx, oracle):
    """scene/primitives.rs: Sphere as the scene's Object -- the reference's three known answers (:62-97) through
    mp_trace_rays, random rays vs the oracle (bit-exact t / point / normal), and render_tile parity in both kernels."""
    import torch

    sph = mp.Sphere((1.0, 2.0, 3.0), 1.0, ctx)
    o = torch.tensor([[1.0, 2.0, 0.0], [2.0, 2.0, 0.0], [2.0, 2.01, 0.0]], device="cuda")
    d = torch.tensor([[0.0, 0.0, 1.0]] * 3, device="cuda")
    out = sph.intersect(o, d, full=True)
    t = out["t"].cpu().numpy()
    assert abs(t[0] - 2.0) < 1e-6 and abs(t[1] - 3.0) < 1e-6 and out["prim"].cpu().numpy().view(np.uint32)[2] == 0xFFFFFFFF
    bmin, bmax = sph.get_bounding_box()
    assert np.allclose(bmin, [0, 1, 2]) and np.allclose(bmax, [2, 3, 4])
    ro, rd = meshes.random_rays(5000, 3, bmin, bmax)
    out = sph.intersect(torch.from_numpy(ro).cuda(), torch.from_numpy(rd).cuda(), full=True)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    nh = 0
    for i in range(0, 5000, 7):
        h = oracle.sphere_intersect((1.0, 2.0, 3.0), 1.0, oracle.ray_new(ro[i], rd[i]))
        assert (got["prim"].view(np.uint32)[i] != 0xFFFFFFFF) == bool(h.hit)
        if h.hit:
            nh += 1
            assert bits(got["t"][i:i + 1])[0] == bits(np.array([h.t], np.float32))[0]
            assert np.array_equal(bits(got["normal"][i]), bits(np.array(list(h.normal), np.float32)))
            assert np.array_equal(bits(got["point"][i]), bits(np.array(list(h.point), np.float32)))
    assert nh > 50
    cam = mp.Camera.default().look_at((1.0, 2.0, -4.0), (1.0, 2.0, 3.0), (0, 1, 0)).f_number(2.0)
    oc = oracle.Camera()
    import ctypes as C
    oracle.lib().mpo_camera_default(C.byref(oc))
    oracle.lib().mpo_camera_look_at(C.byref(oc), oracle.vec3(1.0, 2.0, -4.0), oracle.vec3(1.0, 2.0, 3.0), oracle.vec3(0, 1, 0))
    oc.f_number = 2.0
    for traversal in ("packets", "groups"):
        st = mp.RenderSettings(64, 5, (128, 128), seed=9, traversal=traversal)
        f, u8 = mp.render_tile(mp.Scene(sph), cam.build_sampler((128, 128)), st, mp.ScreenBlock(32, 32, 96, 96))
        of, ou8 = oracle.render_tile_sphere((1.0, 2.0, 3.0), 1.0, oracle.build_sampler(oc, 128, 128), 128, 5, 9, 32, 32, 96, 96)
        assert np.array_equal(bits(f), bits(of)) and np.array_equal(u8, ou8)
        assert (of[..., 3] > 0).mean() > 0.2
    with pytest.raises(mp.MinipathError) as e:  # the build-defined path extension is specified for TriangleBvh only
        mp.render_tile(mp.Scene(sph), cam.build_sampler((128, 128)), mp.RenderSettings(64, 1, (128, 128), max_depth=2), mp.ScreenBlock(0, 0, 64, 64))
    assert e.value.code == 5


@pytest.mark.parametrize("max_depth,traversal", [(0, "packets"), (0, "groups"), (5, "packets"), (5, "wavefront")])
def test_progressive_passes_equal_single_launch(teapot, tmp_path, max_depth, traversal):
    """MP_FLAG_ACCUMULATE: the samples of a frame drawn in several launches (ragged pass sizes, not multiples of the 8 samples in
    flight) accumulate to the bit-identical frame of one launch, also through a checkpoint file and a fresh renderer; the running
    state between passes is (sum, sum, sum, hit count)."""
    import torch

    from minipath_amd import io

    cam = mp.Camera.teapot_view()
    wavefront = traversal == "wavefront"
    traversal = "packets" if wavefront else traversal
    st = mp.RenderSettings(32, 23, (96, 80), seed=SEED, traversal=traversal, max_depth=max_depth, wavefront=wavefront)
    ref = mp.FrameRenderer(teapot, cam, st)
    ref.render()
    ref_img, ref_u8 = ref.untile()
    ref_seg = int(ref.segments.item())
    prog = mp.FrameRenderer(teapot, cam, st)
    nxt, seg = 0, 0
    for count in (1, 7, 9):  # 17 samples, then a checkpoint
        nxt = prog.render_pass(nxt, count)
        seg += int(prog.segments.item())
    assert nxt == 17
    mid = prog.tile_buf.clone()
    assert float(mid[..., 3].max()) <= 17.0 and torch.equal(mid[..., 0], mid[..., 1])  # sums and hit counts, not means
    assert float(mid[..., 3].max()) == 17.0  # some pixel was hit by every sample so far
    ck = str(tmp_path / "frame.ckpt.npz")
    io.save_checkpoint(ck, prog, nxt)
    resumed = mp.FrameRenderer(teapot, cam, st)
    nxt2 = io.load_checkpoint(ck, resumed)
    assert nxt2 == 17
    assert resumed.render_pass(nxt2, 2) == 19
    seg += int(resumed.segments.item())
    assert resumed.render_pass(19) == 23  # through the last sample: writes the means
    seg += int(resumed.segments.item())
    img, u8 = resumed.untile()
    torch.cuda.synchronize()
    assert torch.equal(img.view(torch.int32), ref_img.view(torch.int32)) and torch.equal(u8, ref_u8)
    assert seg == ref_seg
    with pytest.raises(ValueError):
        resumed.render_pass(23)
    with pytest.raises(ValueError):
        io.load_checkpoint(ck, mp.FrameRenderer(teapot, cam, mp.RenderSettings(32, 24, (96, 80), seed=SEED, traversal=traversal, max_depth=max_depth)))
    # the flag is refused where the library owns the tile buffer
    bad = st.as_struct()
    bad.flags |= 8
    from minipath_amd import _lib
    import ctypes as C

    out = np.zeros((32, 32, 4), np.float32)
    smp = cam.build_sampler((96, 80)).as_struct()
    rc = _lib.lib().mp_render_tile(teapot.object.ctx.handle, teapot.object.handle, C.byref(smp), C.byref(bad),
                                   mp.ScreenBlock(0, 0, 32, 32).as_struct(), out.ctypes.data, None)
    assert rc != 0


def test_two_rays_per_lane_walk_is_bit_identical(teapot, oracle, teapot_oracle_bvh):
    """mp_ctx_set_option("packet_rays_per_lane", 2): 128-ray walks (two rays per lane, 4x2-pixel units) must give the frame of the
    64-ray walk and of the oracle bit for bit, incl. clipped tiles, ragged progressive passes and the chunked accumulation rule.
    The option takes effect only where the launcher has 16 samples in flight (a plain scene, stack in registers); at other
    counts it is ignored and the 64-ray kernels run, so the test asks for 16 and checks the name of every launch."""
    import torch

    ctx = teapot.object.ctx
    cam = mp.Camera.teapot_view()
    res, spp = (250, 131), 37
    of, ou8, *_ = teapot_oracle_bvh.render_image_mt(oracle.build_sampler(oracle.teapot_camera(), *res), res[0], res[1], spp, SEED, 32, 8)
    try:
        ctx.set_option("packet_rays_per_lane", 2)
        # the 128-ray walk exists for 16 samples in flight only; left to itself the launcher gives these sample counts 4, 8 or 32
        # (mask cache, small launch) and the 64-ray kernels -- so 16 are asked for, and the name of what ran is checked
        ctx.set_option("packet_samples_in_flight", 16)
        st = mp.RenderSettings(32, spp, res, seed=SEED)
        fr = mp.FrameRenderer(teapot, cam, st)
        fr.render()
        assert launched(ctx) == ["render_tiles_packet2_kernel<6>"]
        img, img8 = fr.untile()
        torch.cuda.synchronize()
        assert np.array_equal(bits(img.cpu().numpy()), bits(of)) and np.array_equal(img8.cpu().numpy(), ou8)
        pr = mp.FrameRenderer(teapot, cam, st)
        nxt = 0
        for count in (16, 5, 0):
            nxt = pr.render_pass(nxt, count)
            assert launched(ctx) == ["render_tiles_packet2_kernel<6>"]
        img2, _ = pr.untile()
        torch.cuda.synchronize()
        assert torch.equal(img2.view(torch.int32), img.view(torch.int32))
        stc = mp.RenderSettings(32, 300, (64, 40), seed=SEED, chunked_sum=True)
        two = mp.FrameRenderer(teapot, cam, stc); two.render()
        assert launched(ctx) == ["render_tiles_packet2_kernel<6>"]
        a, _ = two.untile()
        ctx.set_option("packet_rays_per_lane", 1)
        one = mp.FrameRenderer(teapot, cam, stc); one.render()
        assert launched(ctx) == ["render_tiles_packet_kernel<16, false, 8, false, true>"]
        b, _ = one.untile()
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    finally:
        ctx.set_option("packet_rays_per_lane", 1)
        ctx.set_option("packet_samples_in_flight", 0)


def test_samples_in_flight_do_not_change_the_frame(teapot, oracle, teapot_oracle_bvh):
    """The number of samples of a pixel a wavefront holds per pass (work-unit size; 16 = one DPP row with row_newbcast sums,
    others through lane shuffles) must not change a single bit: the per-pixel sum stays sequential in sample order."""
    import torch

    res, spp = (72, 40), 37  # ragged: not a multiple of any S, clipped tiles
    st = mp.RenderSettings(32, spp, res, seed=SEED)
    cam = mp.Camera.teapot_view()
    ctx = teapot.object.ctx
    want, _, _, _, _ = teapot_oracle_bvh.render_image_mt(oracle.build_sampler(oracle.teapot_camera(), *res), res[0], res[1], spp, SEED, 32, 4)
    try:
        for s_in_flight in (1, 2, 4, 8, 16, 32, 64):
            ctx.set_option("packet_samples_in_flight", s_in_flight)
            fr = mp.FrameRenderer(teapot, cam, st)
            fr.render()
            # S in the kernel's name is the S asked for, every time; 37 samples are four passes or more of 4 and of 8: those two run
            # on the mask cache's form
            form = "8, false, true" if s_in_flight in (4, 8) else "7"
            assert launched(ctx) == [f"render_tiles_packet_kernel<{s_in_flight}, false, {form}>"]
            img, _ = fr.untile()
            torch.cuda.synchronize()
            assert np.array_equal(bits(img.cpu().numpy()), bits(want)), s_in_flight
        with pytest.raises(mp.MinipathError):
            ctx.set_option("packet_samples_in_flight", 3)
    finally:
        ctx.set_option("packet_samples_in_flight", 0)


@pytest.mark.parametrize("max_depth", [0, 4])
def test_profile_guided_tile_order_same_image(teapot, max_depth):
    """mp_launch_extras: tiles handed out in any order (here: by the measured cost of a first launch, then reversed) render the
    same frame, the per-tile cost counters fill, and a non-permutation is refused."""
    import ctypes as C

    import torch

    from minipath_amd import _lib

    st = mp.RenderSettings(32, 9, (200, 136), seed=SEED, max_depth=max_depth)
    fr = mp.FrameRenderer(teapot, mp.Camera.teapot_view(), st)
    fr.render()
    ref = fr.tile_buf.clone()
    torch.cuda.synchronize()
    cost = fr.tile_cost.cpu().numpy()
    assert (cost[: len(fr.tiles)] > 0).all()
    order = fr.rebalance()
    assert sorted(order) == list(range(len(fr.tiles))) and int(fr.tile_cost.sum().item()) == 0
    assert cost[order[0]] == cost.max()  # most expensive tile first
    fr.tile_buf.zero_()
    fr.render()
    torch.cuda.synchronize()
    assert torch.equal(fr.tile_buf.view(torch.int32), ref.view(torch.int32))
    rev = order[::-1]
    fr._order_c = (C.c_uint32 * len(rev))(*rev)
    fr._extras.tile_order = C.cast(fr._order_c, C.POINTER(C.c_uint32))
    fr.tile_buf.zero_()
    fr.render()
    torch.cuda.synchronize()
    assert torch.equal(fr.tile_buf.view(torch.int32), ref.view(torch.int32))
    bad = list(order)
    bad[0] = bad[1]
    fr._order_c = (C.c_uint32 * len(bad))(*bad)
    fr._extras.tile_order = C.cast(fr._order_c, C.POINTER(C.c_uint32))
    with pytest.raises(_lib.MinipathError):
        fr.render()


def test_tile_list_cache_eviction(teapot, oracle, teapot_oracle_bvh):
    """The context keeps device copies of the tile lists callers pass (32 entries, least recently used evicted): more distinct
    lists than that, re-used afterwards, still render their own tiles."""
    import torch

    res, spp = (512, 512), 2
    st = mp.RenderSettings(32, spp, res, seed=SEED)
    cam = mp.Camera.teapot_view()
    smp = oracle.build_sampler(oracle.teapot_camera(), *res)
    lists = [[mp.ScreenBlock(32 * (i % 16), 32 * (i // 16) + 128, 32 * (i % 16) + 32, 32 * (i // 16) + 160)] for i in range(40)]
    renderers = [mp.FrameRenderer(teapot, cam, st, tiles=tl) for tl in lists]
    for rounds in range(2):  # second round: the first eight lists were evicted in the first
        for fr in renderers:
            fr.tile_buf.zero_()
            fr.render()
        torch.cuda.synchronize()
        for i in (0, 7, 21, 39):
            t = lists[i][0]
            want, _ = teapot_oracle_bvh.render_tile(smp, res[0], res[1], spp, SEED, t.min_x, t.min_y, t.max_x, t.max_y)
            assert np.array_equal(bits(renderers[i].tile_buf[0].cpu().numpy()), bits(want)), (rounds, i)


def test_tile_list_cache_eviction_under_two_threads(teapot, oracle, teapot_oracle_bvh):
    """two host threads launching through one context with more distinct tile lists than the cache holds (each on
    its own stream): a list evicted by one thread between the other thread's lookup and its launch must stay alive (the cache
    hands out reference-counted entries).  Every tile must still be the oracle's."""
    import threading

    import torch

    res, spp = (512, 512), 2
    st = mp.RenderSettings(32, spp, res, seed=SEED)
    cam = mp.Camera.teapot_view()
    smp = oracle.build_sampler(oracle.teapot_camera(), *res)
    lists = [[mp.ScreenBlock(32 * (i % 16), 32 * (i // 16) + 96, 32 * (i % 16) + 32, 32 * (i // 16) + 128)] for i in range(96)]
    renderers = [mp.FrameRenderer(teapot, cam, st, tiles=tl) for tl in lists]
    errors = []

    def work(part):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                for _ in range(3):
                    for fr in part:
                        fr.render()
            stream.synchronize()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(renderers[k::2],)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    torch.cuda.synchronize()
    assert not errors, errors
    for i in (0, 1, 33, 64, 95):
        t = lists[i][0]
        want, _ = teapot_oracle_bvh.render_tile(smp, res[0], res[1], spp, SEED, t.min_x, t.min_y, t.max_x, t.max_y)
        assert np.array_equal(bits(renderers[i].tile_buf[0].cpu().numpy()), bits(want)), i


def test_differential_fuzz(ctx):
    """tools/fuzz_gpu.py, bounded: random scenes / cameras (incl. axis-aligned views with zero direction components) / sizes /
    sample counts / kernels (packets, groups, fused paths, staged paths) / work-unit sizes / stack splits / progressive splits,
    every frame bit-identical to the oracle.  (Round 1 ran 10 650 such cases with no mismatch.)"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("fuzz_gpu", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(60, 20261005, ctx) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("balance", ["static", "lpt"])
def test_bench_two_rank_rehearsal(balance):
    """bench.py's N > 1 path (shard plan, gather to rank 0, reassembly, max-over-ranks timing) with two ranks sharing this
    box's GPU over gloo (MP_BENCH_REHEARSAL=1: RCCL refuses duplicate devices); the gathered frame is checked against the
    oracle inside bench.py (--check)."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MP_BENCH_REHEARSAL="1", MASTER_ADDR="127.0.0.1")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None)
    bench_args = [os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--scene", "teapot", "--width", "320",
                  "--height", "200", "--spp", "16", "--no-cpu-baseline", "--no-extension", "--check", "--balance", balance]
    if balance == "static":  # the driver's form: launched by torch.distributed.run
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", "29533"] + bench_args
    else:                    # the plain form: bench.py starts its own ranks (child processes) and relays rank 0's line
        cmd = [sys.executable] + bench_args
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["check_mismatches"] == 0
    assert d["config"]["rays_per_step"] == 320 * 200 * 16


@pytest.mark.gpu
def test_bench_two_rank_progressive_rehearsal():
    """BASELINE configs[4]'s shape through bench.py's N > 1 path (VERDICT r2 #4b): every frame = 3 ragged progressive passes, the
    running sums stay in each rank's shard, ONE gather per frame after the last pass; two ranks share this box's GPU over gloo.
    The gathered frame equals the oracle's single-pass frame (--check)."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MP_BENCH_REHEARSAL="1", MASTER_ADDR="127.0.0.1")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--scene", "teapot", "--width", "320",
           "--height", "200", "--spp", "40", "--depth", "3", "--progressive", "3", "--no-cpu-baseline", "--no-extension", "--check"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 2 and d["check_mismatches"] == 0 and "3 progressive passes" in d["config"]["parallelism"]
    assert 320 * 200 * 40 < d["config"]["rays_per_step"] <= 320 * 200 * 40 * 3


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_frame(tmp_path, oracle, teapot_oracle_bvh):
    """A plain bench.py run (no --full) times exactly --steps frames, carries none of the --full keys, and --dump-outputs writes
    the last timed frame: f32 bit-exact and u8 exact against the oracle's render of the same frame."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None); env.pop("RANK", None)
    w, h, spp = 320, 200, 16
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--scene", "teapot",
           "--width", str(w), "--height", str(h), "--spp", str(spp), "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["config"]["rays_per_step"] == w * h * spp
    assert not {"teapot_c2", "paths_depth8", "cpu_baseline"} & set(d)
    img, img8 = np.load(tmp_path / "image.npy"), np.load(tmp_path / "image_u8.npy")
    assert img.shape == img8.shape == (h, w, 4) and img.dtype == img8.dtype == np.float32
    of, ou8, *_ = teapot_oracle_bvh.render_image_mt(oracle.build_sampler(oracle.teapot_camera(), w, h), w, h, spp, SEED, 64, 8)
    assert np.array_equal(bits(img), bits(of))
    assert np.array_equal(img8, ou8.astype(np.float32))
