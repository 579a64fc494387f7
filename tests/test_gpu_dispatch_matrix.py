"""GPU dispatch matrix (-m gpu): one case per kernel instantiation of tests/dispatch_cases.py (= every row of kernel_table.h, see
tests/test_dispatch_census_cpu.py).  Each case builds the smallest input that selects its instantiation, runs it through the
public API, asserts that mp_ctx_last_kernels names exactly that instantiation, and compares the result bit for bit with the
oracle's for the same input (never with another GPU run).  Then the gate cases -- the mask cache's guards must send a frame to the
UNCACHED kernel for the right reason -- and frames rendered as ragged MP_FLAG_ACCUMULATE passes, whose kernels follow the samples
of each pass.

The matrix's own tiling never cuts a work unit (dispatch_cases' header), so every render / paths / wf / aov row, and the ragged
passes, run once more per tile list of tests/tile_geometries.py, against the same oracle frames: the row's names, the frame bit for
bit, and -- in a tile buffer pre-filled with a sentinel between sentinel guards -- not one word changed outside the blocks.  Last,
the staged pipeline on 26 tiles in 64 x 64 slots (dispatch_cases.STAGED_BATCHES): several tile batches of several sample chunks."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib, scenes
from tests import aov_model, meshes
from tests import dispatch_cases as dc
from tests import plan_probe as pp
from tests import tile_geometries as tg
from tests.conftest import TEAPOT

pytestmark = pytest.mark.gpu

F = np.float32
NO = 0xFFFFFFFF
FMAX = np.finfo(np.float32).max
SEED = 0x5EED
SENTINEL = 0x5A5A5A5A  # as a float 1.5e16: no pixel of a frame; as an id no primitive of these scenes
PAD = 4096
RES, TS, AOV_RES, AOV_TS, DEPTH = dc.RES, dc.TS, dc.AOV_RES, dc.AOV_TS, dc.DEPTH  # the frames the CPU plan tests size the same rows with
GREY = [(0.8, 0.0), (0.2, 2.5), (0.6, 0.0)]
RGB = [{"albedo": (0.9, 0.85, 0.8), "albedo2": (0.1, 0.15, 0.7), "checker": 6.0}, ((0.7, 0.2, 0.3), (0.0, 0.0, 0.0)),
       {"albedo": 0.4, "emission": (1.5, 0.5, 0.0), "albedo2": (0.2, 0.9, 0.2), "checker": 0.75}]
BALL = ((0.4, 0.0, 0.0), 1.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class World:
    """The context, the scenes (GPU object + oracle twin + camera), and the oracle's results, each built once per module."""

    def __init__(self, oracle):
        import torch

        assert torch.cuda.is_available(), "gpu tests need a GPU"
        self.oracle, self.ctx = oracle, mp.Context(0)
        self._scenes, self._renders, self._facts, self._planes = {}, {}, {}, {}

    def options(self, row=None):
        for k, v in {**dc.DEFAULTS, **(row["opts"] if row else {})}.items():
            self.ctx.set_option(k, v)

    def scene(self, key):
        """{"gpu", "cam", "table", "orc" (Bvh whose render_* / intersect / trace_inst speak for the scene) | "sphere" (c, r), "group"}"""
        if key in self._scenes:
            return self._scenes[key]
        o, ctx = self.oracle, self.ctx
        base, _, rgb = key.partition("+")
        s = {"table": None, "group": False}
        if base == "teapot":
            s.update(gpu=mp.TriangleBvh.with_obj(TEAPOT, ctx), orc=o.Bvh.from_obj(TEAPOT), cam=mp.Camera.teapot_view())
            if rgb:
                s["table"] = RGB[:1]
                s["gpu"].set_materials(RGB[:1], 0.7)
                s["orc"].set_materials(RGB[:1], 0.7)
        elif base == "group":
            pos, nrm, tex, tri = meshes.make("soup_300")
            mat = (np.arange(tri.shape[0]) % 3).astype(np.uint32)
            members = [mp.TriangleBvh.with_obj(TEAPOT, ctx), mp.TriangleBvh.build(pos, nrm, tex, tri, ctx, tri_material=mat), mp.Sphere(*BALL, ctx)]
            twins = [o.Bvh.from_obj(TEAPOT), o.Bvh.build(pos, nrm, tex, tri, tri_material=mat), BALL]
            tr = np.array([[0, 0, 0], [4.0, 1.5, -1.0], [0.0, 4.0, -1.0]], F)
            r = F(np.sqrt(0.5))
            q = np.array([[0, 0, 0, 1], [r, 0, 0, r], [0, 0, 0, 1]], F)
            table, sky = (RGB, 0.5) if rgb else (GREY, 0.25)
            gpu, box = mp.ObjectGroup(members, tr, rotations=q), o.Bvh.from_obj(TEAPOT)
            gpu.set_materials(table, sky)
            box.set_materials(table, sky)
            box.set_group(twins, tr, rotations=q)
            s.update(gpu=gpu, orc=box, cam=mp.Camera.default().look_at((1.0, 6.0, 13.0), (0.0, 2.0, 0.0), (0, 1, 0)), table=table, group=True,
                     keep=(members, twins))
        elif base in ("atrium", "atrium*2^27"):
            pos, nrm, tex, tri = scenes.atrium(1, 0.08)
            eye, at = (-45.0, 22.0, 30.0), (0.0, 5.0, 0.0)  # from outside the hall: its walls, and sky around them
            if base == "atrium":
                cam = mp.Camera.default().look_at(eye, at, (0, 1, 0)).f_number(4.0)
            else:  # a pinhole: the lens radius does not scale with the scene
                k = F(2.0 ** 27)
                pos = (pos * k).astype(F)
                eye, at = [tuple(float(F(x) * k) for x in p) for p in (eye, at)]
                cam = mp.Camera.default().look_at(eye, at, (0, 1, 0)).f_number(1e30)
                assert np.abs(pos).max() > 2.0 ** 30
            s.update(gpu=mp.TriangleBvh.build(pos, nrm, tex, tri, ctx), orc=o.Bvh.build(pos, nrm, tex, tri), cam=cam)
            i = s["gpu"].info()
            assert len(s["gpu"].device_tree()[0]) * 256 + i.packet_count * 384 > 1 << 20, "the big-scene rule of the launcher"
            assert i.stack_bound <= 64
        elif base == "sphere":
            c, r = (0.2, 0.5, -0.3), 1.5
            s.update(gpu=mp.Sphere(c, r, ctx), sphere=(c, r), cam=mp.Camera.default().look_at((0.4, 5.0, 4.5), (0.0, 0.0, 0.0), (0, 1, 0)))
        else:
            raise KeyError(key)
        self._scenes[key] = s
        return s

    def sampler(self, key, res):
        return self.oracle.sampler_from_array(self.scene(key)["cam"].build_sampler(res).as_array())

    def expected(self, key, kind, res, spp, chunked=False):
        """the oracle's frame: (f32, u8, ray segments or None); kind "render" or "paths"; cached.  The oracle renders with the
        matrix's TS whatever tile list the GPU gets: its image does not depend on the tiling.  chunked: MP_FLAG_CHUNKED_SUM's rule"""
        k = (key, kind, res, spp) + (("chunked",) if chunked else ())
        if k not in self._renders:
            s, smp = self.scene(key), self.sampler(key, res)
            if "sphere" in s:
                assert kind == "render" and not chunked
                f, u8 = self.oracle.render_tile_sphere(*s["sphere"], smp, res[0], spp, SEED, 0, 0, res[0], res[1])
                self._renders[k] = (f, u8, None)
            elif kind == "render":
                assert not chunked
                f, u8, *_ = s["orc"].render_image_mt(smp, res[0], res[1], spp, SEED, TS, 16)
                self._renders[k] = (f, u8, None)
            else:
                self.oracle.lib().mpo_set_chunked_sum(1 if chunked else 0)
                try:
                    f, u8, _, seg = s["orc"].render_image_paths_mt(smp, res[0], res[1], spp, SEED, DEPTH, TS, 16)
                finally:
                    self.oracle.lib().mpo_set_chunked_sum(0)
                self._renders[k] = (f, u8, seg)
        return self._renders[k]

    def expected_planes(self, key, spp):
        """the feature planes' model over the oracle for the whole AOV frame, image-major; cached per (scene, samples)"""
        k = (key, spp)
        if k not in self._planes:
            s = self.scene(key)
            self._planes[k] = aov_model.planes(self.oracle, s["orc"].intersect, self.sampler(key, AOV_RES), AOV_RES[0], spp, SEED,
                                               (0, 0, AOV_RES[0], AOV_RES[1]), s["table"])
        return self._planes[k]

    def view_facts(self, key, res):
        """what the first sample of every pixel sees, from the oracle: (hit mask, member index per pixel)"""
        k = (key.partition("+")[0], res)
        if k not in self._facts:
            s, smp, o = self.scene(key), self.sampler(key, res), self.oracle
            if "sphere" in s:
                f, _, _ = self.expected(key, "render", res, 1)
                self._facts[k] = (f[..., 3].reshape(-1) > 0, None)
            else:
                org, dr = np.zeros((res[0] * res[1], 3), F), np.zeros((res[0] * res[1], 3), F)
                for y in range(res[1]):
                    for x in range(res[0]):
                        r = o.sample_ray(smp, x, y, o.lib().mpo_sample_key(C.c_uint64(SEED), res[0], 1, x, y, 0))
                        org[y * res[0] + x], dr[y * res[0] + x] = list(r.o), list(r.d)
                _, prim, _, _, inst = s["orc"].trace_inst(org, dr) if s["group"] else (*s["orc"].trace(org, dr), None)
                self._facts[k] = (prim != NO, inst)
        return self._facts[k]

    def assert_not_vacuous(self, key, res, f=None):
        s = self.scene(key)
        hit, inst = self.view_facts(key, res)
        assert 0 < hit.sum() < hit.size, "the view must hold hits and misses"
        if s["group"]:
            assert len(np.unique(inst[hit])) >= 2, "at least two members of the group in view"
        if s["table"] is not None and f is not None and len(s["table"]) and key.endswith("+rgb"):
            px = f[..., :3].reshape(-1, 3)[hit]
            chroma = np.round(px / np.maximum(px.max(axis=1, keepdims=True), 1e-20), 2)
            assert len(np.unique(chroma, axis=0)) >= 2, "at least two distinct colours in view"

    def kernels(self):
        return dc.launched(self.ctx)


@pytest.fixture(scope="module")
def world(oracle):
    w = World(oracle)
    yield w
    w.options()


def _stack_in_lds(world, row):
    regs = row["opts"].get("packet_stack_registers", 64)
    bound = world.scene(row["scene"])["gpu"].info().stack_bound
    if regs < 64:
        assert bound > regs, "the case lowers packet_stack_registers below the scene's stack bound"
    else:
        assert bound <= regs


class GuardedTiles:
    """a tile-major buffer [n, ts, ts, 4] (float32, or int32 for the "ids" plane) pre-filled with the sentinel, in the middle of a
    larger tensor of sentinels: include/minipath_hip.h's "clipped tiles leave the rest untouched", for blocks anywhere in their slot"""

    def __init__(self, blocks, ts, ids=False):
        import torch

        self.blocks, self.ts, self.count = blocks, ts, len(blocks) * ts * ts * 4
        self.whole = torch.full((PAD + self.count + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
        body = self.whole[PAD:PAD + self.count]
        self.buf = (body if ids else body.view(torch.float32)).view(len(blocks), ts, ts, 4)
        assert self.buf.data_ptr() == self.whole.data_ptr() + 4 * PAD and self.buf.data_ptr() % 16 == 0
        self.own = tg.owned(blocks, ts)

    def refill(self):
        self.whole.fill_(SENTINEL)

    def assert_rest_untouched(self, what=""):
        """after a synchronize: every word of a slot outside its block's w x h still holds the sentinel, and so do the guards"""
        raw = self.whole.cpu().numpy().view(np.uint32)
        assert np.all(raw[:PAD] == SENTINEL) and np.all(raw[-PAD:] == SENTINEL), f"{what}: a guard was written"
        body = raw[PAD:-PAD].reshape(len(self.blocks), self.ts, self.ts, 4)
        changed = body[~self.own] != SENTINEL
        assert not changed.any(), f"{what}: {int(changed.sum())} words changed outside the blocks, slots {np.unique(np.nonzero(changed)[0]).tolist()[:8]}"
        assert (body[self.own] != SENTINEL).any(axis=-1).all(), f"{what}: a pixel of a block was not written"


def _assert_names(names, expect):
    if isinstance(expect, set):
        assert set(names) == expect and len(names) == len(expect), names
    else:
        assert names == expect, names


def _rebalanced(fr, staged=False):
    """FrameRenderer.rebalance() after a launch on the "ragged" list: every tile was charged, and the order it installs -- the
    most expensive first, where the list begins with a block of three pixels -- is not the identity.  The staged pipeline ignores
    tile_order / d_tile_cost (include/minipath_hip.h): there nothing is charged and the frame must simply not change."""
    n = len(fr.tiles)
    cost = fr.tile_cost[:n].cpu().numpy().copy()
    order = fr.rebalance()
    assert sorted(order) == list(range(n))
    if staged:
        assert not cost.any()
        return
    assert np.all(cost > 0), f"tiles without a cost: {np.nonzero(cost == 0)[0].tolist()}"
    assert order != list(range(n)), "the hand-out order must differ from the list's"


def _frame(world, row, expect, res=RES, geometry="grid"):
    """render / paths / wf rows: one frame through FrameRenderer over the tile list of `geometry`, into a sentinel-filled buffer
    between guards: the names reported, the frame against the oracle, nothing written outside the blocks"""
    import torch

    s = world.scene(row["scene"])
    paths = row["api"] in ("paths", "wf")
    tile_size, blocks = tg.geometry(geometry, res, TS)
    st = mp.RenderSettings(tile_size, row["spp"], res, seed=SEED, traversal=row["traversal"], max_depth=DEPTH if paths else 0,
                           wavefront=row["api"] == "wf")
    of, ou8, oseg = world.expected(row["scene"], "paths" if paths else "render", res, row["spp"])
    world.assert_not_vacuous(row["scene"], res, of)
    if "sphere" not in s:
        _stack_in_lds(world, row)
    g = GuardedTiles(blocks, tile_size)
    fr = mp.FrameRenderer(mp.Scene(s["gpu"]), s["cam"], st, tiles=None if geometry == "grid" else blocks, tile_buf=g.buf)
    assert fr.tiles == blocks and sum(t.area() for t in blocks) == res[0] * res[1]

    def render_and_check(what):
        fr.render()
        names = world.kernels()
        img, img8 = fr.untile()
        torch.cuda.synchronize()
        _assert_names(names, expect)
        got = img.cpu().numpy()
        assert np.array_equal(bits(got), bits(of)), f"{what}: {int(np.sum(bits(got) != bits(of)))} f32 values differ"
        assert np.array_equal(img8.cpu().numpy(), ou8), what
        seg = int(fr.segments.item())
        if paths:
            assert seg == oseg and seg > res[0] * res[1] * row["spp"], "paths bounce: more segments than camera rays"
        else:
            assert seg == sum(t.area() for t in blocks) * row["spp"]
        g.assert_rest_untouched(what)

    render_and_check(geometry)
    if geometry == "ragged":  # the measured hand-out order, over units that are mostly outside their tile: the same bits
        _rebalanced(fr, staged=row["api"] == "wf")
        g.refill()
        render_and_check("ragged, rebalanced")


def _aov(world, name, row, geometry="grid"):
    import torch

    s = world.scene(row["scene"])
    _stack_in_lds(world, row)
    want = world.expected_planes(row["scene"], row["spp"])
    hits = want["ids"][..., 3]
    assert 0 < hits.sum() < hits.size, "the view must hold hits and misses"
    if s["group"]:
        assert len(np.unique(want["ids"][..., 1][hits == 1])) >= 2, "at least two members in view"
        assert len(np.unique(want["albedo"][..., :3].reshape(-1, 3)[hits.reshape(-1) == 1], axis=0)) >= 2, "at least two colours in view"
    tile_size, blocks = tg.geometry(geometry, AOV_RES, AOV_TS)
    fr = mp.FrameRenderer(mp.Scene(s["gpu"]), s["cam"], mp.RenderSettings(tile_size, row["spp"], AOV_RES, seed=SEED),
                          tiles=None if geometry == "grid" else blocks)
    assert fr.tiles == blocks

    def same_as_model(planes, what):
        img = {k: fr.untile_plane(v) for k, v in planes.items()}
        torch.cuda.synchronize()
        for k in ("shade", "normal", "albedo", "ids"):
            got = img[k].cpu().numpy()
            assert np.array_equal(bits(got), bits(want[k])), (what, k, int(np.sum(bits(got) != bits(want[k]))))

    out = fr.render_aov()  # allocates its own planes: the names and the bits
    names = world.kernels()
    assert names == [name], names
    same_as_model(out, geometry)
    if geometry != "ragged":
        return
    # the same frame through render_aov_pass into sentinel-filled planes between guards, then once more in the measured order
    guarded = {k: GuardedTiles(blocks, tile_size, ids=k == "ids") for k in ("shade", "normal", "albedo", "ids")}
    planes = {k: v.buf for k, v in guarded.items()}
    for what in ("ragged, one pass", "ragged, rebalanced"):
        assert fr.render_aov_pass(planes) == row["spp"]
        names = world.kernels()
        assert names == [name], names
        same_as_model(planes, what)
        for k, v in guarded.items():
            v.assert_rest_untouched(f"{what}, {k}")
        if what == "ragged, one pass":
            _rebalanced(fr)
            for v in guarded.values():
                v.refill()


def _box_exit(info, o, d):
    """slab exit of the scene's box in f64, padded (child boxes are rounded outward): at or above it a bounded query equals the
    unbounded one wherever t* lies below the bound (include/minipath_hip.h, consequence 4)"""
    lo, hi = np.array(list(info.bbox_min), np.float64), np.array(list(info.bbox_max), np.float64)
    dd = d.astype(np.float64)
    dd = dd / np.linalg.norm(dd, axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        a, c = (lo - o) / dd, (hi - o) / dd
    far = np.where(np.isnan(np.maximum(a, c)), np.inf, np.maximum(a, c)).min(axis=1)
    far = np.where(np.isfinite(far), far, 0.0)
    return (np.maximum(far, 0.0) * (1 + 1e-3) + 1e-2 * (1 + np.abs(hi - lo).max())).astype(F)


def _queries(world, name, row):
    import torch

    s = world.scene(row["scene"])
    gpu, info = s["gpu"], s["gpu"].info()
    o, d = meshes.random_rays(dc.N_RAYS, 23, np.array(list(info.bbox_min), F), np.array(list(info.bbox_max), F))
    t, prim, u, v, inst = s["orc"].trace_inst(o, d) if s["group"] else (*s["orc"].trace(o, d), np.zeros(o.shape[0], np.uint32))
    hit = prim != NO
    assert 0 < hit.sum() < hit.size, "hits and misses"
    if s["group"]:
        assert len(np.unique(inst[hit])) >= 2, "at least two members hit"
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()

    def same_as_oracle(got):
        got = {k: x.cpu().numpy() for k, x in got.items()}
        assert np.array_equal(got["prim"].view(np.uint32), prim) and np.array_equal(bits(got["t"]), bits(t))
        assert np.array_equal(bits(got["u"])[hit], bits(u)[hit]) and np.array_equal(bits(got["v"])[hit], bits(v)[hit])
        assert np.array_equal(got["instance"].view(np.uint32)[hit], inst[hit])

    if row["api"] == "trace":
        got = gpu.intersect(to, td, full=True)
        names = world.kernels()
        torch.cuda.synchronize()
        assert names == [name], names
        same_as_oracle(got)
        return
    # bounds at the padded box exit: exactly the oracle's unbounded record; bounds AT t*: a miss (strict t < b), nothing occluded
    exit_ = _box_exit(info, o, d)
    assert np.all(t[hit] < exit_[hit])
    at_hit = np.where(hit, t, F(1.0)).astype(F)
    for tm, level in ((exit_, "exit"), (at_hit, "t*")):
        tt = torch.from_numpy(tm).cuda()
        if row["api"] == "bounded":
            got = gpu.intersect(to, td, full=True, tmax=tt)
            names = world.kernels()
            torch.cuda.synchronize()
            assert names == [name], names
            if level == "exit":
                same_as_oracle(got)
            else:
                assert np.all(got["prim"].cpu().numpy().view(np.uint32)[hit] == NO) and np.all(got["t"].cpu().numpy()[hit] == FMAX)
        else:
            occ = gpu.occluded(to, td, tmax=tt)
            names = world.kernels()
            torch.cuda.synchronize()
            assert names == [name], names
            occ = occ.cpu().numpy().astype(bool)
            assert np.array_equal(occ, hit) if level == "exit" else not occ[hit].any()


def _generate_rays(world, name, row):
    import torch

    o, st = world.oracle, mp.RenderSettings(TS, row["spp"], RES, seed=SEED)
    smp = world.scene(row["scene"])["cam"].build_sampler(RES)
    blk = mp.ScreenBlock(30, 17, 41, 26)
    bufs = [torch.empty(blk.area(), dtype=torch.float32, device="cuda") for _ in range(6)]
    s, ss, osmp = smp.as_struct(), st.as_struct(), world.sampler(row["scene"], RES)
    for sample in (0, row["spp"] - 1):
        _lib.check(_lib.lib().mp_generate_rays(world.ctx.handle, C.byref(s), C.byref(ss), blk.as_struct(), sample, *[b.data_ptr() for b in bufs], None))
        names = world.kernels()
        torch.cuda.synchronize()
        assert names == [name], names
        g = np.stack([b.cpu().numpy() for b in bufs], axis=1)
        for i, (x, y) in enumerate(blk.internal_points()):
            r = o.sample_ray(osmp, x, y, o.lib().mpo_sample_key(C.c_uint64(SEED), RES[0], row["spp"], x, y, sample))
            assert np.array_equal(bits(g[i]), bits(np.array(list(r.o) + list(r.d), F))), (x, y, sample)
    assert len(np.unique(g, axis=0)) == blk.area()


def _untile(world, name, row):
    import torch

    s = world.scene(row["scene"])
    of, ou8, _ = world.expected(row["scene"], "render", RES, row["spp"])
    world.assert_not_vacuous(row["scene"], RES)
    fr = mp.FrameRenderer(mp.Scene(s["gpu"]), s["cam"], mp.RenderSettings(TS, row["spp"], RES, seed=SEED))
    fr.render()
    img, img8 = fr.untile()
    names = world.kernels()
    torch.cuda.synchronize()
    assert names == [name], names
    assert np.array_equal(bits(img.cpu().numpy()), bits(of)) and np.array_equal(img8.cpu().numpy(), ou8)


def _async(world, name, row):
    s = world.scene(row["scene"])
    of, ou8, _ = world.expected(row["scene"], "render", RES, row["spp"])
    world.assert_not_vacuous(row["scene"], RES)
    job = mp.render(mp.Scene(s["gpu"]), s["cam"], mp.RenderSettings(TS, row["spp"], RES, seed=SEED))
    job.wait()
    assert world.kernels() == list(row["also"]) + [name]  # every batch: the render kernel, then color_to_image on the device
    assert np.array_equal(bits(job.image_f32()), bits(of)) and np.array_equal(job.image(), ou8)
    job.close()


@pytest.mark.parametrize("key", list(dc.FACTS))
def test_scene_facts(world, key):
    """The live scene reports what dispatch_cases.FACTS records for it, so that the CPU plan tests size and select with the
    GPU's own numbers.  (tris_bounded / boxes_ordered are not reported: the kernel names of the cached rows and of the gate
    "triangle coordinates beyond 2^30" hold them.)"""
    want, s = dc.FACTS[key], world.scene(key)
    gpu, info = s["gpu"], s["gpu"].info()
    assert info.stack_bound == want["stack_bound"]
    assert ("sphere" in s) == (want["kind"] == 1) and s["group"] == (want["members"] != 0)
    if s["group"]:
        assert len(s["keep"][0]) == want["members"]
        assert info.stack_bound == max(m.info().stack_bound for m in s["keep"][0])
    if want["kind"] == 0 and not s["group"]:  # a tree of its own: the wide tree's nodes, the packets
        nodes = gpu.device_tree()[0]
        assert (len(nodes), info.packet_count) == (want["nodes"], want["packets"])
    else:  # no arrays of its own: the plans read 0 and 0
        assert (want["nodes"], want["packets"]) == (0, 0)
        with pytest.raises(mp.MinipathError):
            gpu.device_tree()


@pytest.mark.parametrize("name", list(dc.CASES))
def test_instantiation(world, name):
    row = dc.CASES[name]
    world.options(row)
    try:
        api = row["api"]
        if api in ("render", "paths"):
            _frame(world, row, [name])
        elif api == "wf":
            _frame(world, row, {name, *row["also"]})
        elif api == "aov":
            _aov(world, name, row)
        elif api in ("trace", "bounded", "occluded"):
            _queries(world, name, row)
        elif api == "rays":
            _generate_rays(world, name, row)
        elif api == "untile":
            _untile(world, name, row)
        else:
            _async(world, name, row)
    finally:
        world.options()


@pytest.mark.parametrize("guard", list(dc.GATES))
def test_mask_cache_gate(world, guard):
    """The mask cache is on and the sample count asks for it; the guard alone refuses: the uncached kernel is named."""
    expected, row = dc.GATES[guard]
    world.options(row)
    try:
        if guard != "the option off":
            assert {**dc.DEFAULTS, **row["opts"]}["packet_mask_cache"] == 1
        _frame(world, row, [expected])
    finally:
        world.options()


def _ragged_passes(world, which, geometry="grid"):
    import torch

    row, passes = dc.RAGGED[which]
    paths = row["api"] == "paths"
    world.options(row)
    try:
        s = world.scene(row["scene"])
        of, ou8, oseg = world.expected(row["scene"], row["api"], RES, row["spp"])
        world.assert_not_vacuous(row["scene"], RES)
        tile_size, blocks = tg.geometry(geometry, RES, TS)
        g = GuardedTiles(blocks, tile_size)
        fr = mp.FrameRenderer(mp.Scene(s["gpu"]), s["cam"], mp.RenderSettings(tile_size, row["spp"], RES, seed=SEED, max_depth=DEPTH if paths else 0),
                              tiles=None if geometry == "grid" else blocks, tile_buf=g.buf)
        assert fr.tiles == blocks
        nxt, seen, seg = 0, [], 0
        for n, _ in passes:
            nxt = fr.render_pass(nxt, n)
            seen += world.kernels()
            seg += int(fr.segments.item())
            # between passes: the running sums neither leak into the lanes outside a block nor come back from them
            g.assert_rest_untouched(f"after sample {nxt}")
        assert nxt == row["spp"]
        assert seen == [k for _, k in passes], seen
        img, img8 = fr.untile()
        torch.cuda.synchronize()
        assert np.array_equal(bits(img.cpu().numpy()), bits(of)) and np.array_equal(img8.cpu().numpy(), ou8)
        assert seg == (oseg if paths else RES[0] * RES[1] * row["spp"])
        if paths:
            assert seg > RES[0] * RES[1] * row["spp"]
    finally:
        world.options()


@pytest.mark.parametrize("which", list(dc.RAGGED))
def test_ragged_passes_select_by_the_pass(world, which):
    """One frame of 70 samples per pixel as MP_FLAG_ACCUMULATE passes of falling size: every pass is launched on the kernel its own
    sample count selects, and the finished frame is the oracle's single render."""
    _ragged_passes(world, which)


# ---- the same rows on tile lists that cut their pixel blocks ---------------------------------------------------------------------
@pytest.mark.parametrize("geometry", tg.GEOMETRIES)
@pytest.mark.parametrize("name", dc.tiled_rows())
def test_instantiation_on_cut_tiles(world, name, geometry):
    """Every render / paths / aov row and every configuration of the staged rows on tile_size 13, on one tile per pixel and on a
    partition into unaligned blocks (tests/tile_geometries.py; tests/test_tile_geometries_cpu.py shows that units are cut there and
    that the plans keep the row's names): the names, the oracle's frame bit for bit, the segments, and not one word of the
    sentinel-filled tile buffer changed outside the blocks; on the unaligned blocks once more in the hand-out order
    FrameRenderer.rebalance() measures."""
    row = dc.CASES[name]
    world.options(row)
    try:
        if row["api"] in ("render", "paths"):
            _frame(world, row, [name], geometry=geometry)
        elif row["api"] == "wf":
            _frame(world, row, {name, *row["also"]}, geometry=geometry)
        else:
            _aov(world, name, row, geometry=geometry)
    finally:
        world.options()


@pytest.mark.parametrize("geometry", ["grid13", "ragged"])
@pytest.mark.parametrize("which", list(dc.RAGGED))
def test_ragged_passes_on_cut_tiles(world, which, geometry):
    """The ragged MP_FLAG_ACCUMULATE passes over cut units: the kernels per pass, the oracle's frame, and between the passes the
    part of every slot that its block does not own still holds the sentinel."""
    _ragged_passes(world, which, geometry)


# ---- the staged pipeline over several tile batches and sample chunks -------------------------------------------------------------
@pytest.mark.parametrize("case", list(dc.STAGED_BATCHES))
def test_staged_pipeline_over_tile_batches(world, case):
    """26 tiles in 64 x 64 slots at 64 samples or more per pass: launch_render_paths_wavefront walks them in batches of 8, 8, 8 and
    2 (tests/test_tile_geometries_cpu.py holds that from the plan), each batch in sample chunks 64 + 6 -- tile_base > 0, the
    output slot tile_base + tile_l, the resets between batches, a shorter last batch, carry_in / finalize across batches and,
    with passes, the state an earlier pass left in the later batches' slots.  Against the oracle, and against the fused kernel."""
    import torch

    scene, spp, passes, chunked = dc.STAGED_BATCHES[case]
    world.options()
    s = world.scene(scene)
    tile_size, blocks = tg.geometry("ragged26", RES, TS)
    facts = dc.scene_facts(scene)
    plan = pp.plan(pp.STAGED, pp.launch(facts, len(blocks), tile_size, spp, max_depth=DEPTH, chunked=1 if chunked else 0))
    assert plan.rc == 0 and plan.tb < len(blocks) and plan.ws_bytes < 256 << 20, "the workspace of a batch: 192 MB today"
    of, ou8, oseg = world.expected(scene, "paths", RES, spp, chunked=chunked)
    world.assert_not_vacuous(scene, RES, of)
    staged_names = dc.staged_names(scene)
    results = {}
    for wavefront in (True, False):
        st = mp.RenderSettings(tile_size, spp, RES, seed=SEED, max_depth=DEPTH, wavefront=wavefront, chunked_sum=chunked)
        g = GuardedTiles(blocks, tile_size)
        fr = mp.FrameRenderer(mp.Scene(s["gpu"]), s["cam"], st, tiles=blocks, tile_buf=g.buf)
        nxt, seg = 0, 0
        for n in passes:
            if len(passes) == 1:  # one launch, without MP_FLAG_ACCUMULATE
                fr.render()
                nxt = spp
            else:
                nxt = fr.render_pass(nxt, n)
            names = world.kernels()
            seg += int(fr.segments.item())
            if wavefront:
                assert set(names) == staged_names and len(names) == len(staged_names), names
            else:
                assert len(names) == 1 and names[0].startswith("render_paths_"), names
            g.assert_rest_untouched(f"{'staged' if wavefront else 'fused'}, after sample {nxt}")
        assert nxt == spp
        img, img8 = fr.untile()
        torch.cuda.synchronize()
        results[wavefront] = (img.cpu().numpy(), img8.cpu().numpy(), seg, g.buf.cpu().numpy())
    for wavefront, (img, img8, seg, _) in results.items():
        what = "staged" if wavefront else "fused"
        assert np.array_equal(bits(img), bits(of)), f"{what}: {int(np.sum(bits(img) != bits(of)))} f32 values differ"
        assert np.array_equal(img8, ou8), what
        assert seg == oseg and seg > RES[0] * RES[1] * spp, what
    assert np.array_equal(bits(results[True][3]), bits(results[False][3])), "the staged and the fused tile buffers"
