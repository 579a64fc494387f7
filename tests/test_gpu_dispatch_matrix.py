"""GPU dispatch matrix (-m gpu): one case per kernel instantiation of tests/dispatch_cases.py (= every row of kernel_table.h, see
tests/test_dispatch_census_cpu.py).  Each case builds the smallest input that selects its instantiation, runs it through the
public API, asserts that mp_ctx_last_kernels names exactly that instantiation, and compares the result bit for bit with the
oracle's for the same input (never with another GPU run).  Then the gate cases -- the mask cache's guards must send a frame to the
UNCACHED kernel for the right reason -- and frames rendered as ragged MP_FLAG_ACCUMULATE passes, whose kernels follow the samples
of each pass."""
import ctypes as C

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib, scenes
from tests import aov_model, meshes
from tests import dispatch_cases as dc
from tests.conftest import TEAPOT

pytestmark = pytest.mark.gpu

F = np.float32
NO = 0xFFFFFFFF
FMAX = np.finfo(np.float32).max
SEED = 0x5EED
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
        self._scenes, self._renders, self._facts = {}, {}, {}

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

    def expected(self, key, kind, res, spp):
        """the oracle's frame: (f32, u8, ray segments or None); kind "render" or "paths"; cached"""
        k = (key, kind, res, spp)
        if k not in self._renders:
            s, smp = self.scene(key), self.sampler(key, res)
            if "sphere" in s:
                assert kind == "render"
                f, u8 = self.oracle.render_tile_sphere(*s["sphere"], smp, res[0], spp, SEED, 0, 0, res[0], res[1])
                self._renders[k] = (f, u8, None)
            elif kind == "render":
                f, u8, *_ = s["orc"].render_image_mt(smp, res[0], res[1], spp, SEED, TS, 16)
                self._renders[k] = (f, u8, None)
            else:
                f, u8, _, seg = s["orc"].render_image_paths_mt(smp, res[0], res[1], spp, SEED, DEPTH, TS, 16)
                self._renders[k] = (f, u8, seg)
        return self._renders[k]

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


def _frame(world, row, expect, res=RES):
    """render / paths / wf rows: one frame through FrameRenderer, the names reported, the frame against the oracle"""
    import torch

    s = world.scene(row["scene"])
    paths = row["api"] in ("paths", "wf")
    st = mp.RenderSettings(TS, row["spp"], res, seed=SEED, traversal=row["traversal"], max_depth=DEPTH if paths else 0, wavefront=row["api"] == "wf")
    of, ou8, oseg = world.expected(row["scene"], "paths" if paths else "render", res, row["spp"])
    world.assert_not_vacuous(row["scene"], res, of)
    if "sphere" not in s:
        _stack_in_lds(world, row)
    fr = mp.FrameRenderer(mp.Scene(s["gpu"]), s["cam"], st)
    fr.render()
    names = world.kernels()
    img, img8 = fr.untile()
    torch.cuda.synchronize()
    if isinstance(expect, set):
        assert set(names) == expect and len(names) == len(expect), names
    else:
        assert names == expect, names
    got = img.cpu().numpy()
    assert np.array_equal(bits(got), bits(of)), f"{int(np.sum(bits(got) != bits(of)))} f32 values differ"
    assert np.array_equal(img8.cpu().numpy(), ou8)
    seg = int(fr.segments.item())
    if paths:
        assert seg == oseg and seg > res[0] * res[1] * row["spp"], "paths bounce: more segments than camera rays"
    else:
        assert seg == res[0] * res[1] * row["spp"]


def _aov(world, name, row):
    import torch

    s = world.scene(row["scene"])
    _stack_in_lds(world, row)
    want = aov_model.planes(world.oracle, s["orc"].intersect, world.sampler(row["scene"], AOV_RES), AOV_RES[0], row["spp"], SEED,
                            (0, 0, AOV_RES[0], AOV_RES[1]), s["table"])
    hits = want["ids"][..., 3]
    assert 0 < hits.sum() < hits.size, "the view must hold hits and misses"
    if s["group"]:
        assert len(np.unique(want["ids"][..., 1][hits == 1])) >= 2, "at least two members in view"
        assert len(np.unique(want["albedo"][..., :3].reshape(-1, 3)[hits.reshape(-1) == 1], axis=0)) >= 2, "at least two colours in view"
    fr = mp.FrameRenderer(mp.Scene(s["gpu"]), s["cam"], mp.RenderSettings(AOV_TS, row["spp"], AOV_RES, seed=SEED))
    out = fr.render_aov()
    names = world.kernels()
    img = {k: fr.untile_plane(v) for k, v in out.items()}
    torch.cuda.synchronize()
    assert names == [name], names
    for k in ("shade", "normal", "albedo", "ids"):
        got = img[k].cpu().numpy()
        assert np.array_equal(bits(got), bits(want[k])), (k, int(np.sum(bits(got) != bits(want[k]))))


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


@pytest.mark.parametrize("which", list(dc.RAGGED))
def test_ragged_passes_select_by_the_pass(world, which):
    """One frame of 70 samples per pixel as MP_FLAG_ACCUMULATE passes of falling size: every pass is launched on the kernel its own
    sample count selects, and the finished frame is the oracle's single render."""
    import torch

    row, passes = dc.RAGGED[which]
    paths = row["api"] == "paths"
    world.options(row)
    try:
        s = world.scene(row["scene"])
        of, ou8, oseg = world.expected(row["scene"], row["api"], RES, row["spp"])
        world.assert_not_vacuous(row["scene"], RES)
        fr = mp.FrameRenderer(mp.Scene(s["gpu"]), s["cam"], mp.RenderSettings(TS, row["spp"], RES, seed=SEED, max_depth=DEPTH if paths else 0))
        nxt, seen, seg = 0, [], 0
        for n, _ in passes:
            nxt = fr.render_pass(nxt, n)
            seen += world.kernels()
            seg += int(fr.segments.item())
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
