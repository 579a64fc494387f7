"""GPU tests of the tie rule inside a triangle packet (-m gpu): triangles are taken in (packet, lane) order and replace the best
hit on a strict `t < best.t` (ray_bvh_intersection.rs:104-140, :59), so of two triangles of one packet with the same t the lower
lane wins.  Every walk on the device implements that rule on its own -- the 8-lane group walk's cross-lane minimum and lane pick,
the packet walks' running compare, the cached walk's triangle masks -- and ordinary meshes almost never tie.  The scenes here do:
meshes.doubled holds every triangle twice, and in about half of all hits the twin sits in the packet of the hit and ties in t, u
and v bit for bit (tests/test_exact_ties_cpu.py measures the share and proves the ties); meshes.stack is one triangle 2, 8, 9 and
16 times over.  The copies carry different materials, so the winner shows in HitRecord.prim / material, in the ids and albedo
feature planes, and in every bounce-mode frame.  All comparisons are against the oracle, on u32 views, zero differing words."""
import numpy as np
import pytest

import minipath_amd as mp
from tests import aov_model
from tests import dispatch_cases as dc
from tests import tie_model as tm

pytestmark = pytest.mark.gpu

F = np.float32
NO = tm.NO
FMAX = np.finfo(F).max
HIT_FIELDS = ("t", "prim", "u", "v", "point", "normal", "tex", "material", "instance")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class World:
    """The context, every tie scene (GPU object and oracle twin, built once), the oracle's hit records, planes and frames."""

    def __init__(self, oracle):
        import torch

        assert torch.cuda.is_available(), "gpu tests need a GPU"
        self.oracle, self.ctx = oracle, mp.Context(0)
        self._scenes, self._records, self._planes, self._frames, self._twins = {}, {}, {}, {}, {}

    def options(self, row=None):
        for k, v in {**dc.DEFAULTS, **(row["opts"] if row else {})}.items():
            self.ctx.set_option(k, v)

    def scene(self, name, which="copy", group=False):
        """{"gpu", "orc", "keep"} of a tie scene with tri_material = copy_id ("copy") or source % 3; group: {it, it shifted}"""
        k = (name, which, group)
        if k not in self._scenes:
            pos, nrm, tex, tri, *_ = tm.arrays(name)
            gpu = mp.TriangleBvh.build(pos, nrm, tex, tri, self.ctx, tri_material=tm.material_ids(name, which))
            keep = (gpu,)
            if group:
                gpu = mp.ObjectGroup([gpu, gpu], tm.group_translations())
            self._scenes[k] = {"gpu": gpu, "orc": tm.oracle_scene(self.oracle, name, which, group), "keep": keep, "group": group}
        return self._scenes[k]

    def materials(self, s, table):
        s["gpu"].set_materials(table, tm.SKY)
        s["orc"].set_materials(table, tm.SKY)

    def tied(self, name, prim):
        """mask: hits whose twin sits in the hit packet (doubled meshes; the slots do not depend on the materials)"""
        if name not in self._twins:
            self._twins[name] = tm.twin_slots(tm.oracle_scene(self.oracle, name, "source"))[1]
        return tm.tied(prim, self._twins[name])

    def records(self, name, which, group):
        """the rays of the scene, rolled so that a short call starts on hits, and the oracle's full hit record of each"""
        k = (name, which, group)
        if k not in self._records:
            s, po = self.scene(name, which, group), self.oracle
            plain = self.scene(name, which, False)["orc"]
            o, d = tm.rays(name, plain)
            if group:  # the second half of the rays aimed at the shifted member
                o[1::2] += np.array(tm.GROUP_SHIFT, F)
            n = o.shape[0]
            rec = {"t": np.full(n, FMAX, F), "prim": np.full(n, NO, np.uint32), "u": np.zeros(n, F), "v": np.zeros(n, F), "point": np.zeros((n, 3), F),
                   "normal": np.zeros((n, 3), F), "tex": np.zeros((n, 3), F), "material": np.zeros(n, np.uint32), "instance": np.zeros(n, np.uint32)}
            for i in range(n):
                h = s["orc"].intersect(po.ray_new(o[i], d[i]))
                if h.hit:
                    rec["t"][i], rec["prim"][i], rec["u"][i], rec["v"][i] = h.t, h.prim & 0xFFFFFFFF, h.u, h.v
                    rec["point"][i], rec["normal"][i], rec["tex"][i] = list(h.point), list(h.normal), list(h.tex)
                    rec["material"][i], rec["instance"][i] = h.material, h.instance
            # the oracle's batch trace agrees with its per-ray records
            t, prim, *_ = s["orc"].trace_inst(o, d) if group else s["orc"].trace(o, d)
            assert np.array_equal(prim, rec["prim"]) and np.array_equal(bits(t), bits(rec["t"]))
            # short calls (1 ray, 65 rays) start at a tied hit outside lane 0 where the scene has one, else at a hit
            hit = rec["prim"] != NO
            want = (self.tied(name, rec["prim"]) & ((rec["prim"] & 7) != 0)) if name in tm.DOUBLED else hit
            first = int(np.argmax(want)) if want.any() else int(np.argmax(hit))
            roll = lambda a: np.ascontiguousarray(np.roll(a, -first, axis=0))  # noqa: E731
            self._records[k] = (roll(o), roll(d), {f: roll(a) for f, a in rec.items()})
        return self._records[k]

    def planes(self, name, which, group, table, spp):
        k = (name, which, group, id(table), spp)
        if k not in self._planes:
            s = self.scene(name, which, group)
            self.materials(s, table)
            self._planes[k] = aov_model.planes(self.oracle, s["orc"].intersect, tm.sampler(self.oracle, group), tm.RES[0], spp, tm.SEED,
                                               (0, 0, *tm.RES), table)
        return self._planes[k]

    def frame(self, name, group, table, spp, depth):
        """the oracle's frame (f32, u8, ray segments or None)"""
        k = (name, group, id(table), spp, depth)
        if k not in self._frames:
            s, smp = self.scene(name, "copy", group), tm.sampler(self.oracle, group)
            self.materials(s, table)
            if depth:
                f, u8, _, seg = s["orc"].render_image_paths_mt(smp, *tm.RES, spp, tm.SEED, depth, tm.TS, 16)
            else:
                (f, u8, *_), seg = s["orc"].render_image_mt(smp, *tm.RES, spp, tm.SEED, tm.TS, 16), None
            self._frames[k] = (f, u8, seg)
        return self._frames[k]


@pytest.fixture(scope="module")
def world(oracle):
    w = World(oracle)
    yield w
    w.options()


def _cuda(*a):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def _host(out):
    import torch

    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_record(got, rec, sel=slice(None)):
    for f in HIT_FIELDS:
        diff = int(np.sum(bits(got[f])[sel] != bits(rec[f])[sel]))
        assert diff == 0, (f, diff)


# every tie scene alone; the doubled meshes also as members of a group and with tri_material = source % 3
QUERY_SCENES = [(n, "copy", False) for n in tm.names()] + [(n, "copy", True) for n in tm.DOUBLED] + [(n, "source%3", False) for n in tm.DOUBLED]
_ids = [f"{n}{'+group' if g else ''}{'' if w == 'copy' else '/' + w}" for n, w, g in QUERY_SCENES]


@pytest.mark.parametrize("n", [1, 65, 4096])
@pytest.mark.parametrize("scene", QUERY_SCENES, ids=_ids)
def test_ray_queries_resolve_ties_to_the_lower_lane(world, scene, n):
    """mp_trace_rays: the oracle's full hit record.  mp_trace_rays_bounded / mp_occluded_rays with the bound AT t*: a miss, not
    occluded (strict t < b; the twin at the same t must not pass either); at the next float up and at 2 t*: the unbounded
    record -- the lower lane again, although both candidates now pass the bound -- and occluded."""
    name, which, group = scene
    s = world.scene(name, which, group)
    o, d, rec = world.records(name, which, group)
    if n == tm.N_RAYS:
        n = o.shape[0]  # a stack: the grid through its triangle and the random rays
    o, d, rec = o[:n], d[:n], {f: a[:n] for f, a in rec.items()}
    hit = rec["prim"] != NO
    assert hit[0], "short calls start on a hit"
    if n >= tm.N_RAYS:
        assert 50 <= hit.sum() < n, "hits and misses"
        if name in tm.DOUBLED:
            tied = world.tied(name, rec["prim"])
            assert tied.sum() >= tm.MIN_TIED_SHARE * hit.sum() and np.mean((rec["prim"][tied] & 7) != 0) >= 0.5, "ties, and not in lane 0"
            assert len(np.unique(rec["material"][tied])) >= 2
        if group:
            assert len(np.unique(rec["instance"][hit])) == 2, "both members hit"
    elif name in tm.DOUBLED:
        assert world.tied(name, rec["prim"][:1])[0] and rec["prim"][0] & 7, "short calls start on a tie outside lane 0"
    obj = str(group).lower()
    to, td = _cuda(o, d)
    got = _host(s["gpu"].intersect(to, td, full=True))
    assert dc.launched(world.ctx) == [f"trace_rays_kernel<{obj}>"]
    _same_record(got, rec)
    at = np.where(hit, rec["t"], F(1.0)).astype(F)
    for level, tmax in (("t*", at), ("next", np.nextafter(at, F(np.inf))), ("2 t*", at * F(2))):
        (tt,) = _cuda(tmax.astype(F))
        got = _host(s["gpu"].intersect(to, td, full=True, tmax=tt))
        assert dc.launched(world.ctx) == [f"query_rays_kernel<{obj}, kBounded>"]
        occ = s["gpu"].occluded(to, td, tmax=tt).cpu().numpy().astype(bool)
        assert dc.launched(world.ctx) == [f"query_rays_kernel<{obj}, kAnyHit>"]
        if level == "t*":
            assert np.all(got["prim"].view(np.uint32)[hit] == NO) and np.all(got["t"][hit] == FMAX), level
            assert not occ[hit].any(), level
        else:
            _same_record(got, rec, hit)
            assert np.array_equal(occ[hit], hit[hit]), level
        assert np.all(got["prim"].view(np.uint32)[~hit] == NO) and not occ[~hit].any()


def _aov_table(which, rgb):
    return (tm.RGB3 if rgb else tm.GREY3) if which == "source%3" else (tm.RGB if rgb else tm.GREY)


AOV = [(k, m, "copy") for m in tm.AOV_MESHES for k in tm.AOV_CASES] + [
    # the three-entry coloured table over tri_material = source % 3: the twins share a material, prim alone shows the winner
    (k, "grid_40", "source%3") for k in ("render_aov_packet_kernel<4, false, 8, false, true>", "render_aov_packet_kernel<16, false, 6, true>")]


@pytest.mark.parametrize("key,mesh,which", AOV, ids=[f"{k}-{m}{'' if w == 'copy' else '/' + w}" for k, m, w in AOV])
def test_feature_planes_show_the_lower_lane(world, key, mesh, which):
    """render_aov ids (prim, member, material of sample 0) and albedo (the mean over the samples of the winner's reflectance)
    against tests/aov_model.py over the oracle, on every feature-plane walk: cached, uncached at 1, 4 and 16 in flight, LDS
    stack, object group.  Under the checker table the albedo also depends on the winner's texture coordinates."""
    import torch

    row = tm.AOV_CASES[key]
    group = "group" in row["scene"]
    table = _aov_table(which, True)
    s = world.scene(mesh, which, group)
    want = world.planes(mesh, which, group, table, row["spp"])
    ids = want["ids"].reshape(-1, 4)
    hit = ids[:, 3] == 1
    assert 0 < hit.sum() < hit.size, "hits and misses"
    member = ids[:, 1] if group else np.zeros_like(ids[:, 1])
    assert not group or len(np.unique(member[hit])) == 2, "both members in view"
    tied = world.tied(mesh, np.where(hit, ids[:, 0], NO).astype(np.uint32))
    assert tied.sum() >= 0.25 * hit.sum() and np.mean((ids[tied, 0] & 7) != 0) >= 0.5, "ties in view, and not in lane 0"
    if which == "copy":
        assert len(np.unique(ids[tied, 2])) == 2, "winners of both materials"
    world.materials(s, table)
    world.options(row)
    try:
        assert s["keep"][0].info().stack_bound > tm.LDS_REGS
        fr = mp.FrameRenderer(mp.Scene(s["gpu"]), tm.camera(group), mp.RenderSettings(tm.TS, row["spp"], tm.RES, seed=tm.SEED))
        out = fr.render_aov()
        names = dc.launched(world.ctx)
        img = {k: fr.untile_plane(out[k]).cpu().numpy() for k in ("ids", "albedo")}
        torch.cuda.synchronize()
    finally:
        world.options()
    assert names == [key], names
    for k in ("ids", "albedo"):
        diff = int(np.sum(bits(img[k]) != bits(want[k])))
        assert diff == 0, (k, diff)


def _render(world, key, row, mesh, depth):
    """one frame through FrameRenderer: the names reported, the frame and the segment count against the oracle"""
    import torch

    group, rgb = "group" in row["scene"], row["scene"].endswith("+rgb")
    table = tm.RGB if rgb else tm.GREY
    s = world.scene(mesh, "copy", group)
    of, ou8, oseg = world.frame(mesh, group, table, row["spp"], depth)
    alpha = of[..., 3]
    assert alpha.max() == 1.0 and alpha.min() < 1.0, "hits and misses in view"
    world.materials(s, table)
    world.options(row)
    try:
        st = mp.RenderSettings(tm.TS, row["spp"], tm.RES, seed=tm.SEED, traversal=row["traversal"], max_depth=depth, wavefront=row["api"] == "wf")
        fr = mp.FrameRenderer(mp.Scene(s["gpu"]), tm.camera(group), st)
        fr.render()
        names = dc.launched(world.ctx)
        img, img8 = fr.untile()
        torch.cuda.synchronize()
    finally:
        world.options()
    want = tm.expected_names(key, row)
    assert set(names) == want and len(names) == len(want), names
    got = img.cpu().numpy()
    assert np.array_equal(bits(got), bits(of)), f"{int(np.sum(bits(got) != bits(of)))} f32 values differ"
    assert np.array_equal(img8.cpu().numpy(), ou8)
    seg, rays = int(fr.segments.item()), tm.RES[0] * tm.RES[1] * row["spp"]
    if depth:
        assert seg == oseg and seg > rays, "paths bounce: more segments than camera rays"
    else:
        assert seg == rays


PATHS = [(k, m) for m in tm.PATH_MESHES for k in tm.PATH_CASES]


@pytest.mark.parametrize("key,mesh", PATHS, ids=[f"{k}-{m}" for k, m in PATHS])
def test_bounce_frames_shade_the_lower_lane(world, key, mesh):
    """Depth-3 frames under tables whose two copies differ (copy 0: albedo 0.2, no emission; copy 1: albedo 0.9, emission 2.5;
    the coloured table has the same contrast and a checker): the material at every hit sets the path's throughput and emission,
    so a walk that resolved a tie to the other copy renders another frame (tests/test_exact_ties_cpu.py: 41 to 76 % of the pixels).
    The fused kernel at 1, 2, 4 and 8 in flight, its cached camera pass, the object-group forms, the pooled kernels, the staged
    pipeline: frame, 8-bit image and segment count against render_image_paths_mt."""
    _render(world, key, tm.PATH_CASES[key], mesh, tm.DEPTH)


RENDERS = [(k, m) for m in tm.RENDER_MESHES for k in tm.RENDER_CASES]


@pytest.mark.parametrize("key,mesh", RENDERS, ids=[f"{k}-{m}" for k, m in RENDERS])
def test_depth_0_frames_on_tie_heavy_packets(world, key, mesh):
    """NOT tie-order coverage: two coincident triangles shade the same |d.n|, so a depth-0 frame cannot show which one won.  One
    frame per packet family (cached, uncached with the stack in registers and in LDS, two rays per lane, the 8-lane group walk,
    the object-group walk) sends packets full of equal pairs through the triangle masks and the wave-level early-outs, where two
    equal candidates are the case in which tri_may_hit's strict comparisons matter: a mask that dropped both, or a reject that
    fired on the pair, would lose the hit and show here."""
    _render(world, key, tm.RENDER_CASES[key], mesh, 0)
