"""Scenes and rays of the ray-query tests (tests/test_ray_queries_oracle_cpu.py, tests/test_gpu_ray_queries.py): every scene as a
product object and as its oracle twin, built from ONE definition, with the rays the tests send through both.  The product object
is host-only where no context is given (it then serves for mp_scene_info alone).  Also the band fixture: the rays on which a bounded
walk differs from what the facts of include/minipath_hip.h ("Bounded and occlusion queries") would derive from the unbounded walk."""
import functools

import numpy as np

import minipath_amd as mp
from minipath_amd import scenes
from tests import meshes
from tests.conftest import TEAPOT

F = np.float32
FMAX = np.finfo(F).max
NO = 0xFFFFFFFF
MESHES = ["soup_300", "soup_5000", "grid_40", "sphere_24", "flat_plane", "two_clusters", "sliver_fan"]
SCENES = ["teapot", "atrium"] + MESHES + ["sphere", "group", "instances"]
FULL = ("t", "prim", "u", "v", "point", "normal", "tex", "material", "instance")  # mp_hits_soa
WALLS = "walls_600"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class OracleScene:
    """The oracle's side of a scene: a Bvh (plain, instanced or a group) or a plain Sphere given as (center, radius)."""

    def __init__(self, oracle, bvh=None, sphere=None, keep=()):
        self.oracle, self.bvh, self.sphere, self._keep = oracle, bvh, sphere, keep

    def intersect(self, o, d):
        """one ray through mpo_bvh_intersect / mpo_sphere_intersect: the Hit record"""
        ray = self.oracle.ray_new(o, d)
        return self.oracle.sphere_intersect(*self.sphere, ray) if self.sphere else self.bvh.intersect(ray)

    def trace(self, o, d):
        """the unbounded batch trace: t, prim, u, v, instance"""
        if self.sphere is None:
            return self.bvh.trace_inst(o, d)
        n = o.shape[0]
        t, prim = np.full(n, FMAX, F), np.full(n, NO, np.uint32)
        for i in range(n):
            h = self.intersect(o[i], d[i])
            if h.hit:
                t[i], prim[i] = h.t, 0
        return t, prim, np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.uint32)

    def trace_bounded(self, o, d, tmax=None):
        if self.sphere is None:
            return self.bvh.trace_bounded(o, d, tmax)
        return self.oracle.sphere_trace_bounded(*self.sphere, o, d, tmax)

    def occluded(self, o, d, tmax=None):
        if self.sphere is None:
            return self.bvh.occluded(o, d, tmax)
        return self.oracle.sphere_occluded(*self.sphere, o, d, tmax)


def _quats(rng, n):
    q = rng.standard_normal((n, 4)).astype(F)
    q /= np.sqrt((q.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(F)
    q[0] = (0.0, 0.0, 0.0, 1.0)
    return q.astype(F)


def _camera_rays(oracle, n, seed):
    s = oracle.build_sampler(oracle.teapot_camera(), 256, 256)
    rng = np.random.default_rng(seed)
    o, d = np.zeros((n, 3), F), np.zeros((n, 3), F)
    for i in range(n):
        r = oracle.sample_ray(s, int(rng.integers(0, 256)), int(rng.integers(0, 256)), 77 + i)
        o[i], d[i] = list(r.o), list(r.d)
    return o, d


def _box(scene):
    i = scene.info()
    return np.array(list(i.bbox_min), F), np.array(list(i.bbox_max), F)


def make(name, ctx, oracle):
    """(product scene object -- on the GPU of ctx, host-only for ctx None --, OracleScene, rays o, d)"""
    if name == "teapot":
        gpu, orc = mp.TriangleBvh.with_obj(TEAPOT, ctx), oracle.Bvh.from_obj(TEAPOT)
        o1, d1 = meshes.random_rays(12000, 31, *orc.bbox())
        o2, d2 = _camera_rays(oracle, 4000, 5)
        return gpu, OracleScene(oracle, orc), np.concatenate([o1, o2]), np.concatenate([d1, d2])
    if name == "atrium" or name in MESHES:
        pos, nrm, tex, tri = scenes.atrium(1, 0.05) if name == "atrium" else meshes.make(name)
        gpu, orc = mp.TriangleBvh.build(pos, nrm, tex, tri, ctx), oracle.Bvh.build(pos, nrm, tex, tri)
        bmin, bmax = orc.bbox()
        o, d = meshes.random_rays(16000, 41, bmin, np.maximum(bmax, bmin + 1e-3))
        # and rays aimed at triangle centroids: hits on sparse scenes too
        rng = np.random.default_rng(42)
        c = pos[tri[rng.integers(0, tri.shape[0], 4000)]].mean(axis=1).astype(F)
        d[-4000:] = (c - o[-4000:]).astype(F)
        return gpu, OracleScene(oracle, orc), o, d
    if name == "sphere":
        c, r = (1.0, 2.0, 3.0), 1.5
        o, d = meshes.random_rays(3000, 43, np.array(c, F) - r, np.array(c, F) + r)
        return mp.Sphere(c, r, ctx), OracleScene(oracle, sphere=(c, r)), o, d
    if name == "group":
        rng = np.random.default_rng(19)
        pos, nrm, tex, tri = meshes.make("soup_300")
        teapot, soup, ball = mp.TriangleBvh.with_obj(TEAPOT, ctx), mp.TriangleBvh.build(pos, nrm, tex, tri, ctx), mp.Sphere((0.4, 0, 0), 1.0, ctx)
        o_teapot, o_soup = oracle.Bvh.from_obj(TEAPOT), oracle.Bvh.build(pos, nrm, tex, tri)
        tr = np.array([[0, 0, 0], [7.0, 0.5, -2.0], [-5.5, 2.0, 1.0], [0.0, 5.0, -1.0], [3.0, 4.5, 2.5]], F)
        q = _quats(rng, 5)
        gpu = mp.ObjectGroup([teapot, teapot, soup, ball, soup], tr, rotations=q)
        box = oracle.Bvh.from_obj(TEAPOT)
        box.set_group([box, o_teapot, o_soup, ((0.4, 0.0, 0.0), 1.0), o_soup], tr, rotations=q)
        gpu._keep = (teapot, soup, ball)
        o, d = meshes.random_rays(16000, 23, *_box(gpu))
        return gpu, OracleScene(oracle, box, keep=(o_teapot, o_soup)), o, d
    if name == "instances":
        base = mp.TriangleBvh.with_obj(TEAPOT, ctx)
        tr = np.array([[0, 0, 0], [7.5, 0, -3], [-7.0, 0.5, -6], [0.25, 3.4, -1.0]], F)
        gpu = mp.Instances(base, tr)
        orc = oracle.Bvh.from_obj(TEAPOT)
        orc.set_instances(tr)
        o, d = meshes.random_rays(16000, 4, *_box(gpu))
        return gpu, OracleScene(oracle, orc), o, d
    if name in ("walls", "wall_group"):
        # the wall scene on its own, and as the first member (identity transform: its rays reach it unchanged) of a two-member
        # rotated group; the rays are the band fixture's
        pos, nrm, tex, tri = meshes.make(WALLS)
        o, d = (a.copy() for a in band_candidates(oracle))
        if name == "walls":
            return mp.TriangleBvh.build(pos, nrm, tex, tri, ctx), OracleScene(oracle, _walls_bvh(oracle)), o, d
        spos, snrm, stex, stri = meshes.make("soup_300")
        walls, soup = mp.TriangleBvh.build(pos, nrm, tex, tri, ctx), mp.TriangleBvh.build(spos, snrm, stex, stri, ctx)
        tr = np.array([[0, 0, 0], [9.0, 0.5, -2.0]], F)
        q = _quats(np.random.default_rng(20), 2)
        gpu = mp.ObjectGroup([walls, soup], tr, rotations=q)
        gpu._keep = (walls, soup)
        o_walls, o_soup = oracle.Bvh.build(pos, nrm, tex, tri), oracle.Bvh.build(spos, snrm, stex, stri)
        o_walls.set_group([o_walls, o_soup], tr, rotations=q)
        return gpu, OracleScene(oracle, o_walls, keep=(o_soup,)), o, d
    raise KeyError(name)


# ---- the band fixture ---------------------------------------------------------------------------------------------------------
N_CANDIDATES = 200_000  # aimed rays searched; the grazing copies of those that still hit are searched too
N_ORDINARY = 4000


@functools.lru_cache(maxsize=None)
def _walls_bvh(oracle):
    return oracle.Bvh.build(*meshes.make(WALLS))


def band_mask(orc, o, d):
    """Rays whose walk with b = nextafter(t*) is NOT what consequence 4's rule (t* < b ? the unbounded record : miss) gives,
    established by the oracle alone.  Returns (mask, the unbounded records, the records of W(nextafter(t*)))."""
    unb = orc.trace_bounded(o, d)
    hit = unb["prim"] != NO
    with np.errstate(over="ignore"):
        b = np.where(hit, np.nextafter(unb["t"], F(np.inf)), F(1)).astype(F)
    w = orc.trace_bounded(o, d, b)
    differs = np.zeros(o.shape[0], bool)
    for k in FULL:
        differs |= (bits(w[k]) != bits(unb[k])).reshape(o.shape[0], -1).any(axis=1)
    return hit & differs, unb, w


@functools.lru_cache(maxsize=None)
def band_candidates(oracle):
    """Rays of the wall scene: every band ray found among N_CANDIDATES rays aimed at triangle centroids from random_rays' origins
    and among their grazing copies (one direction component scaled by 1e-4), then N_ORDINARY ordinary rays of both kinds."""
    orc = OracleScene(oracle, _walls_bvh(oracle))
    pos, _, _, tri = meshes.make(WALLS)
    o, _ = meshes.random_rays(N_CANDIDATES, 51, *orc.bvh.bbox())
    rng = np.random.default_rng(52)
    c = pos[tri[rng.integers(0, tri.shape[0], N_CANDIDATES)]].astype(np.float64).mean(axis=1).astype(F)
    d = (c - o).astype(F)
    g = d.copy()
    g[np.arange(N_CANDIDATES), rng.integers(0, 3, N_CANDIDATES)] *= F(1e-4)
    aimed, _, _ = band_mask(orc, o, d)
    grazing, _, _ = band_mask(orc, o, g)
    h = N_ORDINARY // 2
    oo = np.concatenate([o[aimed], o[grazing], o[:h], o[h:2 * h]])
    dd = np.concatenate([d[aimed], g[grazing], d[:h], g[h:2 * h]])
    oo.setflags(write=False)
    dd.setflags(write=False)
    return oo, dd


# ---- secondary rays -----------------------------------------------------------------------------------------------------------
PATH_EPS = F(1e-4)  # the path extension's offset along the normal


def secondary_rays(orc, o, d, light, seed):
    """Shadow and bounce rays off the hit points of primary rays (o, d), as a path tracer starts them: origin = HitRecord.point +
    1e-4 * the normal, flipped towards the incoming ray.  Returns {set name: (o, d, tmax)}: "shadow" -- un-normalised directions
    to the point `light`, tmax = dist * (1 - 1e-4) in units of the NORMALISED ray (Ray::new normalises) --, "bounce2" and
    "bounce005" -- uniformly random directions, tmax = 2 and 0.05."""
    rec = orc.trace_bounded(o, d)
    hit = rec["prim"] != NO
    p, n = rec["point"][hit], rec["normal"][hit].copy()
    n[(d[hit] * n).sum(axis=1) > 0] *= F(-1)
    so = (p + n * PATH_EPS).astype(F)
    to_light = (np.asarray(light, F) - so).astype(F)
    dist = np.linalg.norm(to_light.astype(np.float64), axis=1)
    rng = np.random.default_rng(seed)
    bd = rng.standard_normal(so.shape).astype(F)
    m = so.shape[0]
    return {"shadow": (so, to_light, (dist * (1 - 1e-4)).astype(F)),
            "bounce2": (so, bd, np.full(m, 2.0, F)),
            "bounce005": (so, bd, np.full(m, 0.05, F))}


# scene -> the point light of its shadow rays (inside the atrium's hall, outside the teapot, above the height field, ...)
SECONDARY = {"teapot": (4.0, 6.0, 5.0), "grid_40": (0.5, 1.5, 0.3), "atrium": (0.0, 9.0, 0.0), "walls": (6.0, 6.0, 6.0),
             "group": (2.0, 8.0, 3.0)}


def primary_rays(name, orc, o, d):
    """about 8 000 primary rays of scene `name` (o, d = make()'s rays), most of which hit"""
    if name == "atrium":  # from inside the hall: from outside every hit point lies on the outer face of a wall
        rng = np.random.default_rng(7)
        o = (np.array([0, 7, 0], F) + (rng.random((8000, 3), dtype=F) - F(0.5)) * np.array([30, 10, 12], F)).astype(F)
        return o, rng.standard_normal((8000, 3)).astype(F)
    if name == "walls":
        return meshes.random_rays(8000, 61, *orc.bvh.bbox())
    if name == "group":  # one ray in six hits
        return o, d
    return o[-8000:], d[-8000:]
