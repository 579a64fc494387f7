"""CPU tests that pin the oracle's bounded closest-hit and occlusion walks (mpo_trace_rays_bounded, mpo_occluded_rays and the
sphere twins; W(b) of include/minipath_hip.h "Bounded and occlusion queries") before tests/test_gpu_ray_queries.py lets them judge
the kernels:
  * an unbounded bound gives the bits of the oracle's existing unbounded walk in every field;
  * the numpy model walk of tests/test_ray_queries_cpu.py -- a second, independent statement of the walk with a starting bound --
    gives the same t and hit/miss on the literal and on the wide tree;
  * the early-exit walk agrees with the bounded walk on hit/miss for every ray and bound, boundary values included;
  * the band fixture holds enough rays on which the walk differs from what the header's facts derive from the unbounded trace."""
import numpy as np
import pytest

from minipath_amd import scenes
from tests import meshes
from tests import ray_query_scenes as rq
from tests.ray_query_scenes import FMAX, FULL, NO, F, bits
from tests.test_device_tree_cpu import _host, _leaf_tris, _slots, _walk
from tests.test_ray_queries_cpu import MODEL_SCENES, _bounds, _max_entry, _model_rays, _walk_bounded

SPECIALS = np.array([0.0, -0.0, -1.0, np.nan, -np.inf, 1e-45, 3e-39], F)


@pytest.mark.parametrize("name", ["teapot", "sphere", "group", "instances"])
def test_unbounded_bound_gives_the_unbounded_walk(oracle, name):
    """tmax NULL, +inf and f32::MAX: the bits of mpo_trace_rays(_inst) in t, prim, u, v, instance on every ray, and of the
    per-ray mpo_bvh_intersect / mpo_sphere_intersect record in every field on every eighth ray; occluded == hit."""
    _, orc, o, d = rq.make(name, None, oracle)
    n = o.shape[0]
    t, prim, u, v, inst = orc.trace(o, d)
    hit = prim != NO
    assert 0.02 < hit.mean() < 0.98
    sub = np.arange(0, n, 8)
    ref = {k: np.zeros((sub.size, 3) if k in ("point", "normal", "tex") else sub.size, np.uint32 if k in ("prim", "material", "instance") else F)
           for k in FULL}
    ref["t"][:], ref["prim"][:] = FMAX, NO
    for j, i in enumerate(sub):
        h = orc.intersect(o[i], d[i])
        assert bool(h.hit) == bool(hit[i])
        if h.hit:
            ref["t"][j], ref["prim"][j], ref["u"][j], ref["v"][j] = h.t, h.prim, h.u, h.v
            ref["point"][j], ref["normal"][j], ref["tex"][j] = list(h.point), list(h.normal), list(h.tex)
            ref["material"][j], ref["instance"][j] = h.material, h.instance
    for tm in (None, np.inf, FMAX, np.full(n, np.inf, F), np.full(n, FMAX, F)):
        got = orc.trace_bounded(o, d, tm)
        for k, want in (("t", t), ("prim", prim), ("u", u), ("v", v), ("instance", inst)):
            assert np.array_equal(bits(got[k]), bits(want)), k
        for k in FULL:
            assert np.array_equal(bits(got[k][sub]), bits(ref[k])), k
        assert np.array_equal(orc.occluded(o, d, tm), hit)
    miss = ~hit
    for k in FULL:  # the miss record: f32::MAX, NO_PRIM and zeros
        want = FMAX.view(np.uint32) if k == "t" else NO if k == "prim" else 0
        assert np.all(bits(got[k][miss]) == want), k


def _oracle_leaf_tris(host, lit, oracle):
    """tests/test_ray_queries_cpu._tris with the reference's triangle arithmetic: the t of every triangle of a leaf from
    mpo_tri8_intersect (pinned by tests/test_oracle_known_answers.py) on the vertices as RelativePoint8::decompress gives them,
    +inf where the test or t >= 0 fails.  The numpy Moeller-Trumbore of _tris orders its operations differently and lands an ulp
    or two beside the reference's t; the model walk around it is what this module compares."""
    _, pk = _leaf_tris(host)
    leaf_box = {l: box for n in range(lit.shape[0]) for box, l in _slots(lit, n) if l & 63}
    cache = {}

    def tris_of(link, o, d):
        if link not in cache:
            first, nreal = link >> 6, link & 63
            box = leaf_box[link]
            mn, size = box[:3], (box[3:] - box[:3]).astype(F)
            rel = pk[first:first + (nreal + 7) // 8].astype(F) * (F(1) / F(65535))  # [packet, vertex, coordinate, lane]
            cache[link] = (np.float64(size)[None, None, :, None] * np.float64(rel) + np.float64(mn)[None, None, :, None]).astype(F)
        ray = oracle.Ray()
        ray.o[:], ray.d[:] = [float(x) for x in o], [float(x) for x in d]
        out = []
        for p in cache[link]:
            m, t, _, _ = oracle.tri8_intersect(*[np.ascontiguousarray(p[a]) for a in range(3)], ray)
            ok = np.array([(m >> i) & 1 for i in range(8)], bool) & (t >= 0)
            out.append(np.where(ok, t, np.inf).astype(F))
        return np.concatenate(out)[:link & 63]

    return tris_of


@pytest.mark.parametrize("name", MODEL_SCENES)
def test_model_walk_restates_the_oracle(oracle, name):
    """The scenes, the 120 rays and the bounds of test_bounded_model_walk_facts: the oracle's t and hit/miss equal the numpy
    model walk's on the literal and on the wide tree, for every bound; the early-exit walks of both agree as well."""
    host = _host(name)
    orc = oracle.Bvh.build(*(scenes.atrium(1, float(name.split(":")[1])) if name.startswith("atrium") else meshes.make(name)))
    wide, wroot, _, _ = host.device_tree()
    lit, lroot, _, _ = host.device_tree(literal=True)
    info = host.info()
    tris_of = _oracle_leaf_tris(host, lit, oracle)

    def tris_min(link, o, d):
        t = tris_of(link, o, d)
        return F(np.inf) if t.size == 0 else t.min()

    o, d = _model_rays(lit, np.array(list(info.bbox_min), F), np.array(list(info.bbox_max), F))
    hits = misses = 0
    for k in range(o.shape[0]):
        dk = np.array(list(oracle.ray_new(o[k], d[k]).d), F)  # Ray::new's direction: the model walks the ray the oracle walks
        _, tu, _ = _walk(lit, lroot, tris_min, o[k], dk)
        bs = np.array(_bounds(None if tu == FMAX else F(tu), _max_entry(lit, lroot, o[k], dk)), F)
        ok, dk_ = np.repeat(o[k:k + 1], bs.size, 0), np.repeat(d[k:k + 1], bs.size, 0)
        got, occ = orc.trace_bounded(ok, dk_, bs), orc.occluded(ok, dk_, bs)
        for j, b in enumerate(bs):
            want = None if got["prim"][j] == NO else got["t"][j]
            for nodes, root in ((lit, lroot), (wide, wroot)):
                _, t = _walk_bounded(nodes, root, tris_of, o[k], dk, b)
                assert t == want, (k, b, t, want)
            _, ta = _walk_bounded(lit, lroot, tris_of, o[k], dk, b, any_hit=True)
            assert (ta is not None) == bool(occ[j]), (k, b)
            hits += want is not None
            misses += want is None
    assert hits > 40 and misses > 100


def _identity_bounds(t, hit, rng):
    """per-ray bounds of the identity test: around t* for hits, finite values for misses, then every special value"""
    n = t.shape[0]
    ts = np.where(hit, t, F(1)).astype(F)
    up = lambda x, k: x if k == 0 else up(np.nextafter(x, F(np.inf)), k - 1)  # noqa: E731
    rounds = [ts * F(1 - 2**-8), ts, up(ts, 1), up(ts, 2), up(ts, 4), ts * F(1 + 2**-12), ts * F(1 + 2**-8), ts * F(2)]
    miss_vals = np.exp(rng.uniform(-3, 9, n)).astype(F)
    rounds = [np.where(hit, r, miss_vals).astype(F) for r in rounds]
    return rounds + [np.full(n, s, F) for s in SPECIALS]


@pytest.mark.parametrize("name", ["teapot", "soup_5000", "sphere", "group", "instances", "walls", "wall_group"])
def test_occlusion_walk_agrees_with_the_bounded_walk(oracle, name):
    """mpo_occluded_rays (a walk of its own) == (mpo_trace_rays_bounded prim != NO_PRIM) for every ray and bound: t*, nextafter(t*),
    0, -0, -1, NaN, -inf, 1e-45, 3e-39 and the band rays included.  Bounds that are not walked miss; a hit lies below its bound."""
    _, orc, o, d = rq.make(name, None, oracle)
    o, d = o[:6000], d[:6000]  # the band rays come first in the wall scenes' set
    unb = orc.trace_bounded(o, d)
    hit = unb["prim"] != NO
    n_hit = 0
    for tm in _identity_bounds(unb["t"], hit, np.random.default_rng(6)):
        got = orc.trace_bounded(o, d, tm)
        ghit = got["prim"] != NO
        assert np.array_equal(orc.occluded(o, d, tm), ghit), int((orc.occluded(o, d, tm) != ghit).sum())
        with np.errstate(invalid="ignore"):
            b = np.where(tm > 0, np.minimum(tm, FMAX), F(0))
        assert not ghit[~(unb["t"] < b) | ~hit].any()  # consequence 2, and the bounds that are not walked
        assert np.all(got["t"][ghit] < b[ghit]) and np.all(got["t"][~ghit] == FMAX)
        n_hit += int(ghit.sum())
    assert n_hit > 1000


@pytest.mark.parametrize("name", ["walls", "wall_group"])
def test_band_fixture(oracle, name):
    """The wall scene's rays hold at least 32 band rays -- rays with W(nextafter(t*)) != (t* < b ? the unbounded record : miss),
    by the oracle alone -- on its own and as a group's member.  This recipe finds 79 among 200 000 aimed rays and their grazing
    copies (66 aimed, 13 grazing); every one of them is a miss of W(nextafter(t*)).
    For every band ray the expectation derived from the facts (consequence 4's rule applied below its level) is NOT the walk's
    answer: that is why consequence 4 asks for b above every box's entry, and why only a W(b) oracle can judge these rays."""
    _, orc, o, d = rq.make(name, None, oracle)
    band, unb, w = rq.band_mask(orc, o, d)
    print(f"{name}: {int(band.sum())} band rays of {o.shape[0]}")
    assert band.sum() >= 32
    assert o.shape[0] - band.sum() >= rq.N_ORDINARY
    # the facts-derived expectation at b = nextafter(t*) is the unbounded record (t* < b); the walk's answer differs, field for field
    assert np.all(unb["prim"][band] != NO) and np.all(unb["t"][band] < np.nextafter(unb["t"][band], F(np.inf)))
    differs = np.zeros(int(band.sum()), bool)
    for f in FULL:
        differs |= (bits(w[f][band]) != bits(unb[f][band])).reshape(differs.size, -1).any(axis=1)
    assert differs.all()
    assert not orc.occluded(o[band], d[band], np.nextafter(unb["t"][band], F(np.inf)))[w["prim"][band] == NO].any()
