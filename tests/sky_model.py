"""numpy restatement of include/minipath_sky.h, operation by operation in np.float32: the expectation of libminipath_sky.so's
kernels, which must give these bits, and of SkyLight's batch loop over tests/secondary_model.py (the rays) and the oracle's occlusion
query.  Everything is vectorised over the pixels or the directions.  Runs under np.errstate(all="ignore"): NaN and infinite
intermediates are part of the definition (they fail the compares), not warnings.

lookup() also reports where every direction went (`info`), which the tests use to show that their inputs reach every rule."""
import numpy as np

from tests import secondary_model as sm
from tests.secondary_model import F, bits  # noqa: F401  (bits is re-exported for the tests)

# the order of (d.x, d.y, d.z) that is (m.x, m.y, m.z), by pole
POLE_ORDER = {2: (0, 1, 2), 1: (2, 0, 1), 0: (1, 2, 0)}


def to_map(d, pole):
    """m of a direction d [..., 3]"""
    return np.asarray(d, F)[..., POLE_ORDER[pole]]


def from_map(m, pole):
    """the direction whose m is given: the inverse of to_map"""
    d = np.empty_like(np.asarray(m, F))
    d[..., POLE_ORDER[pole]] = np.asarray(m, F)
    return d


def fold(px, py):
    """the fold of the lower hemisphere, both from the old values"""
    return np.copysign(F(1) - np.abs(py), px).astype(F), np.copysign(F(1) - np.abs(px), py).astype(F)


def taps(u, n):
    """one axis of step 2: (i0, i1, w) of u for a map of n texels"""
    nf = F(n)
    f = (u * nf - F(0.5)).astype(F)
    f = np.where(f > 0, f, F(0)).astype(F)
    top = F(nf - F(1))
    f = np.where(f < top, f, top).astype(F)
    fl = np.floor(f)
    i0 = fl.astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, (f - fl).astype(F)


def lookup(env, d, pole, want_info=False):
    """L(d) [n, 3] of directions d [n, 3] in the map env [N, N, 4]"""
    env, d = np.asarray(env, F), np.asarray(d, F).reshape(-1, 3)
    n = env.shape[0]
    with np.errstate(all="ignore"):
        m = to_map(d, pole)
        l1 = ((np.abs(m[:, 0]) + np.abs(m[:, 1])) + np.abs(m[:, 2])).astype(F)
        ok = (l1 > 0) & (l1 < F(np.inf))
        px, py = (m[:, 0] / l1).astype(F), (m[:, 1] / l1).astype(F)
        folded = m[:, 2] < 0
        qx, qy = fold(px, py)
        px, py = np.where(folded, qx, px), np.where(folded, qy, py)
        u, v = (px * F(0.5) + F(0.5)).astype(F), (py * F(0.5) + F(0.5)).astype(F)
        x0, x1, wx = taps(u, n)
        y0, y1, wy = taps(v, n)
        T = env[..., :3]
        ax, ay = (F(1) - wx)[:, None], (F(1) - wy)[:, None]
        top = (T[y0, x0] * ax + T[y0, x1] * wx[:, None]).astype(F)
        bot = (T[y1, x0] * ax + T[y1, x1] * wx[:, None]).astype(F)
        L = (top * ay + bot * wy[:, None]).astype(F)
        L = np.where(ok[:, None], L, F(0)).astype(F)
    if want_info:
        return L, dict(ok=ok, folded=folded & ok, x0=x0, x1=x1, y0=y0, y1=y1, wx=wx, wy=wy, u=u, v=v, l1=l1)
    return L


def resolve(env, dx, dy, dz, tmax, occluded, shape, batch, pole, sums=None, want_out=True):
    """mpe_resolve for shape = (H, W): (sums, out or None); sums given = MPE_FLAG_ACCUMULATE from them"""
    h, w = shape
    n = batch * h * w
    d = np.stack([np.asarray(a, F).reshape(-1)[:n] for a in (dx, dy, dz)], -1)
    tmax = np.asarray(tmax, F).reshape(-1)[:n].reshape(batch, h, w)
    occluded = np.asarray(occluded, np.uint8).reshape(-1)[:n].reshape(batch, h, w)
    L = lookup(env, d, pole).reshape(batch, h, w, 3)
    with np.errstate(all="ignore"):
        E, Cn = np.zeros((h, w, 3), F), np.zeros((h, w), F)
        if sums is not None:
            E, Cn = np.array(np.asarray(sums, F)[..., :3]), np.array(np.asarray(sums, F)[..., 3])
        for b in range(batch):
            t = tmax[b]
            Cn = np.where((t > 0) | (t == F(-1)), Cn + F(1), Cn).astype(F)
            looked = (t > 0) & (occluded[b] == 0)
            E = np.where(looked[..., None], E + L[b], E).astype(F)
        new = np.concatenate([E, Cn[..., None]], -1).astype(F)
        out = None
        if want_out:
            counted = Cn > 0
            out = np.concatenate([np.where(counted[..., None], E / Cn[..., None], F(0)), np.where(counted, F(1), F(0))[..., None]], -1).astype(F)
    return new, out


def texel_directions(n):
    """(m [n, n, 3], z < 0 [n, n]) of mpe_fill_gradient: the direction, in the map's frame, of the centre of every texel T[j][i]"""
    nf = F(n)
    c = (((np.arange(n, dtype=F) + F(0.5)) / nf).astype(F) * F(2) - F(1)).astype(F)
    px, py = np.broadcast_to(c[None, :], (n, n)), np.broadcast_to(c[:, None], (n, n))
    z = ((F(1) - np.abs(px)) - np.abs(py)).astype(F)
    qx, qy = fold(px, py)
    lower = z < 0
    return np.stack([np.where(lower, qx, px), np.where(lower, qy, py), z], -1).astype(F), lower


def fill_gradient(n, zenith, horizon, ground):
    """mpe_fill_gradient: the map [n, n, 4]"""
    zenith, horizon, ground = (np.asarray(c, F).reshape(3) for c in (zenith, horizon, ground))
    with np.errstate(all="ignore"):
        m, _ = texel_directions(n)
        px, py, z = m[..., 0], m[..., 1], m[..., 2]
        ln = np.sqrt(((px * px + py * py) + z * z).astype(F)).astype(F)
        hgt = (z / ln).astype(F)
        up = (horizon + ((zenith - horizon).astype(F) * hgt[..., None]).astype(F)).astype(F)
        c = np.where((hgt >= 0)[..., None], up, ground).astype(F)
    return np.concatenate([c, np.ones((n, n, 1), F)], -1).astype(F)


def run(po, occluded_fn, position, normal, env, seed, samples, batch, eye, pole=1, radius=float("inf"), bias=1e-4, visibility=False,
        want_rays=False):
    """SkyLight's batch loop: ceil(samples / batch) batches of secondary_model.generate (MODE_AO) -> occluded_fn(o, d, tmax) (the
    oracle's Bvh.occluded) -> resolve, continuing the sums from the second batch on, `out` from the last: (out, sums); with
    visibility (out, sums, ao, counts), the last two from secondary_model.resolve on the same answers; with want_rays a dict
    {"d" [samples, H, W, 3], "tmax", "occluded" [samples, H, W]} of every ray is appended"""
    h, w = np.asarray(position).shape[:2]
    sums = out = counts = ao = None
    ds, tms, occs = [], [], []
    for begin in range(0, samples, batch):
        n = min(batch, samples - begin)
        last = begin + n == samples
        g = sm.generate(po, position, normal, sm.MODE_AO, seed, samples, begin, n, eye, radius=radius, bias=bias)
        o, d, tm = sm.rays_of(g)
        occ = np.asarray(occluded_fn(o, d, tm), np.uint8)
        sums, out = resolve(env, g["dx"], g["dy"], g["dz"], g["tmax"], occ, (h, w), n, pole, sums=sums, want_out=last)
        if visibility:
            counts, ao = sm.resolve(g["tmax"], occ, (h, w), n, counts=counts, want_out=last)
        ds.append(d.reshape(n, h, w, 3))
        tms.append(g["tmax"].reshape(n, h, w))
        occs.append(occ.reshape(n, h, w))
    res = (out, sums, ao, counts) if visibility else (out, sums)
    if want_rays:
        res += ({"d": np.concatenate(ds), "tmax": np.concatenate(tms), "occluded": np.concatenate(occs)},)
    return res
