"""numpy restatement of include/minipath_lights.h, operation by operation in np.float32: the expectation of libminipath_lights.so's
kernels, which must give these bits, and of LocalLights' batch loop.  What does not depend on a random number is vectorised over the
pixels; the disc samples are calls of the oracle's RNG (oracle/pyoracle.py: mpo_sample_key, mpo_rng_seed, mpo_rng_unit_disc), one
stream per (pixel, sample) and one draw per sphere light from it, so size the cases at a few thousand rays.  dot, basis and bits
are those of tests/secondary_model.py, as the header says.  Runs under np.errstate(all="ignore"): NaN and infinite intermediates
are part of the definition (they fail the compares), not warnings.

Besides the rays generate() reports what happened to every pixel and every ray (`info`), which the tests use to show that their
inputs reach every rule."""
import ctypes as C

import numpy as np

from tests.secondary_model import F, basis, bits, dot  # noqa: F401  (bits is re-exported for the tests)

RAY_ARRAYS = ("ox", "oy", "oz", "dx", "dy", "dz", "tmax", "weight")
# info["pixel"][y, x]
P_NONE_ALPHA, P_NONE_NORMAL, P_LIVE = 0, 1, 3


def table(lights):
    """[L, 8] float32 rows {p.x, p.y, p.z, radius, i.r, i.g, i.b, reserved} of a sequence of (position, radius, intensity) or of
    such rows"""
    rows = []
    for lt in lights:
        rows.append(list(lt[0]) + [lt[1]] + list(lt[2]) + [0.0] if len(lt) == 3 else list(lt))
    return np.array(rows, F).reshape(-1, 8)


def disc_samples(po, seed, width, sample_count, x, y, s, count):
    """step 3: the first `count` UnitDisc samples of the stream seeded from the key of sample s of pixel (x, y): [count, 2]"""
    L = po.lib()
    key = L.mpo_sample_key(C.c_uint64(seed), width, sample_count, x, y, s)
    rng = po.Rng()
    L.mpo_rng_seed(C.byref(rng), C.c_uint64(key))
    uv = np.zeros((count, 2), F)
    for i in range(count):
        L.mpo_rng_unit_disc(C.byref(rng), po._f32p(uv[i]))
    return uv


def generate(po, position, normal, lights, seed, sample_count, sample_begin, batch, eye, bias=1e-4, margin=0.0, want_info=False):
    """mpl_generate: {ox, oy, oz, dx, dy, dz, tmax, weight}, float32 [batch * L * H * W] each, ray (b * L + l) * (H * W) + p"""
    position, normal, lights = np.asarray(position, F), np.asarray(normal, F), table(lights)
    h, w = position.shape[:2]
    L, pixels = len(lights), h * w
    eye = np.asarray(eye, F).reshape(3)
    bias, margin = F(bias), F(margin)
    with np.errstate(all="ignore"):
        A = position[..., 3]
        kind = np.full((h, w), P_LIVE, np.int32)
        kind[~(A > 0)] = P_NONE_ALPHA                                   # 1.
        P = (position[..., :3] / A[..., None]).astype(F)                # 2.
        N = normal[..., :3]
        l2 = dot(N, N)
        kind[(kind == P_LIVE) & ~(l2 > 0)] = P_NONE_NORMAL
        n = (N / np.sqrt(l2)[..., None]).astype(F)
        flipped = dot((P - eye).astype(F), n) > 0
        n = np.where(flipped[..., None], -n, n).astype(F)
        O = (P + n * bias).astype(F)
        live = kind == P_LIVE
        spheres = [l for l in range(L) if lights[l, 3] > 0]             # 3.
        uv = np.zeros((batch, L, h, w, 2), F)
        if spheres:
            for y, x in np.argwhere(live):
                for b in range(batch):
                    uv[b, spheres, y, x] = disc_samples(po, seed, w, sample_count, int(x), int(y), sample_begin + b, len(spheres))
        out = {k: np.zeros(batch * L * pixels, F) for k in RAY_ARRAYS}
        why = {k: np.zeros((batch, L, h, w), bool) for k in ("lit", "inside", "behind", "at", "short", "grazing")}
        zero = np.zeros((h, w), F)
        for b in range(batch):                                          # 4.
            for l in range(L):
                c, R = lights[l, :3], lights[l, 3]
                wv = (c - O).astype(F)
                q2 = dot(wv, wv)
                if R > 0:
                    inside = ~(q2 > R * R)
                    t, bt = basis((wv / np.sqrt(q2)[..., None]).astype(F))
                    ur, vr = (uv[b, l, ..., 0] * R).astype(F), (uv[b, l, ..., 1] * R).astype(F)
                    g = (c + (t * ur[..., None] + bt * vr[..., None])).astype(F)
                else:
                    inside = np.zeros((h, w), bool)
                    g = np.broadcast_to(c, (h, w, 3))
                d = (g - O).astype(F)
                dd = dot(d, d)
                ln = np.sqrt(dd).astype(F)
                nd = dot(n, d)
                reach = (ln - margin).astype(F)
                lit = live & ~inside & (nd > 0) & (dd > 0) & (reach > 0)
                weight = (nd / (dd * ln)).astype(F)
                s = slice((b * L + l) * pixels, (b * L + l + 1) * pixels)
                for k, v in (("ox", O[..., 0]), ("oy", O[..., 1]), ("oz", O[..., 2]), ("dx", d[..., 0]), ("dy", d[..., 1]), ("dz", d[..., 2]),
                             ("weight", weight)):
                    out[k][s] = np.where(lit, v, zero).reshape(-1)
                out["tmax"][s] = np.where(lit, reach, np.where(live, F(-1), F(0))).reshape(-1)
                why["lit"][b, l], why["inside"][b, l] = lit, live & inside
                ok = live & ~inside
                why["behind"][b, l], why["at"][b, l], why["short"][b, l] = ok & ~(nd > 0), ok & ~(dd > 0), ok & (dd > 0) & ~(reach > 0)
                why["grazing"][b, l] = lit & (nd < F(2.0 ** -126))  # lit at a cosine term that is a subnormal
    if want_info:
        return out, dict(why, pixel=kind, flipped=flipped & live, n=n, O=O, uv=uv)
    return out


def resolve(tmax, weight, occluded, lights, shape, batch, sums=None, want_out=True):
    """mpl_resolve for shape = (H, W): (sums, out or None); sums given = MPL_FLAG_ACCUMULATE from them"""
    h, w = shape
    lights = table(lights)
    L = len(lights)
    n = batch * L * h * w
    tmax = np.asarray(tmax, F).reshape(-1)[:n].reshape(batch, L, h, w)
    weight = np.asarray(weight, F).reshape(-1)[:n].reshape(batch, L, h, w)
    occluded = np.asarray(occluded, np.uint8).reshape(-1)[:n].reshape(batch, L, h, w)
    with np.errstate(all="ignore"):
        E, Cn = np.zeros((h, w, 3), F), np.zeros((h, w), F)
        if sums is not None:
            E, Cn = np.array(np.asarray(sums, F)[..., :3]), np.array(np.asarray(sums, F)[..., 3])
        for b in range(batch):
            t0 = tmax[b, 0]
            Cn = np.where((t0 > 0) | (t0 == F(-1)), Cn + F(1), Cn).astype(F)
            for l in range(L):
                seen = (tmax[b, l] > 0) & (occluded[b, l] == 0)
                for c in range(3):
                    E[..., c] = np.where(seen, E[..., c] + (lights[l, 4 + c] * weight[b, l]).astype(F), E[..., c])
        new = np.concatenate([E, Cn[..., None]], -1).astype(F)
        out = None
        if want_out:
            counted = Cn > 0
            out = np.concatenate([np.where(counted[..., None], E / Cn[..., None], F(0)), np.where(counted, F(1), F(0))[..., None]], -1).astype(F)
    return new, out


def rays_of(g):
    """(origins [n, 3], directions [n, 3], tmax [n]) of generate()'s arrays, for Bvh.occluded"""
    return np.stack([g["ox"], g["oy"], g["oz"]], -1), np.stack([g["dx"], g["dy"], g["dz"]], -1), g["tmax"]


def run(po, occluded_fn, position, normal, lights, seed, samples, batch, eye, want_rays=False, **kw):
    """LocalLights' batch loop: ceil(samples / batch) batches of generate -> occluded_fn(o, d, tmax) (the oracle's Bvh.occluded with
    a tmax per ray) -> resolve, continuing the sums from the second batch on, `out` from the last: (out, sums), and with want_rays
    {"tmax", "occluded"} [samples, L, H, W] of every ray as well"""
    h, w = np.asarray(position).shape[:2]
    L = len(table(lights))
    sums = out = None
    tms, occs = [], []
    for begin in range(0, samples, batch):
        n = min(batch, samples - begin)
        g = generate(po, position, normal, lights, seed, samples, begin, n, eye, **kw)
        o, d, tm = rays_of(g)
        # the query's own contract: a ray with tmax <= 0 is not walked and reports 0
        occ = np.asarray(occluded_fn(o, d, tm), np.uint8)
        sums, out = resolve(g["tmax"], g["weight"], occ, lights, (h, w), n, sums=sums, want_out=begin + n == samples)
        tms.append(g["tmax"].reshape(n, L, h, w))
        occs.append(occ.reshape(n, L, h, w))
    if want_rays:
        return out, sums, {"tmax": np.concatenate(tms), "occluded": np.concatenate(occs)}
    return out, sums
