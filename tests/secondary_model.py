"""numpy restatement of include/minipath_secondary.h, operation by operation in np.float32: the expectation of
libminipath_secondary.so's kernels, which must give these bits, and of SecondaryVisibility's batch loop.  What a pixel alone decides
is vectorised over the pixels; the disc sample is one call of the oracle's RNG per ray (oracle/pyoracle.py: mpo_sample_key,
mpo_rng_seed, mpo_rng_unit_disc), so size the cases at a few thousand rays.  Runs under np.errstate(all="ignore"): NaN and infinite
intermediates are part of the definition (they fail the compares), not warnings.

Besides the rays generate() reports what happened to every pixel (`info`), which the tests use to show that their inputs reach
every rule."""
import ctypes as C

import numpy as np

F = np.float32
MODE_AO, MODE_SUN = 0, 1
RAY_ARRAYS = ("ox", "oy", "oz", "dx", "dy", "dz", "tmax")
# info["pixel"][y, x]
P_NONE_ALPHA, P_NONE_NORMAL, P_UNLIT, P_LIVE = 0, 1, 2, 3


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def dot(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F)


def basis(m):
    """the header's basis(m) for m [..., 3]: (t, bt)"""
    m = np.asarray(m, F)
    mx, my, mz = m[..., 0], m[..., 1], m[..., 2]
    sg = np.copysign(F(1), mz).astype(F)
    a = (F(-1) / (sg + mz)).astype(F)
    bb = ((mx * my) * a).astype(F)
    t = np.stack([F(1) + ((sg * mx) * mx) * a, sg * bb, -sg * mx], -1).astype(F)
    bt = np.stack([bb, sg + (my * my) * a, -my], -1).astype(F)
    return t, bt


def disc_sample(po, seed, width, sample_count, x, y, s):
    """step 3: the key of sample s of pixel (x, y) and the UnitDisc sample of the stream seeded from it"""
    L = po.lib()
    key = L.mpo_sample_key(C.c_uint64(seed), width, sample_count, x, y, s)
    rng = po.Rng()
    L.mpo_rng_seed(C.byref(rng), C.c_uint64(key))
    uv = np.zeros(2, F)
    L.mpo_rng_unit_disc(C.byref(rng), po._f32p(uv))
    return key, uv


def generate(po, position, normal, mode, seed, sample_count, sample_begin, batch, eye, light=(0, 0, 1), radius=1.0, bias=1e-4,
             spread=0.0, want_info=False):
    """mps_generate: {ox, oy, oz, dx, dy, dz, tmax}, float32 [batch * H * W] each, sample-major"""
    position, normal = np.asarray(position, F), np.asarray(normal, F)
    h, w = position.shape[:2]
    eye, light = np.asarray(eye, F).reshape(3), np.asarray(light, F).reshape(3)
    radius, bias, spread = F(radius), F(bias), F(spread)
    with np.errstate(all="ignore"):
        A = position[..., 3]
        kind = np.full((h, w), P_LIVE, np.int32)
        kind[~(A > 0)] = P_NONE_ALPHA                                   # 1.
        P = (position[..., :3] / A[..., None]).astype(F)                # 2.
        N = normal[..., :3]
        l2 = dot(N, N)
        kind[(kind == P_LIVE) & ~(l2 > 0)] = P_NONE_NORMAL
        n = (N / np.sqrt(l2)[..., None]).astype(F)
        wv = (P - eye).astype(F)
        flipped = dot(wv, n) > 0
        n = np.where(flipped[..., None], -n, n).astype(F)
        if mode == MODE_SUN:                                            # 5.
            kind[(kind == P_LIVE) & ~(dot(n, np.broadcast_to(light, n.shape)) > 0)] = P_UNLIT
            t, bt = basis(np.broadcast_to(light, n.shape))
        else:
            t, bt = basis(n)
        O = (P + n * bias).astype(F)
        pixels = h * w
        out = {k: np.zeros(batch * pixels, F) for k in RAY_ARRAYS}
        uvs = np.zeros((batch, h, w, 2), F)
        for y in range(h):
            for x in range(w):
                p = y * w + x
                if kind[y, x] != P_LIVE:
                    if kind[y, x] == P_UNLIT:
                        out["tmax"][p::pixels] = F(-1)
                    continue
                for b in range(batch):
                    r = b * pixels + p
                    _, (u, v) = disc_sample(po, seed, w, sample_count, x, y, sample_begin + b)
                    uvs[b, y, x] = (u, v)
                    if mode == MODE_SUN:
                        us, vs = F(u * spread), F(v * spread)
                        d = ((t[y, x] * us + bt[y, x] * vs) + light).astype(F)
                    else:                                               # 4.
                        z = np.sqrt(F(F(1) - F(F(u * u) + F(v * v))))
                        d = ((t[y, x] * u + bt[y, x] * v) + n[y, x] * z).astype(F)
                    out["ox"][r], out["oy"][r], out["oz"][r] = O[y, x]
                    out["dx"][r], out["dy"][r], out["dz"][r] = d
                    out["tmax"][r] = radius
    if want_info:
        return out, {"pixel": kind, "flipped": flipped & ((kind == P_LIVE) | (kind == P_UNLIT)), "n": n, "P": P, "uv": uvs}
    return out


def resolve(tmax, occluded, shape, batch, counts=None, want_out=True):
    """mps_resolve for shape = (H, W): (counts, out or None); counts given = MPS_FLAG_ACCUMULATE onto them"""
    h, w = shape
    pixels = h * w
    tmax = np.asarray(tmax, F).reshape(-1)[:batch * pixels].reshape(batch, h, w)
    occluded = np.asarray(occluded, np.uint8).reshape(-1)[:batch * pixels].reshape(batch, h, w)
    with np.errstate(all="ignore"):
        V, Cn = np.zeros((h, w), F), np.zeros((h, w), F)
        for b in range(batch):
            traced = tmax[b] > 0
            unlit = ~traced & (tmax[b] == F(-1))
            Cn = np.where(traced | unlit, Cn + F(1), Cn).astype(F)
            V = np.where(traced & (occluded[b] == 0), V + F(1), V).astype(F)
        if counts is not None:
            V = (np.asarray(counts, F)[..., 0] + V).astype(F)
            Cn = (np.asarray(counts, F)[..., 1] + Cn).astype(F)
        new = np.stack([V, Cn, np.zeros((h, w), F), np.zeros((h, w), F)], -1).astype(F)
        out = None
        if want_out:
            a = np.where(Cn > 0, V / Cn, F(1)).astype(F)
            out = np.stack([a, a, a, np.where(Cn > 0, F(1), F(0))], -1).astype(F)
    return new, out


def rays_of(g):
    """(origins [n, 3], directions [n, 3], tmax [n]) of generate()'s arrays, for Bvh.occluded"""
    return np.stack([g["ox"], g["oy"], g["oz"]], -1), np.stack([g["dx"], g["dy"], g["dz"]], -1), g["tmax"]


def run(po, occluded_fn, position, normal, mode, seed, samples, batch, eye, **kw):
    """SecondaryVisibility's batch loop: ceil(samples / batch) batches of generate -> occluded_fn(o, d, tmax) (the oracle's
    Bvh.occluded, W(b) of include/minipath_hip.h) -> resolve, accumulating from the second batch on, `out` from the last:
    (out, counts)"""
    h, w = np.asarray(position).shape[:2]
    counts = out = None
    for begin in range(0, samples, batch):
        n = min(batch, samples - begin)
        g = generate(po, position, normal, mode, seed, samples, begin, n, eye, **kw)
        o, d, tm = rays_of(g)
        # the query's own contract: a ray with tmax <= 0 is not walked and reports 0; +inf is clamped by the query
        occ = np.asarray(occluded_fn(o, d, tm), np.uint8)
        counts, out = resolve(g["tmax"], occ, (h, w), n, counts=counts, want_out=begin + n == samples)
    return out, counts
