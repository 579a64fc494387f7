"""numpy restatement of the filter of include/minipath_denoise.h, operation by operation in np.float32: the expectation of
libminipath_denoise.so's kernels, which must give these bits.  Vectorised over the pixels, a loop over the 25 taps in the header's
order (dy outer, dx inner), every sum taken in that order from +0.0.  Runs under np.errstate(all="ignore"): NaN and infinite
intermediates are part of the definition (a NaN weight is +0), not warnings."""
import numpy as np

F = np.float32
H5 = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))
FLAG_DEMODULATE_ALBEDO = 1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def mx(a, b):
    """the header's max(a, b) = a > b ? a : b with b the constant: b for NaN, +0 for max(-0, 0)"""
    return np.where(a > F(b), a, F(b)).astype(F)


def _windows(n, off):
    """slices (p, q) of the positions p in [0, n) whose tap q = p + off is in [0, n); None if there are none"""
    lo, hi = max(0, -off), min(n, n - off)
    if lo >= hi:
        return None
    return slice(lo, hi), slice(lo + off, hi + off)


def one_pass(C, N, V, s, k, sigma_depth, sigma_luminance):
    """C_i, V_i (None without variance) -> C_{i+1}, V_{i+1} at step s"""
    h, w = C.shape[:2]
    hit = C[..., 3] != 0  # NaN alpha is a hit
    sw = np.zeros((h, w), F)
    sc = np.zeros((h, w, 3), F)
    sv = np.zeros((h, w), F)
    lum = ((C[..., 0] + C[..., 1]) + C[..., 2]).astype(F)
    sd = F(sigma_depth) * F(s)
    if V is not None:
        den = (F(sigma_luminance) * np.sqrt(mx(V[..., 0], 0)) + F(1e-6)).astype(F)
    else:
        den = np.full((h, w), F(sigma_luminance), F)
    for dy in range(-2, 3):
        wy = _windows(h, s * dy)
        for dx in range(-2, 3):
            wx = _windows(w, s * dx)
            if wy is None or wx is None:
                continue  # every such tap is outside the image
            p, q = (wy[0], wx[0]), (wy[1], wx[1])
            hw = F(H5[dx + 2] * H5[dy + 2])
            if dx == 0 and dy == 0:
                wt = np.full(sw[p].shape, hw, F)
            else:
                Np, Nq = N[p], N[q]
                d = ((Np[..., 0] * Nq[..., 0] + Np[..., 1] * Nq[..., 1]) + Np[..., 2] * Nq[..., 2]).astype(F)
                wn = mx(d, 0)
                for _ in range(k):
                    wn = (wn * wn).astype(F)
                a = (np.abs(Np[..., 3] - Nq[..., 3]) / sd).astype(F)
                wz = (F(1) / (F(1) + a * a)).astype(F)
                b = (np.abs(lum[p] - lum[q]) / den[p]).astype(F)
                wl = (F(1) / (F(1) + b * b)).astype(F)
                wt = (((hw * wn) * wz) * wl).astype(F)
                wt = np.where(np.isnan(wt), F(0), wt).astype(F)
            use = hit[p] & hit[q] & (wt != 0)  # a miss is never read as a tap; a zero weight adds nothing
            Cq = C[q]
            sw[p] = np.where(use, sw[p] + wt, sw[p])
            for c in range(3):
                sc[p + (c,)] = np.where(use, sc[p + (c,)] + wt * Cq[..., c], sc[p + (c,)])
            if V is not None:
                sv[p] = np.where(use, sv[p] + (wt * wt) * V[q][..., 0], sv[p])
    out = C.copy()
    for c in range(3):
        out[..., c] = np.where(hit, sc[..., c] / sw, C[..., c])
    Vn = None
    if V is not None:
        Vn = np.zeros_like(V)
        Vn[..., 0] = np.where(hit, sv / (sw * sw), V[..., 0])
    return out.astype(F), Vn


def atrous(color, normal_depth, albedo=None, variance=None, iterations=5, k=7, sigma_depth=1.0, sigma_luminance=1.0, demodulate=False):
    """mpd_atrous on host arrays [h, w, 4] float32: out, or (out, variance_out) with a variance plane"""
    with np.errstate(all="ignore"):
        C = np.array(color, F, copy=True)
        N = np.asarray(normal_depth, F)
        V = None if variance is None else np.array(variance, F, copy=True)
        hit = C[..., 3] != 0
        if demodulate:
            f = mx(np.asarray(albedo, F)[..., :3], 1e-3)
            for c in range(3):
                C[..., c] = np.where(hit, C[..., c] / f[..., c], C[..., c])
        for i in range(iterations):
            C, V = one_pass(C, N, V, 1 << i, int(k), sigma_depth, sigma_luminance)
        if demodulate:
            for c in range(3):
                C[..., c] = np.where(hit, C[..., c] * f[..., c], C[..., c])
        if V is None:
            return C
        V[..., 1:] = 0
        return C, V


def variance_from_moments(shade, shade_sq, sample_count):
    """mpd_variance_from_moments: {v, 0, 0, 0}"""
    with np.errstate(all="ignore"):
        shade, shade_sq = np.asarray(shade, F), np.asarray(shade_sq, F)
        alpha = shade[..., 3]
        m = (shade[..., 0] / alpha).astype(F)
        q = (shade_sq[..., 0] / alpha).astype(F)
        v = (mx(q - m * m, 0) / (F(sample_count) * alpha)).astype(F)
        out = np.zeros(shade.shape, F)
        out[..., 0] = np.where(alpha != 0, v, F(0))
        return out


def synthetic(w, h, seed):
    """Seeded test planes [h, w, 4]: colour (about 10 % misses with alpha 0 and a huge colour that must never be read, some partial
    alphas), normal + depth (unit normals around 4 directions in cells of 3 x 2 pixels, depths around 3 layers, some NaN normals),
    albedo (some zeros and tiny values, below the 1e-3 floor) and variance (some zeros, a few negatives)."""
    rng = np.random.default_rng(seed)
    dirs = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 1, 0], [-0.48, 0.6, 0.64]], np.float64)
    cell = rng.integers(0, 4, ((h + 1) // 2, (w + 2) // 3))
    which = np.repeat(np.repeat(cell, 2, 0), 3, 1)[:h, :w]
    n = dirs[which] + rng.normal(0, 0.05, (h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    layer = np.array([1.0, 1.5, 4.0])[rng.integers(0, 3, ((h + 3) // 4, (w + 4) // 5))]
    t = np.repeat(np.repeat(layer, 4, 0), 5, 1)[:h, :w] + rng.normal(0, 0.02, (h, w))
    nd = np.concatenate([n, t[..., None]], -1).astype(F)
    nd[rng.random((h, w)) < 0.03, :3] = np.nan
    color = rng.random((h, w, 4)).astype(F)
    color[..., 3] = np.where(rng.random((h, w)) < 0.15, F(0.5), F(1))
    miss = rng.random((h, w)) < 0.10
    color[miss] = (F(3e30), F(-3e30), F(1e38), F(0))
    albedo = rng.random((h, w, 4)).astype(F)
    albedo[rng.random((h, w)) < 0.05, 0] = 0
    albedo[rng.random((h, w)) < 0.05, 1] = F(1e-5)
    var = np.zeros((h, w, 4), F)
    var[..., 0] = (rng.random((h, w)) * 0.01).astype(F)
    var[rng.random((h, w)) < 0.10, 0] = 0
    var[rng.random((h, w)) < 0.03, 0] = F(-1e-3)
    var[..., 1:] = F(7)  # never read
    return {"color": color, "normal": nd, "albedo": albedo, "variance": var}
