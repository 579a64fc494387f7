"""numpy restatement of include/minipath_resample.h, operation by operation in np.float32: the expectation of
libminipath_resample.so's kernels, which must give these bits.  downsample() walks the blocks in Python (a few thousand pixels);
upsample() is vectorised over the full pixels, one pass per tap, and has no tiles: whatever it gives does not depend on where a
16 x 16 tile of the kernel begins.  Runs under np.errstate(all="ignore"): NaN and infinite intermediates are part of the definition
(they fail the compares), not warnings.

Besides the planes both report what happened to every pixel (`info`), which the tests use to show that their inputs reach every
rule.  upsample(dtype=np.float64) evaluates the same text in binary64 for the error bound of tests/test_resample_cpu.py."""
import numpy as np

F = np.float32
PICK_PHASE, PICK_NEAREST = 0, 1
PICK_NONE = 0xFFFFFFFF
MAX_PLANES = 4


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def low_size(W, H, f):
    return (W + f - 1) // f, (H + f - 1) // f


def valid(position, normal):
    """the header's VALID, per pixel"""
    with np.errstate(all="ignore"):
        N = np.asarray(normal, F)[..., :3]
        return (np.asarray(position, F)[..., 3] > 0) & (dot(N, N).astype(F) > 0)


def downsample(position, normal, sources, f, pick_mode=PICK_PHASE, phase=0, want_info=False):
    """mpr_downsample: (picks u32 [h, w], [destination planes, the dtype of their sources]).  info["how"][Y, X]: 0 no pick, 1 the
    phase candidate, 2 the scan after an invalid or outside candidate, 3 nearest; info["replaced"]: the times NEAREST's pick changed
    after the first; info["ties"]: valid pixels whose depth equalled the best and lost; info["nan_first"]: a NaN depth was picked"""
    position, normal = np.asarray(position, F), np.asarray(normal, F)
    H, W = position.shape[:2]
    w, h = low_size(W, H, f)
    ok = valid(position, normal)
    with np.errstate(all="ignore"):
        depth = (normal[..., 3] / position[..., 3]).astype(F)
    picks = np.full((h, w), PICK_NONE, np.uint32)
    how, replaced, ties, nan_first = (np.zeros((h, w), np.int32) for _ in range(4))
    for Y in range(h):
        for X in range(w):
            xs, ys = range(f * X, min(f * X + f, W)), range(f * Y, min(f * Y + f, H))
            best = None
            if pick_mode == PICK_PHASE:
                cx, cy = f * X + phase % f, f * Y + phase // f
                if cx < W and cy < H and ok[cy, cx]:
                    best, how[Y, X] = (cx, cy), 1
                else:
                    for y in ys:
                        for x in xs:
                            if best is None and ok[y, x]:
                                best, how[Y, X] = (x, y), 2
            else:
                d_best = None
                for y in ys:
                    for x in xs:
                        if not ok[y, x]:
                            continue
                        if best is None or depth[y, x] < d_best:
                            replaced[Y, X] += best is not None
                            best, d_best, how[Y, X] = (x, y), depth[y, x], 3
                        elif depth[y, x] == d_best:
                            ties[Y, X] += 1
                nan_first[Y, X] = best is not None and np.isnan(d_best)
            if best is not None:
                picks[Y, X] = best[1] * W + best[0]
    out = []
    for s in sources:
        s = np.ascontiguousarray(s)
        assert s.shape == (H, W, 4) and s.dtype.itemsize == 4
        d = np.zeros((h, w, 4), s.dtype)
        have = picks != PICK_NONE
        d[have] = s.reshape(-1, 4)[picks[have]]
        out.append(d)
    if want_info:
        return picks, out, {"how": how, "replaced": replaced, "ties": ties, "nan_first": nan_first}
    return picks, out


def upsample(position, normal, position_lo, normal_lo, picks, color_lo, f, k, sigma_plane, want_info=False, dtype=F):
    """mpr_upsample: out [H, W, 4].  info: "used" = taps with w != 0, "live" = taps not skipped, "wn0" = live taps with wn == 0,
    "wp_half" = live taps with wp < 1/2, "how" = 0 a zero pixel of step 1 or 2, 1 the weighted mean, 2 the nearest tap, 3 a hole,
    "own" = the pixel is its block's pick and its own tap is live, "w_own" / "sum_w" for such pixels"""
    T = dtype
    position, normal = np.asarray(position, F).astype(T), np.asarray(normal, F).astype(T)
    position_lo, normal_lo, color_lo = (np.asarray(a, F).astype(T) for a in (position_lo, normal_lo, color_lo))
    picks = np.asarray(picks, np.uint32).astype(np.int64)
    H, W = position.shape[:2]
    h, w = picks.shape
    assert (w, h) == low_size(W, H, f) and position_lo.shape == normal_lo.shape == color_lo.shape == (h, w, 4)
    sigma_plane, ff = T(sigma_plane), T(f * f)
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        A = position[..., 3]
        N = normal[..., :3]
        l2 = dot(N, N).astype(T)
        zero = ~(A > 0) | ~(l2 > 0)                                             # 1., 2.
        P = (position[..., :3] / A[..., None]).astype(T)
        n = (N / np.sqrt(l2)[..., None]).astype(T)
        tp = (normal[..., 3] / A).astype(T)
        sd = (sigma_plane * tp).astype(T)
        # what a low pixel alone decides
        Nq = normal_lo[..., :3]
        lq2 = dot(Nq, Nq).astype(T)
        skip_lo = (picks == PICK_NONE) | (picks >= W * H) | (color_lo[..., 3] == 0) | ~(position_lo[..., 3] > 0) | ~(lq2 > 0)
        Pq_lo = (position_lo[..., :3] / position_lo[..., 3:4]).astype(T)
        nq_lo = (Nq / np.sqrt(lq2)[..., None]).astype(T)
        xq_lo, yq_lo = picks % W, picks // W

        sum_w, sum_c = np.zeros((H, W), T), np.zeros((H, W, 3), T)
        near_have = np.zeros((H, W), bool)
        near_d2, near_c = np.zeros((H, W), T), np.zeros((H, W, 3), T)
        used, live_n, wn0, wp_half = (np.zeros((H, W), np.int32) for _ in range(4))
        own, w_own = np.zeros((H, W), bool), np.zeros((H, W), T)
        for dY in (-1, 0, 1):
            for dX in (-1, 0, 1):                                               # 3.
                qx, qy = xs // f + dX, ys // f + dY
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cqx, cqy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                live = inside & ~skip_lo[cqy, cqx]
                ddx, ddy = (xs - xq_lo[cqy, cqx]).astype(T), (ys - yq_lo[cqy, cqx]).astype(T)
                d2 = (ddx * ddx + ddy * ddy).astype(T)
                ws = (T(1) / (T(1) + d2 / ff)).astype(T)
                nq, Pq, cq = nq_lo[cqy, cqx], Pq_lo[cqy, cqx], color_lo[cqy, cqx]
                dn = dot(n, nq).astype(T)
                wn = np.where(dn > 0, dn, T(0)).astype(T)
                for _ in range(int(k)):
                    wn = (wn * wn).astype(T)
                e = dot(n, (Pq - P).astype(T)).astype(T)
                a = (np.abs(e) / sd).astype(T)
                wp = (T(1) / (T(1) + a * a)).astype(T)
                wt = ((ws * wn) * wp).astype(T)
                wt = np.where(np.isnan(wt), T(0), wt)
                nearer = live & (~near_have | (d2 < near_d2))
                near_have |= nearer
                near_d2 = np.where(nearer, d2, near_d2)
                near_c = np.where(nearer[..., None], cq[..., :3], near_c)
                add = live & (wt != 0)
                sum_w = np.where(add, sum_w + wt, sum_w).astype(T)
                sum_c = np.where(add[..., None], sum_c + wt[..., None] * cq[..., :3], sum_c).astype(T)
                used += add
                live_n += live
                wn0 += live & (wn == 0)
                wp_half += live & (wp < 0.5)
                if dX == 0 and dY == 0:
                    own = live & (xq_lo[cqy, cqx] == xs) & (yq_lo[cqy, cqx] == ys)
                    w_own = np.where(own, wt, T(0))
        out = np.zeros((H, W, 4), T)                                            # 4.
        mean = ~zero & (sum_w > 0)
        nearest = ~zero & ~mean & near_have
        out[..., :3] = np.where(mean[..., None], sum_c / sum_w[..., None], np.where(nearest[..., None], near_c, T(0)))
        out[..., 3] = np.where(mean | nearest, T(1), T(0))
        out[zero] = 0
    if want_info:
        how = np.where(zero, 0, np.where(mean, 1, np.where(nearest, 2, 3)))
        return out, {"used": used, "live": live_n, "wn0": wn0, "wp_half": wp_half, "how": how, "own": own & ~zero, "w_own": w_own,
                     "sum_w": sum_w}
    return out


def replicate(picks, color_lo, position, f):
    """each block's low colour copied over the block's hit pixels (the unguided upsampling the filter is measured against)"""
    H, W = np.asarray(position).shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.asarray(color_lo, F)[ys // f, xs // f].copy()
    out[~(np.asarray(position, F)[..., 3] > 0)] = 0
    return out
