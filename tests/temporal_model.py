"""numpy restatement of include/minipath_temporal.h, operation by operation in np.float32: the expectation of
libminipath_temporal.so's kernels, which must give these bits.  Vectorised over the pixels, a loop over the four taps in the
header's order (j outer, i inner), every sum taken in that order from +0.0.  Runs under np.errstate(all="ignore"): NaN and infinite
intermediates are part of the definition (they fail the compares), not warnings.

Besides the results reproject() reports what happened to every pixel and tap (`info`), which the tests use to show that their inputs
reach every rule."""
import numpy as np

F = np.float32
FLAG_MATCH_PRIM = 1

# info["tap"][y, x, 2*j + i]: the first rule of step 4 that skipped the tap, in the header's order; KEPT otherwise
KEPT, T_OUTSIDE, T_PREV_MISS, T_IDS, T_POSITION, T_NORMAL, T_ZERO_WEIGHT, T_NONE = 0, 1, 2, 3, 4, 5, 6, 7  # T_NONE: no taps were made
# info["pixel"][y, x]
P_MISS, P_BEHIND, P_OFFSCREEN, P_NO_TAP_KEPT, P_HISTORY = 0, 1, 2, 3, 4


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def mx(a, c):
    """the header's max(a, c) = a > c ? a : c with c the constant: c for NaN, +0 for max(-0, 0)"""
    return np.where(a > F(c), a, F(c)).astype(F)


def mn(a, c):
    """the header's min(a, c) = a < c ? a : c with c the constant: c for NaN"""
    return np.where(a < F(c), a, F(c)).astype(F)


def dot(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F)


class View:
    """mpt_view"""

    def __init__(self, center, forward, right, up, k, cx, cy):
        self.center, self.forward, self.right, self.up = (np.asarray(v, F).reshape(3) for v in (center, forward, right, up))
        self.k, self.cx, self.cy = F(k), F(cx), F(cy)

    def floats(self):
        return np.concatenate([self.center, self.forward, self.right, self.up, [self.k, self.cx, self.cy]]).astype(F)


def view_of(center, forward, up, right, focal_length, pixel_scale, resolution):
    """the arithmetic of TemporalAccumulator.view_of: (center, forward, up, right) in the order of Camera.center_forward_up_right()"""
    w, h = resolution
    return View(center, forward, right, up, F(focal_length) / F(pixel_scale), F(w - 1) * F(0.5), F(h - 1) * F(0.5))


def project(view, P):
    """step 3 for points P [..., 3]: (a, u, v); u and v are meaningless where !(a > 0)"""
    with np.errstate(all="ignore"):
        w = (np.asarray(P, F) - view.center).astype(F)
        a, b, c = dot(w, view.forward), dot(w, view.right), dot(w, view.up)
        s = (view.k / a).astype(F)
        return a, (view.cx + b * s).astype(F), (view.cy - c * s).astype(F)


def luminance(color):
    return ((color[..., 0] + color[..., 1]) + color[..., 2]).astype(F)


def reset(color, position):
    """mpt_reset: (out, moments_out)"""
    with np.errstate(all="ignore"):
        color, position = np.asarray(color, F), np.asarray(position, F)
        hit = position[..., 3] != 0
        l = luminance(color)
        mom = np.zeros(color.shape, F)
        mom[..., 0] = np.where(hit, l, F(0))
        mom[..., 1] = np.where(hit, (l * l).astype(F), F(0))
        mom[..., 2] = np.where(hit, F(1), F(0))
        return color.copy(), mom


def reproject(color, position, normal, ids, prev_view, prev_position, prev_normal, prev_ids, hist_color, hist_moments, sigma_position,
              normal_min, max_history, alpha_color, alpha_moments, min_variance_history, match_prim=False, variance_in=None,
              want_info=False):
    """mpt_reproject on host arrays [h, w, 4]: (out, moments_out, variance_out), and info with want_info"""
    with np.errstate(all="ignore"):
        color, position, normal = (np.asarray(v, F) for v in (color, position, normal))
        prev_position, prev_normal, hist_color, hist_moments = (np.asarray(v, F) for v in (prev_position, prev_normal, hist_color, hist_moments))
        ids, prev_ids = np.asarray(ids).view(np.uint32), np.asarray(prev_ids).view(np.uint32)
        H, W = color.shape[:2]
        # 1, 2
        A = position[..., 3]
        hit = A != 0
        P = (position[..., :3] / A[..., None]).astype(F)
        tp = (normal[..., 3] / A).astype(F)
        l = luminance(color)
        ll = (l * l).astype(F)
        # 3
        a, u, v = project(prev_view, P)
        front = a > 0
        inside = front & (u > F(-1)) & (u < F(W)) & (v > F(-1)) & (v < F(H))
        us, vs = np.where(inside, u, F(0)), np.where(inside, v, F(0))
        x0, y0 = np.floor(us).astype(np.int64), np.floor(vs).astype(np.int64)
        fx, fy = (us - x0.astype(F)).astype(F), (vs - y0.astype(F)).astype(F)
        # 4
        r = (F(sigma_position) * tp).astype(F)
        rr = (r * r).astype(F)
        sw = np.zeros((H, W), F)
        sums = np.zeros((H, W, 6), F)  # colour x, y, z, moments x, y, z
        tap = np.full((H, W, 4), T_NONE, np.uint8)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                inb = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                qpos, qnrm, qid = prev_position[cy, cx], prev_normal[cy, cx], prev_ids[cy, cx]
                B = qpos[..., 3]
                same = (qid[..., 1] == ids[..., 1]) & (qid[..., 2] == ids[..., 2])
                if match_prim:
                    same &= qid[..., 0] == ids[..., 0]
                e = ((qpos[..., :3] / B[..., None]).astype(F) - P).astype(F)
                near = dot(e, e) <= rr
                facing = dot(normal, qnrm) >= (F(normal_min) * (A * B).astype(F)).astype(F)
                wx = fx if i else (F(1) - fx).astype(F)
                wy = fy if j else (F(1) - fy).astype(F)
                wt = (wx * wy).astype(F)
                why = np.full((H, W), KEPT, np.uint8)
                for code, ok in ((T_ZERO_WEIGHT, wt != 0), (T_NORMAL, facing), (T_POSITION, near), (T_IDS, same), (T_PREV_MISS, B != 0),
                                 (T_OUTSIDE, inb)):
                    why = np.where(ok, why, code).astype(np.uint8)  # the earliest failing rule is written last
                why = np.where(hit & inside, why, T_NONE).astype(np.uint8)
                tap[..., 2 * j + i] = why
                keep = why == KEPT
                hc, hm = hist_color[cy, cx], hist_moments[cy, cx]
                sw = np.where(keep, sw + wt, sw).astype(F)
                for n, src in enumerate((hc[..., 0], hc[..., 1], hc[..., 2], hm[..., 0], hm[..., 1], hm[..., 2])):
                    sums[..., n] = np.where(keep, sums[..., n] + wt * src, sums[..., n])
        # 5
        have = hit & (sw > 0)
        h = (sums / sw[..., None]).astype(F)
        N = mn(h[..., 5] + F(1), max_history)
        ac, am = mx(F(1) / N, alpha_color), mx(F(1) / N, alpha_moments)
        out = color.copy()
        for c in range(3):
            out[..., c] = np.where(have, h[..., c] + ac * (color[..., c] - h[..., c]), color[..., c])
        m1 = np.where(have, h[..., 3] + am * (l - h[..., 3]), l).astype(F)
        m2 = np.where(have, h[..., 4] + am * (ll - h[..., 4]), ll).astype(F)
        N = np.where(have, N, F(1)).astype(F)
        mom = np.zeros(color.shape, F)
        for n, src in enumerate((m1, m2, N)):
            mom[..., n] = np.where(hit, src, F(0))
        # 6
        var = np.zeros(color.shape, F)
        vv = mx(m2 - (m1 * m1).astype(F), 0)
        if variance_in is not None:
            vv = np.where(N >= F(min_variance_history), vv, np.asarray(variance_in, F)[..., 0]).astype(F)
        var[..., 0] = np.where(hit, vv, F(0))
        if not want_info:
            return out, mom, var
        pixel = np.full((H, W), P_HISTORY, np.uint8)
        pixel = np.where(have, pixel, P_NO_TAP_KEPT)
        pixel = np.where(inside, pixel, P_OFFSCREEN)
        pixel = np.where(front, pixel, P_BEHIND)
        pixel = np.where(hit, pixel, P_MISS).astype(np.uint8)
        return out, mom, var, {"pixel": pixel, "tap": tap, "kept": (tap == KEPT).sum(-1), "u": u, "v": v, "x0": x0, "y0": y0}


def classes(info):
    """The pixel classes the end-to-end case must hold, as boolean masks.  A pixel without a kept tap is put down to the LAST rule any
    of its taps got to: "normal" if a tap failed only there, else "position" if one got as far as that test, else "ids"."""
    px, tap, kept = info["pixel"], info["tap"], info["kept"]
    none = px == P_NO_TAP_KEPT
    got_to = lambda code: (tap == code).any(-1)  # noqa: E731
    return {
        "four_taps": (px == P_HISTORY) & (kept == 4),
        "one_to_three_taps": (px == P_HISTORY) & (kept >= 1) & (kept <= 3),
        "ids": none & got_to(T_IDS) & ~got_to(T_POSITION) & ~got_to(T_NORMAL),
        "position": none & got_to(T_POSITION) & ~got_to(T_NORMAL),
        "normal": none & got_to(T_NORMAL),
        "offscreen": px == P_OFFSCREEN,
        "miss": px == P_MISS,
    }


class Accumulator:
    """TemporalAccumulator on the host: chained model calls with the accumulator's settings"""

    def __init__(self, **settings):
        self.settings = settings
        self.prev = None

    def reset(self):
        self.prev = None

    def accumulate(self, color, position, normal, ids, view, variance=None):
        if self.prev is None:
            out, mom = reset(color, position)
            var = first_frame_variance(mom.shape, variance, self.settings["min_variance_history"])
        else:
            p = self.prev
            out, mom, var = reproject(color, position, normal, ids, p["view"], p["position"], p["normal"], p["ids"], p["color"], p["moments"],
                                      variance_in=variance, **self.settings)
        self.prev = {"view": view, "position": np.array(position, F), "normal": np.array(normal, F), "ids": np.array(ids).view(np.uint32).copy(),
                     "color": out, "moments": mom}
        return out, var


def first_frame_variance(shape, variance, min_variance_history):
    """What TemporalAccumulator returns beside a first frame, which has no temporal variance: the caller's plane as it is while a
    history of length 1 is below min_variance_history, else zeros (step 6 at N' = 1: max(l*l - l*l, 0))"""
    if variance is None or not (F(1) < F(min_variance_history)):
        return np.zeros(shape, F)
    return np.array(variance, F)
