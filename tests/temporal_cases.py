"""The inputs the CPU and the GPU tests of the temporal reprojection share: seeded synthetic frames whose projections are planted on
every special place of include/minipath_temporal.h, and the two-camera teapot case.  Everything here is made once and never
changed; the CPU tests show that the inputs reach every rule (tests/test_temporal_cpu.py), the GPU tests compare bits."""
import ctypes as C

import numpy as np

from tests import temporal_model as tm
from tests.temporal_model import F

# below, at and above one 32 x 8 block in each direction, ragged right and bottom edges
SIZES = [(1, 1), (3, 2), (31, 9), (33, 8), (37, 23), (64, 16)]
SIGMA_POSITION, NORMAL_MIN = 1.2, 0.8  # for the synthetic frames: neighbouring hit points are a unit apart and the distance plane says 0.8 .. 1.2


def exact_view(w, h):
    """a previous view under which the point (X, Y, 1) is seen at exactly u = cx + X, v = cy + Y: k = 1, up = -y"""
    return tm.View((0, 0, 0), (0, 0, 1), (1, 0, 0), (0, -1, 0), 1.0, F(w - 1) * F(0.5), F(h - 1) * F(0.5))


def general_view(w, h):
    """a previous view in general position: nothing about it is exact"""
    f = np.array([0.3, -0.2, 0.93], np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(f, [0.1, 1.0, 0.05])
    r /= np.linalg.norm(r)
    return tm.View((0.7, -1.3, 2.1), f, r, np.cross(r, f), 41.7, F(w - 1) * F(0.5), F(h - 1) * F(0.5))


_synthetic = {}


def synthetic(w, h, general=False):
    """{"cur": colour, position, normal, ids, variance; "prev": position, normal, ids, color, moments; "view"} for a size.

    Previous frame: pixel q holds the point the view sees at q (plus a little noise) at distance about 1, so a current point planted
    at (u, v) finds taps whose points are about a pixel (one unit under exact_view) away.  Planted in the current frame, cycling
    over the pixels so that the smallest sizes get the first few: landings exactly on integers, in (-1, 0) and (W-1, W) and the
    same in y, outside the image, behind the camera, a == 0, NaN and infinite points, misses and partial alphas.  Ids take few
    values, so every compare of the skip rule sees both outcomes; some normals are turned away or NaN; the history of a previous
    miss holds NaN and huge values that must never be read."""
    key = (w, h, general)
    if key in _synthetic:
        return _synthetic[key]
    rng = np.random.default_rng(7919 * w + 31 * h + general)
    view = general_view(w, h) if general else exact_view(w, h)
    c64, f64, r64, u64 = (np.asarray(v, np.float64) for v in (view.center, view.forward, view.right, view.up))
    k, cx, cy = float(view.k), float(view.cx), float(view.cy)

    def points(u, v, a):
        """the points seen at (u, v) at depth a"""
        u, v, a = (np.asarray(t, np.float64)[..., None] for t in (u, v, a))
        return c64 + f64 * a + r64 * ((u - cx) * a / k) + u64 * ((cy - v) * a / k)

    def ids_plane(alphas):
        """{prim, instance, material, hit}: mostly 0, so most compares of the skip rule agree and each of them sometimes does not"""
        few = lambda p: rng.choice([0, 1, 0xFFFFFFFF], (h, w), p=[1 - 2 * p, p, p])  # noqa: E731
        return np.stack([few(0.04), few(0.03), few(0.03), alphas != 0], -1).astype(np.uint32)

    yy, xx = np.mgrid[0:h, 0:w]
    depth = 1.0 if not general else 41.7  # one pixel is one unit wide at this depth under either view
    # ---- the previous frame
    pa = rng.choice([1.0, 0.5, 0.125, 0.0], (h, w), p=[0.7, 0.1, 0.1, 0.1])  # previous alphas, some misses
    pp = points(xx, yy, depth) + rng.normal(0, 0.05, (h, w, 3))
    pn = np.array([0.0, 0.0, -1.0]) + rng.normal(0, 0.2, (h, w, 3))
    pn /= np.linalg.norm(pn, axis=-1, keepdims=True)
    pn[rng.random((h, w)) < 0.05] *= -1  # turned away
    prev = {"position": np.concatenate([pp * pa[..., None], pa[..., None]], -1).astype(F),
            "normal": np.concatenate([pn * pa[..., None], pa[..., None]], -1).astype(F),  # (.w, the distance, is not read)
            "ids": ids_plane(pa),
            "color": rng.random((h, w, 4)).astype(F), "moments": np.zeros((h, w, 4), F)}
    prev["normal"][rng.random((h, w)) < 0.05, :3] = np.nan
    prev["position"][rng.random((h, w)) < 0.03, 0] = np.nan
    prev["moments"][..., 0] = rng.random((h, w)).astype(F) * 3
    prev["moments"][..., 1] = prev["moments"][..., 0] ** 2 + rng.random((h, w)).astype(F)
    prev["moments"][..., 2] = rng.integers(1, 6, (h, w)).astype(F)
    gone = pa == 0
    prev["color"][gone] = (F(np.nan), F(3e38), F(-3e38), F(np.inf))  # never read
    prev["moments"][gone] = F(np.nan)
    # ---- the current frame: where each pixel is to land in the previous one
    n = np.arange(h * w).reshape(h, w)
    u = xx + rng.uniform(-1.5, 1.5, (h, w))
    v = yy + rng.uniform(-1.5, 1.5, (h, w))
    a = np.full((h, w), depth)
    kind = n % 16
    ix, iy = rng.integers(0, w, (h, w)), rng.integers(0, h, (h, w))
    u = np.where(kind == 0, ix, u); v = np.where(kind == 0, iy, v)                        # noqa: E702  both integers: three zero weights
    u = np.where(kind == 1, ix, u)                                                       # fx == 0
    v = np.where(kind == 2, iy, v)                                                       # fy == 0
    u = np.where(kind == 3, -0.25, u); v = np.where(kind == 3, iy + 0.5, v)              # noqa: E702  x0 == -1
    u = np.where(kind == 4, w - 0.25, u); v = np.where(kind == 4, iy + 0.5, v)           # noqa: E702  x0 == W - 1
    u = np.where(kind == 5, ix + 0.5, u); v = np.where(kind == 5, -0.5, v)               # noqa: E702  y0 == -1
    u = np.where(kind == 6, ix + 0.5, u); v = np.where(kind == 6, h - 0.5, v)            # noqa: E702  y0 == H - 1
    u = np.where(kind == 7, rng.choice([-1.0, float(w), -3.0, w + 2.5], (h, w)), u)      # off the image, the open ends included
    v = np.where(kind == 8, rng.choice([-1.0, float(h), -3.0, h + 2.5], (h, w)), v)
    a = np.where(kind == 9, -depth, a)                                                   # behind the camera
    a = np.where(kind == 10, 0.0, a)                                                     # a == 0
    cp = points(u, v, a)
    alpha = rng.choice([1.0, 1.0, 0.5, 0.375], (h, w))
    alpha = np.where(kind == 11, 0.0, alpha)                                             # a miss
    cn = np.array([0.0, 0.0, -1.0]) + rng.normal(0, 0.2, (h, w, 3))
    cn /= np.linalg.norm(cn, axis=-1, keepdims=True)
    cur = {"color": rng.random((h, w, 4)).astype(F),
           "position": np.concatenate([cp * alpha[..., None], alpha[..., None]], -1).astype(F),
           "normal": np.concatenate([cn * alpha[..., None], (rng.uniform(0.8, 1.2, (h, w)) * alpha)[..., None]], -1).astype(F),
           "ids": ids_plane(alpha),
           "variance": np.zeros((h, w, 4), F)}
    if not general:  # the integer landings are exact when nothing is rounded: no division by a partial alpha other than a power of two
        exact = (kind <= 6) & (alpha == 0.375)
        cur["position"][exact] = np.concatenate([cp, np.ones((h, w, 1))], -1).astype(F)[exact]
    cur["position"][kind == 12, 1] = np.nan
    cur["position"][kind == 13, 2] = np.inf
    cur["position"][kind == 14, 3] = np.nan  # a NaN alpha is a hit
    cur["normal"][(kind == 15) & (rng.random((h, w)) < 0.5), :3] = np.nan
    cur["color"][rng.random((h, w)) < 0.02, 1] = np.nan  # passes through or poisons: the model says which
    cur["variance"][..., 0] = rng.random((h, w)).astype(F) * F(0.01)
    cur["variance"][..., 1:] = F(7)  # never read
    _synthetic[key] = {"cur": cur, "prev": prev, "view": view}
    return _synthetic[key]


def synthetic_settings(max_history, alpha, match_prim):
    """the model's keyword arguments for a parameter combination; alpha_moments differs from alpha_color so the two cannot be mixed up"""
    return dict(sigma_position=SIGMA_POSITION if np.isfinite(max_history) else float("inf"), normal_min=NORMAL_MIN, max_history=max_history,
                alpha_color=alpha, alpha_moments=0.25 if alpha == 0 else alpha, min_variance_history=3.0, match_prim=match_prim)


def model_on(case, settings, with_variance, want_info=False):
    cur, prev = case["cur"], case["prev"]
    return tm.reproject(cur["color"], cur["position"], cur["normal"], cur["ids"], case["view"], prev["position"], prev["normal"], prev["ids"],
                        prev["color"], prev["moments"], variance_in=cur["variance"] if with_variance else None, want_info=want_info, **settings)


# ---- the two-camera case on the renderer's own planes ---------------------------------------------------------------------------
# Two instances of the teapot, the second behind and beside the first: a single teapot has one instance and one material, so no
# camera move could make the ids rule skip a tap.  The second camera is the first moved to the right and turned a little, which
# uncovers parts of the far teapot (ids), of the near one's body behind its spout and handle (position) and of creases (normal), and
# takes the left edge of the frame out of the first camera's image.
E2E = dict(res=(96, 64), spp=8, tile=32, seeds=(100, 101), instances=[[0, 0, 0], [2.5, 0.3, -3.5]],
           cameras=[((0.0, 2.0, 10.0), (0.0, 1.5, 0.0)), ((0.8, 2.2, 10.0), (0.6, 1.5, 0.0))],
           settings=dict(sigma_position=0.01, normal_min=0.98, max_history=32.0, alpha_color=0.2, alpha_moments=0.2, min_variance_history=4.0,
                         match_prim=False))
E2E_MIN_PER_CLASS = 8


def e2e_camera(mp, i):
    """camera i of the case: a pinhole (f_number = inf), so every sample of a pixel goes through the lens centre"""
    eye, at = E2E["cameras"][i]
    return mp.Camera.default().look_at(eye, at, (0.0, 1.0, 0.0)).f_number(float("inf"))


def oracle_camera(po, eye, at, f_number=float("inf"), focus_distance=None):
    c = po.Camera()
    po.lib().mpo_camera_default(C.byref(c))
    po.lib().mpo_camera_look_at(C.byref(c), po.vec3(*eye), po.vec3(*at), po.vec3(0.0, 1.0, 0.0))
    c.f_number = f_number
    if focus_distance is not None:
        c.focus_distance = focus_distance
    return c


def oracle_view(po, cam, resolution):
    """(mpt_view of an oracle camera by the model's view_of, its sampler)"""
    out = [np.zeros(3, F) for _ in range(4)]
    po.lib().mpo_camera_basis(C.byref(cam), *[po._f32p(o) for o in out])
    s = po.build_sampler(cam, *resolution)
    return tm.view_of(out[0], out[1], out[2], out[3], cam.focal_length, s.pixel_scale, resolution), s


_e2e = {}


def e2e_model(po, teapot_obj):
    """The oracle's planes of the two frames, the model's first frame and its reprojection with info: made once"""
    if not _e2e:
        from tests import aov_pass_model

        w, h = E2E["res"]
        b = po.Bvh.from_obj(teapot_obj)
        b.set_instances(np.array(E2E["instances"], F))
        frames = []
        for i, (eye, at) in enumerate(E2E["cameras"]):
            view, smp = oracle_view(po, oracle_camera(po, eye, at), E2E["res"])
            frames.append((aov_pass_model.planes(po, b.intersect, smp, w, E2E["spp"], E2E["seeds"][i], (0, 0, w, h)), view))
        (p0, v0), (p1, v1) = frames
        out0, mom0 = tm.reset(p0["shade"], p0["position"])
        out1, mom1, var1, info = tm.reproject(p1["shade"], p1["position"], p1["normal"], p1["ids"], v0, p0["position"], p0["normal"], p0["ids"],
                                              out0, mom0, want_info=True, **E2E["settings"])
        _e2e.update(planes=(p0, p1), views=(v0, v1), first=(out0, mom0), second=(out1, mom1, var1), info=info, keep=b)
    return _e2e
