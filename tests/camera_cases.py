"""The camera matrix: samplers (the 15 floats of mp_camera_sampler) that the kernels accept at the C ABI and that no other test
renders -- an open lens at infinite focus, focus nearer than the focal length, focus 0, an 8 mm and an 800 mm lens, a portrait frame
sized by its sensor width, a rolled camera, look_direction, film scales that cross the windows of rm::ray_dir (ray_math.h) or make its
squares subnormal or zero, and samplers that are no rigid camera.  Plain data and host code, importable without a GPU:
tests/test_camera_cases_cpu.py proves that every case is what its name says, tests/test_gpu_cameras.py renders every case through
every route (ROUTES) against the oracle at the same 15 floats.

A case: values   the 15 sampler floats, np.float32
        sampler  the oracle's Sampler of the same floats (pyoracle.sampler_from_array)
        camera   what the product's drivers take: they only call camera.build_sampler(resolution), so a builder-made case hands them
                 its mp.Camera and a hand-made one a FixedSampler, which returns CameraSampler(values) whatever the resolution
        res      (width, height)
        built    builder-made cases: (mp.Camera, oracle Camera), the same builder calls on either side; None for hand-made ones

All cases look at the teapot (tests/golden/teapot.obj) on 48 x 32 pixels (portrait: 32 x 48), tile size 16, seed 0x5EED."""
import ctypes as C
from dataclasses import replace

import numpy as np

import minipath_amd as mp

F = np.float32
INF = float("inf")
RES, PORTRAIT_RES, TILE, SEED = (48, 32), (32, 48), 16, 0x5EED
DEPTH = 3
EYE, TARGET, UP = (0.0, 2.0, 10.0), (0.0, 1.5, 0.0), (0.0, 1.0, 0.0)  # the teapot view (benches/render_teapot.rs)

# ---- builder-made samplers: the calls, made once on mp.Camera and once on the oracle's mpo_camera_* ------------------------------
# eye, then "at" (look_at, which also focuses at the target) or "forward" (look_direction, which leaves the focus alone); focus None
# keeps what the placement left.  The teapot view is look_at + f/4.8 + focus 10.
TEAPOT_VIEW = dict(eye=EYE, at=TARGET, up=UP, f_number=4.8, focus=10.0)
WIDE = dict(eye=(0.0, 2.5, 2.0), at=TARGET, up=UP, focal=8e-3, sensor=("height", 36e-3))
BUILDERS = {
    "inf_focus_open": dict(TEAPOT_VIEW, f_number=1.4, focus=INF),
    "near_focus": dict(TEAPOT_VIEW, f_number=2.0, focus=0.02),
    "focus_zero": dict(TEAPOT_VIEW, f_number=2.0, focus=0.0),
    "wide": dict(WIDE, f_number=4.0),
    "wide_pinhole": dict(WIDE, f_number=INF),
    "tele": dict(eye=(0.0, 2.0, 160.0), at=TARGET, up=UP, focal=0.8, f_number=8.0),
    "portrait": dict(TEAPOT_VIEW, sensor=("width", 36e-3), res=PORTRAIT_RES),
    "rolled": dict(TEAPOT_VIEW, up=(0.3, 1.0, 0.2)),
    "look_direction": dict(eye=EYE, forward=(0.0, -0.05, -1.0), up=UP, f_number=4.8, focus=2.0),
}
# builder-made too, but no case of their own: what the hand-made cases are derived from (and compared with)
BASES = {
    "teapot": dict(TEAPOT_VIEW),
    "pinhole": dict(TEAPOT_VIEW, f_number=INF),
}
# ---- the film scales: film_origin_offset and pixel_scale * 2^k, which scales every unnormalised pinhole direction by 2^k exactly ---
K_MIXED = -32      # part of the frame has a direction component below 2^-40 (kCompLo), part has none
K_HIGH = 46        # part of the frame has the sum of squares >= 2^80 (kSumHi), part has not
K_SUBNORMAL = -60  # every square is subnormal: the plain sqrtf and / on denormal operands
K_FLUSH = -72      # every square is zero and no component is: x / 0, infinite directions with inverses of +-0
SCALED = {"scaled_mixed": ("wide_pinhole", K_MIXED), "scaled_high": ("wide_pinhole", K_HIGH),
          "scaled_subnormal": ("pinhole", K_SUBNORMAL), "scaled_flush": ("pinhole", K_FLUSH)}
HAND_MADE = tuple(SCALED) + ("anisotropic", "sheared", "negative_lens")
NAMES = tuple(BUILDERS) + HAND_MADE
NON_FINITE = ("focus_zero", "scaled_flush")  # every direction is NaN / infinite: the oracle's frame is all miss, without a NaN
FINITE = tuple(n for n in NAMES if n not in NON_FINITE)

# ---- the routes of tests/test_gpu_cameras.py: the call, its samples per pixel, the context options, the kernels it must report ----
# (tests/test_camera_cases_cpu.py holds the names against the launch plans; "wf": the staged pipeline's six kernels, as a set)
ROUTES = {
    "cached": dict(api="render", spp=64, opts={"packet_mask_cache": 1}, names=["render_tiles_packet_kernel<16, false, 8, false, true>"]),
    "uncached": dict(api="render", spp=64, opts={"packet_mask_cache": 0}, names=["render_tiles_packet_kernel<32, false, 7>"]),
    "groups": dict(api="render", spp=16, opts={}, traversal="groups", names=["render_tiles_kernel<1, false>"]),
    "paths": dict(api="paths", spp=16, opts={"paths_pooled": 1}, names=["render_paths_kernel<8, false, false>"]),
    "paths_pooled": dict(api="paths", spp=32, opts={"paths_pooled": 3}, names=["render_paths_pooled_kernel<4>"]),
    "staged": dict(api="wf", spp=16, opts={}, names={"wf_camera_kernel<false, false>", "wf_vertex_kernel<1, false>", "wf_scan_kernel",
                                                      "wf_scatter_kernel", "wf_trace_groups_kernel<false>", "wf_accumulate_kernel"}),
    "aov": dict(api="aov", spp=16, opts={}, names=["render_aov_packet_kernel<4, false, 8, false, true>"]),
}
SCALE_INVARIANT_ROUTES = ("cached", "uncached", "paths")  # where the scaled frames are held against the GPU's own wide_pinhole frame
# one cached-walk frame as two MP_FLAG_ACCUMULATE passes: (samples, the kernel its own sample count selects), both cached
TWO_PASS = ("inf_focus_open", ((24, "render_tiles_packet_kernel<4, false, 8, false, true>"), (40, "render_tiles_packet_kernel<8, false, 8, false, true>")))
RAYS_BLOCK, RAYS_SAMPLES = (16, 8, 32, 24), (0, 1, 2, 3)  # mp_generate_rays: one 16 x 16 block (x0, y0, x1, y1), samples 0-3


class FixedSampler:
    """a camera whose build_sampler returns the same 15 floats at every resolution: carries a hand-made sampler through every driver"""

    def __init__(self, values):
        self.values = tuple(float(v) for v in np.asarray(values, F).reshape(15))

    def build_sampler(self, resolution):
        return mp.CameraSampler(self.values)


def product_camera(spec):
    """the builder calls of `spec` on mp.Camera"""
    cam = mp.Camera.default()
    if "focal" in spec:
        cam = replace(cam, focal_length=spec["focal"])
    if "sensor" in spec:
        cam = cam.sensor_width(spec["sensor"][1]) if spec["sensor"][0] == "width" else cam.sensor_height(spec["sensor"][1])
    cam = cam.look_at(spec["eye"], spec["at"], spec["up"]) if "at" in spec else cam.look_direction(spec["eye"], spec["forward"], spec["up"])
    if "f_number" in spec:
        cam = cam.f_number(spec["f_number"])
    if spec.get("focus") is not None:
        cam = cam.focus_distance(spec["focus"])
    return cam


def oracle_camera(po, spec):
    """the same calls on the oracle's camera"""
    c, L = po.Camera(), po.lib()
    L.mpo_camera_default(C.byref(c))
    if "focal" in spec:
        c.focal_length = spec["focal"]
    if "sensor" in spec:
        c.sensor_is_width, c.sensor_size = (1 if spec["sensor"][0] == "width" else 0), spec["sensor"][1]
    if "at" in spec:
        L.mpo_camera_look_at(C.byref(c), po.vec3(*spec["eye"]), po.vec3(*spec["at"]), po.vec3(*spec["up"]))
    else:
        L.mpo_camera_look_direction(C.byref(c), po.vec3(*spec["eye"]), po.vec3(*spec["forward"]), po.vec3(*spec["up"]))
    if "f_number" in spec:
        c.f_number = spec["f_number"]
    if spec.get("focus") is not None:
        c.focus_distance = spec["focus"]
    return c


def scaled(values, k):
    """film_origin_offset and pixel_scale * 2^k"""
    v = np.array(values, F)
    v[9:13] = v[9:13] * F(2.0) ** F(k)
    return v


def film_at_centres(values, res):
    """camera_film (camera_rays.h) at the pixel centres in np.float32, operation by operation: [h, w, 3].  A pinhole's unnormalised
    direction is its negative, so |component| and the sum of squares are those rm::ray_dir tests."""
    s = np.asarray(values, F)
    up, right, foo, pixel_scale = s[3:6], s[6:9], s[9:12], s[12]
    v, u = np.meshgrid(np.arange(res[1], dtype=F), np.arange(res[0], dtype=F), indexing="ij")
    fv, fu = v * pixel_scale, u * pixel_scale
    return np.stack([(foo[k] + up[k] * fv) - right[k] * fu for k in range(3)], -1).astype(F)


def window_counts(values, res):
    """pixel centres (with a component below 2^-40, with the sum of squares >= 2^80, with the sum below 2^-80)"""
    f = film_at_centres(values, res)
    with np.errstate(over="ignore", under="ignore"):
        x = ((f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]) + f[..., 2] * f[..., 2]).astype(F)
    return int((np.abs(f).min(-1) < F(2.0) ** -40).sum()), int((x >= F(2.0) ** 80).sum()), int((x < F(2.0) ** -80).sum())


_cases = {}


def base_values(name):
    """the product's sampler of a builder spec (a case or a base) at its resolution"""
    spec = {**BUILDERS, **BASES}[name]
    return product_camera(spec).build_sampler(spec.get("res", RES)).as_array()


def cases():
    """{name: case}, made once"""
    if _cases:
        return _cases
    from oracle import pyoracle as po

    def add(name, values, camera, res, built=None):
        values = np.ascontiguousarray(values, F)
        _cases[name] = dict(values=values, sampler=po.sampler_from_array(values), camera=camera, res=res, built=built)

    for name, spec in BUILDERS.items():
        cam, res = product_camera(spec), spec.get("res", RES)
        add(name, cam.build_sampler(res).as_array(), cam, res, (cam, oracle_camera(po, spec)))
    hand = {name: scaled(base_values(base), k) for name, (base, k) in SCALED.items()}
    teapot = base_values("teapot")
    hand["anisotropic"] = teapot.copy()
    hand["anisotropic"][6:9] *= F(2)
    hand["sheared"] = teapot.copy()
    hand["sheared"][3:6] = teapot[3:6] + F(0.5) * teapot[6:9]
    hand["negative_lens"] = teapot.copy()
    hand["negative_lens"][13] = -teapot[13]
    for name in HAND_MADE:
        add(name, hand[name], FixedSampler(hand[name]), RES)
    assert tuple(_cases) == NAMES
    return _cases
