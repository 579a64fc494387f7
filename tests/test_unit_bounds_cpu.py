"""The mask cache's unit bounds from the camera (mask_cache_begin_unit, minipath_amd/csrc/mask_cache.h) in their numpy restatement
(tools/analytic_bounds.py), which tests/test_unit_bounds_gpu.py compares with the device function bit for bit.  ray_math.h's
Ray::new is device code, so the host side of the comparison is this model; here it is held against the oracle's rays:

* the header invariants for an interior view, the teapot view, a pinhole, an f/0.7 lens: lo <= hi, inverse bounds of one sign,
  non-zero and finite, origin bounds within 2^31, direction bounds within 2;
* a view along an axis declines at the image centre (the corners' inverse directions differ in sign);
* the oracle's rays of each unit's first 64 samples per pixel lie inside the bounds: at the shipped margin at most 1 % of the passes
  (16 samples of each of a unit's 2x2 pixels) of the interior and the teapot view may escape.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = (1920, 1080)
SEED = 0x5EED


def _model():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import analytic_bounds as ab
    return ab


def shipped_margin():
    src = open(os.path.join(ROOT, "minipath_amd", "csrc", "mask_cache.h")).read()
    return float(re.search(r"#define MP_MCACHE_MARGIN ([-0-9.e]+)f", src).group(1))


def views(oracle):
    """name -> oracle camera"""
    from minipath_amd import scenes

    def look(eye, at, fnum):
        c = oracle.Camera()
        oracle.lib().mpo_camera_default(C.byref(c))
        oracle.lib().mpo_camera_look_at(C.byref(c), oracle.vec3(*eye), oracle.vec3(*at), oracle.vec3(0, 1, 0))
        c.f_number = fnum
        return c

    eye, at, fnum = scenes.ATRIUM_VIEW
    pin = oracle.teapot_camera(); pin.f_number = 1e9
    wide = look(eye, at, 0.7)
    return {"atrium": look(eye, at, fnum), "teapot": oracle.teapot_camera(), "pinhole": pin, "f/0.7": wide,
            "axis": look((-15.0, 5.0, 0.0), (10.0, 5.0, 0.0), 1e9)}


def unit_blocks(res=RES):
    """2x2 units: the image's centre and corners, odd places, and units a tile edge clips to one column / one row / one pixel"""
    w, h = res
    b = [(0, 1, 0, 1), (w - 2, w - 1, 0, 1), (0, 1, h - 2, h - 1), (w - 2, w - 1, h - 2, h - 1), (w // 2, w // 2 + 1, h // 2, h // 2 + 1),
         (w // 2 - 2, w // 2 - 1, h // 2 - 2, h // 2 - 1), (322, 323, 200, 201), (1400, 1401, 900, 901), (64, 65, 1000, 1001),
         (w - 1, w - 1, 10, 11), (30, 31, h - 1, h - 1), (w - 1, w - 1, h - 1, h - 1)]
    rng = np.random.default_rng(5)
    for _ in range(40):
        x, y = 2 * int(rng.integers(0, w // 2)), 2 * int(rng.integers(0, h // 2))
        b.append((x, x + 1, y, y + 1))
    return b


def check_invariants(state, lo, hi):
    assert state & 0x100 and state < 0x108
    assert (lo <= hi).all()
    for k in range(3):
        neg = bool(state >> k & 1)
        assert np.isfinite(lo[1, k]) and np.isfinite(hi[1, k])
        assert (hi[1, k] < 0) if neg else (lo[1, k] > 0)
    assert (np.abs(lo[0]) <= 2.0 ** 31).all() and (np.abs(hi[0]) <= 2.0 ** 31).all()
    assert (np.abs(lo[2]) <= 2.0).all() and (np.abs(hi[2]) <= 2.0).all()


def escaping_passes(oracle, smp, block, lo, hi, spp=64):
    """passes of 16 samples per pixel of the unit with a ray outside [lo, hi]"""
    x0, x1, y0, y1 = block
    esc = 0
    for p in range(spp // 16):
        out = False
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                for sub in range(16):
                    r = oracle.sample_ray(smp, x, y, oracle.lib().mpo_sample_key(SEED, RES[0], spp, x, y, p * 16 + sub))
                    v = np.array([list(r.o), list(r.inv), list(r.d)], np.float32)
                    out = out or not ((v >= lo) & (v <= hi)).all()
        esc += out
    return esc


@pytest.mark.parametrize("name", ["atrium", "teapot", "pinhole", "f/0.7"])
def test_corner_bounds_hold_the_units_rays(oracle, name):
    ab = _model()
    margin = shipped_margin()
    smp = oracle.build_sampler(views(oracle)[name], *RES)
    s, js = smp.as_array(), ab.jitter_scale()
    passes = esc = adopted = 0
    for blk in unit_blocks():
        state, lo, hi = ab.corner_header(s, js, *blk, margin)
        if state == 0xFFFFFFFF:
            continue
        adopted += 1
        check_invariants(state, lo, hi)
        esc += escaping_passes(oracle, smp, blk, lo, hi)
        passes += 4
    print(f"{name}: margin {margin}: {adopted} units adopted, {esc} of {passes} passes escape")
    assert adopted >= 40
    if name in ("atrium", "teapot"):
        assert esc * 100 <= passes, f"{esc} of {passes} passes escape the corner bounds"


def test_axis_aligned_view_declines(oracle):
    ab = _model()
    smp = oracle.build_sampler(views(oracle)["axis"], *RES)
    s, js = smp.as_array(), ab.jitter_scale()
    w, h = RES
    # the view direction is +x: over the centre unit the y and z components of the corners' directions change sign
    assert ab.corner_header(s, js, w // 2 - 1, w // 2, h // 2 - 1, h // 2, shipped_margin())[0] == 0xFFFFFFFF
    # away from the centre column and row the corners agree
    state, lo, hi = ab.corner_header(s, js, 100, 101, 100, 101, shipped_margin())
    check_invariants(state, lo, hi)


def test_margin_guards():
    """a margin that would carry an inverse bound across zero or to infinity leaves that bound unwidened; origins and directions are
    capped"""
    ab = _model()
    f = np.float32
    lo = np.array([[-2.0 ** 31, 0, 0], [1e-3, -3e38, 1.0], [-1.9, 0.5, -1.0]], f)
    hi = np.array([[2.0 ** 31, 1, 0], [1.0, -1.0, 1.0], [1.9, 0.5, 1.0]], f)
    wlo, whi = ab.widen(lo, hi, 0.25)
    assert wlo[1, 0] == f(1e-3) and whi[1, 0] == f(1.24975)     # 1e-3 - 0.25 would be negative
    assert wlo[1, 1] == f(-3e38) and whi[1, 1] == f(-1.0)       # -inf, and +7.5e37 has the other sign
    assert wlo[1, 2] == 1.0 and whi[1, 2] == 1.0
    assert wlo[0, 0] == f(-2.0 ** 31) and whi[0, 0] == f(2.0 ** 31) and wlo[2, 0] == -2.0 and whi[2, 0] == 2.0
    assert wlo[2, 1] == 0.5 and whi[2, 1] == 0.5
