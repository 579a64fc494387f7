"""mask_cache_begin_unit (minipath_amd/csrc/mask_cache.h) on the GPU, through libmp_mask_probe.so: for an interior view, the teapot
view, a pinhole, an f/0.7 lens and a view along an axis, and units at the image's centre, its corners, odd places and clipped tile
edges,

* the header the device function writes equals the numpy model (tools/analytic_bounds.py) bit for bit, the declined units
  included, and the node / leaf tags are all cleared where it adopts and untouched where it declines;
* the rays mp_generate_rays makes for the unit's first 64 samples per pixel are counted against the header: at the margin the
  library ships at most 1 % of the passes of the interior and the teapot view may have a ray outside it.
"""
import ctypes as C
import os

import numpy as np
import pytest

import minipath_amd as mp
from tests.test_unit_bounds_cpu import RES, SEED, _model, check_invariants, shipped_margin, unit_blocks

pytestmark = pytest.mark.gpu

SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minipath_amd", "csrc", "libmp_mask_probe.so")


def cameras():
    from minipath_amd import scenes

    eye, at, fnum = scenes.ATRIUM_VIEW
    return {"atrium": scenes.atrium_camera(), "teapot": mp.Camera.teapot_view(), "pinhole": mp.Camera.teapot_view().f_number(1e9),
            "f/0.7": mp.Camera.default().look_at(eye, at, (0, 1, 0)).f_number(0.7),
            "axis": mp.Camera.default().look_at((-15.0, 5.0, 0.0), (10.0, 5.0, 0.0), (0, 1, 0)).f_number(1e9)}


def probe_units(sampler, jscale, blocks):
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run build() first")
    L = C.CDLL(SO)
    L.mp_mask_probe_unit.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    s = np.ascontiguousarray(sampler, np.float32)
    b = np.ascontiguousarray(blocks, np.uint32)
    out = np.zeros((b.shape[0], 20), np.uint32)
    ntags, margin = C.c_uint32(0), C.c_float(0)
    rc = L.mp_mask_probe_unit(s.ctypes.data, float(jscale), b.ctypes.data, b.shape[0], out.ctypes.data, C.byref(ntags), C.byref(margin))
    assert rc == 0, f"HIP error {rc}"
    return out, ntags.value, margin.value


def unit_rays(ctx, smp, st, block, samples=64):
    """[samples, pixels, 3 groups, 3]: origin, inverse direction, direction of every ray of the unit"""
    import torch

    from minipath_amd import _lib

    x0, x1, y0, y1 = block
    blk = mp.ScreenBlock(x0, y0, x1 + 1, y1 + 1)
    n = blk.area()
    bufs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(6)]
    s, ss = smp.as_struct(), st.as_struct()
    out = np.zeros((samples, n, 3, 3), np.float32)
    for sample in range(samples):
        _lib.check(_lib.lib().mp_generate_rays(ctx.handle, C.byref(s), C.byref(ss), blk.as_struct(), sample, *[b.data_ptr() for b in bufs], None))
        torch.cuda.synchronize()
        g = np.stack([b.cpu().numpy() for b in bufs], -1)
        out[sample, :, 0], out[sample, :, 2] = g[:, :3], g[:, 3:]
    with np.errstate(divide="ignore"):
        out[:, :, 1] = np.where(out[:, :, 2] == 0, np.float32(np.inf), np.float32(1) / out[:, :, 2])
    return out


@pytest.mark.parametrize("name", ["atrium", "teapot", "pinhole", "f/0.7", "axis"])
def test_begin_unit_header_and_rays(name):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    ab = _model()
    ctx = mp.Context(0)
    st = mp.RenderSettings(64, 64, RES, seed=SEED)
    smp = cameras()[name].build_sampler(RES)
    s, js = smp.as_array(), ab.jitter_scale()
    blocks = unit_blocks()
    got, ntags, margin = probe_units(s, js, blocks)
    assert margin == np.float32(shipped_margin())
    adopted = declined = passes = esc = 0
    for blk, g in zip(blocks, got):
        state, lo, hi = ab.corner_header(s, js, *blk, margin)
        if state == 0xFFFFFFFF:
            declined += 1
            assert g[12] == 0xFFFFFFFF and g[19] == 0, (name, blk)
            continue
        adopted += 1
        check_invariants(state, lo, hi)
        assert np.array_equal(g[:19], ab.header_words(state, lo, hi)), (name, blk, g[:19], ab.header_words(state, lo, hi))
        assert g[19] == ntags, (name, blk)
        rays = unit_rays(ctx, smp, st, blk)  # [64, pixels, 3, 3]
        inside = ((rays >= lo) & (rays <= hi)).all(axis=(1, 2, 3))
        passes += 4
        esc += int((~inside.reshape(4, 16).all(1)).sum())
    print(f"{name}: margin {margin}: {adopted} units adopted, {declined} declined; {esc} of {passes} passes escape")
    if name == "axis":
        assert declined >= 2 and adopted >= 40  # the centre units' corners differ in sign
    else:
        assert adopted >= 40
    if name in ("atrium", "teapot"):
        assert esc * 100 <= passes, f"{esc} of {passes} passes escape the corner bounds"
