"""CPU tests of the feature planes in passes (mp_render_aov_pass_device): the launch plan through the host probe's
mp_plan_aov_pass (the wide park of the point / squared-shade planes, kernels chosen by the pass's samples), the bindings, the
model (tests/aov_pass_model.py) against tests/aov_model.py, and the checkpoint round trip with planes.  The numbers are derived by
hand from the rules of plan_render_aov: park = 4 waves x (64 / S) pixels x 32 or 48 bytes, in front of the mask cache's 4 x 3 712
bytes or the LDS stack's (stack_bound - registers) x 16 bytes x 4 waves."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import aov_model, aov_pass_model
from tests import dispatch_cases as dc
from tests import plan_probe as pp
from tests.aov_model import bits
from tests.conftest import TEAPOT as TEAPOT_OBJ

F = np.float32
TEAPOT, GROUP_RGB = dc.scene_facts("teapot"), dc.scene_facts("group+rgb")
FRAME = (510, 64)  # the benchmark's frame, as tests/test_launch_plan_cpu.py
A = "render_aov_packet_kernel"
STACK = "scene too deep for the LDS traversal stack"


def plan(facts, frame, spp, wide, passes=None, **kw):
    """(PlanOut, park bytes per pixel) of mp_plan_aov_pass"""
    lib = pp.lib()
    lib.mp_plan_aov_pass.argtypes = [C.POINTER(pp.PlanIn), C.c_int, C.POINTER(pp.PlanOut), C.POINTER(C.c_uint32)]
    lib.mp_plan_aov_pass.restype = None
    out, park = pp.PlanOut(), C.c_uint32(0)
    lib.mp_plan_aov_pass(C.byref(pp.launch(facts, frame[0], frame[1], spp, passes, **kw)), 1 if wide else 0, C.byref(out), C.byref(park))
    return out, park.value


def kernel(facts, frame, spp, passes=None, wide=True, **kw):
    out, _ = plan(facts, frame, spp, wide, passes, **kw)
    assert out.rc == 0, out.error
    return pp.name(out)


def test_wide_park_geometry():
    # 24 x 16 in 16 x 16 tiles, S = 16 cached: 4 waves x 4 pixels x 48 bytes in front of the mask cache
    o, park = plan(TEAPOT, (2, 16), 64, True)
    assert (o.rc, o.grid, o.lds, o.lds_per_wave, park) == (0, 32, 768 + 14848, 0, 48)
    o, park = plan(TEAPOT, (2, 16), 16, True)  # S = 4 cached: 16 pixels per wave
    assert (o.grid, o.lds, park) == (8, 3072 + 14848, 48)
    o, park = plan(TEAPOT, FRAME, 3, True)  # S = 1: 64 pixels per wave, nothing behind the park
    assert (o.grid, o.lds, park) == (2048, 12288, 48)
    # the narrow park through the new function is the old plan, field for field
    for frame, spp in (((2, 16), 64), ((2, 16), 16), (FRAME, 3)):
        o, park = plan(TEAPOT, frame, spp, False)
        old = pp.plan(pp.AOV, pp.launch(TEAPOT, frame[0], frame[1], spp))
        assert park == 32 and bytes(o) == bytes(old)
    assert plan(TEAPOT, (2, 16), 64, False)[0].lds == 512 + 14848


def test_stack_refusal_boundary_with_the_wide_park():
    # S = 16, 64 entries in registers: (2612 - 64) x 16 x 4 = 163 072 bytes of stack + 768 of park = 163 840 = all of the CU's LDS
    assert (2612 - 64) * 64 + 768 == 160 * 1024
    o, _ = plan({**TEAPOT, "stack_bound": 2612}, FRAME, 16, True)
    assert (o.rc, o.lds, pp.name(o)) == (0, 163840, A + "<16, true, 8>")
    o, _ = plan({**TEAPOT, "stack_bound": 2613}, FRAME, 16, True)
    assert (o.rc, o.error.decode()) == (pp.MP_ERR_UNSUPPORTED, STACK)
    # the narrow park keeps its boundary (tests/test_launch_plan_cpu.py: 2616 / 2617)
    assert plan({**TEAPOT, "stack_bound": 2616}, FRAME, 16, False)[0].rc == 0
    o, _ = plan({**TEAPOT, "stack_bound": 2617}, FRAME, 16, False)
    assert (o.rc, o.error.decode()) == (pp.MP_ERR_UNSUPPORTED, STACK)
    assert plan({**TEAPOT, "stack_bound": 2616}, FRAME, 16, True)[0].rc == pp.MP_ERR_UNSUPPORTED


# the passes tests/test_gpu_aov_passes.py runs on the teapot at 70 samples per pixel, and the kernel of each
SPLITS = {
    (40, 17, 8, 4, 1): ["<4, false, 8, false, true>", "<4, false, 8, false, true>", "<4, false, 8>", "<4, false, 8>", "<1, false, 8>"],
    (64, 6): ["<16, false, 8, false, true>", "<4, false, 8>"],
    (1, 69): ["<1, false, 8>", "<16, false, 8, false, true>"],
    (40, 17, 13): ["<4, false, 8, false, true>", "<4, false, 8, false, true>", "<4, false, 8>"],
}


@pytest.mark.parametrize("wide", [False, True])
def test_the_kernel_follows_the_samples_of_the_pass(wide):
    small = (6, 32)  # 72 x 40 in tiles of 32
    for frame in (FRAME, small):
        assert kernel(TEAPOT, frame, 70, wide=wide) == A + "<16, false, 8, false, true>"
        for count, name in ((40, "<4, false, 8, false, true>"), (8, "<4, false, 8>"), (1, "<1, false, 8>")):
            assert kernel(TEAPOT, frame, 70, passes=(16, count), wide=wide) == A + name, count
    for split, names in SPLITS.items():
        assert sum(split) == 70
        begin = 0
        for count, name in zip(split, names):
            assert kernel(TEAPOT, small, 70, passes=(begin, count), wide=wide) == A + name, (split, begin)
            begin += count
    # object groups and LDS stacks: 16 or 1, by the pass
    for facts, kw, tail in ((GROUP_RGB, {}, "false, 6, true>"), (GROUP_RGB, {"regs": 21}, "true, 6, true>"), (TEAPOT, {"regs": 21}, "true, 8>")):
        assert kernel(facts, FRAME, 70, wide=wide, **kw) == A + "<16, " + tail
        assert kernel(facts, FRAME, 70, passes=(3, 16), wide=wide, **kw) == A + "<16, " + tail
        assert kernel(facts, FRAME, 70, passes=(3, 15), wide=wide, **kw) == A + "<1, " + tail
        assert kernel(facts, FRAME, 70, passes=(69, 1), wide=wide, **kw) == A + "<1, " + tail
    # the rows of the census, as whole-frame passes with all six planes: their own names
    for name, row in dc.CASES.items():
        if row["api"] == "aov":
            lib_in = pp.row_input(row)
            out, park = pp.PlanOut(), C.c_uint32(0)
            pp.lib().mp_plan_aov_pass(C.byref(lib_in), 1 if wide else 0, C.byref(out), C.byref(park))
            assert out.rc == 0 and pp.name(out) == name and park.value == (48 if wide else 32)


def test_bindings():
    from minipath_amd import _lib

    L = _lib.lib()
    assert L.mp_render_aov_pass_device is not None
    assert C.sizeof(_lib.AovPlanesEx) == L.mp_aov_planes_ex_size() == 56
    assert [n for n, _ in _lib.AovPlanesEx._fields_] == ["struct_size", "d_shade", "d_normal", "d_albedo", "d_ids", "d_position", "d_shade_sq"]
    assert _lib.AovPlanesEx.d_shade.offset == 8 and _lib.AovPlanesEx.d_shade_sq.offset == 48
    import minipath_amd as mp

    assert mp.FrameRenderer.AOV_PLANES == aov_pass_model.PLANES


def test_model_agrees_with_the_four_plane_model(oracle):
    orc = oracle.Bvh.from_obj(TEAPOT_OBJ)
    import minipath_amd as mp

    res, spp, seed = (6, 4), 3, 11
    smp = oracle.sampler_from_array(mp.Camera.teapot_view().build_sampler(res).as_array())
    block = (0, 0, res[0], res[1])
    frame = aov_pass_model.Frame(oracle, orc.intersect, smp, res[0], spp, seed, block)
    old = aov_model.planes(oracle, orc.intersect, smp, res[0], spp, seed, block)
    assert 0 < frame.hit.sum() < frame.hit.size
    new, state, inv = frame.planes(), frame.state_after(spp), F(1) / F(spp)
    for k in ("shade", "normal", "albedo", "ids"):
        assert np.array_equal(bits(new[k]), bits(old[k])), k
    for k in aov_pass_model.FLOAT_PLANES:
        assert np.array_equal(bits((state[k] * inv).astype(F)), bits(new[k])), k
    # the state is sums: hit counts are whole numbers, and grow with k
    s2 = frame.state_after(2)
    assert np.array_equal(s2["shade"][..., 3], frame.hit[..., :2].sum(axis=2).astype(F))
    assert np.all(s2["position"][..., 3] <= state["position"][..., 3])
    # position: alpha-weighted points lie inside the teapot's bounds where every sample hit
    full = new["position"][..., 3] == 1.0
    assert full.any() and np.all(np.abs(new["position"][full][:, :3]) < 10.0)


def test_shade_sq_is_not_the_square_of_shade():
    """Two samples of one pixel: the plane is (F(c0 * c0) + F(c1 * c1)) / 2, the second moment -- not ((c0 + c1) / 2) ** 2."""
    c = [F(0.25), F(0.75)]
    n, z3 = np.array([0, 0, 1], F), np.zeros(3, F)
    vals = np.stack([aov_pass_model.sample_values(ci, n, 1.0, z3, z3) for ci in c])
    acc = aov_pass_model.ordered_sum(vals)
    px = aov_pass_model._pack(acc, 2, F(1) / F(2))
    assert px["shade"][0] == F(0.5) and px["shade_sq"][0] == F(0.3125)
    assert px["shade_sq"][0] != F(px["shade"][0] * px["shade"][0])  # 0.25
    assert F(px["shade_sq"][0] - F(px["shade"][0] * px["shade"][0])) == F(0.0625)  # the variance of {0.25, 0.75}
    # one rounded product per sample: F(c * c) of a value whose square is not representable
    c3 = F(1) / F(3)
    v = aov_pass_model.sample_values(c3, n, 1.0, z3, z3)
    assert v[11] == F(c3 * c3) and float(v[11]) != float(c3) * float(c3)
    assert aov_pass_model.shade_of((0.0, 0.6, -0.8), (0.0, 0.0, 1.0)) == F(0.8)


def test_checkpoint_round_trip_with_planes(tmp_path):
    import torch

    from minipath_amd import io

    blocks = [types.SimpleNamespace(min_x=0, min_y=0, max_x=16, max_y=16), types.SimpleNamespace(min_x=16, min_y=0, max_x=24, max_y=16)]

    def renderer(spp=70):
        st = types.SimpleNamespace(resolution=(24, 16), tile_size=16, sample_count=spp, seed=5, max_depth=0)
        return types.SimpleNamespace(tiles=blocks, settings=st, tile_buf=torch.zeros((2, 16, 16, 4), dtype=torch.float32))

    rng = np.random.default_rng(1)
    src = renderer()
    src.tile_buf.copy_(torch.from_numpy(rng.random((2, 16, 16, 4), dtype=np.float32)))
    planes = {"shade": torch.from_numpy(rng.random((2, 16, 16, 4), dtype=np.float32)),
              "position": rng.standard_normal((2, 16, 16, 4)).astype(F),  # a numpy stand-in beside a tensor
              "ids": torch.from_numpy(rng.integers(-1, 1 << 30, (2, 16, 16, 4)).astype(np.int32))}
    ck = str(tmp_path / "ck.npz")
    io.save_checkpoint(ck, src, 17, planes=planes)
    dst = renderer()
    fresh = {"shade": torch.zeros((2, 16, 16, 4)), "position": np.zeros((2, 16, 16, 4), F), "ids": torch.zeros((2, 16, 16, 4), dtype=torch.int32)}
    assert io.load_checkpoint(ck, dst, planes=fresh) == 17
    assert torch.equal(dst.tile_buf, src.tile_buf)
    for k in planes:
        a, b = (np.asarray(v) if isinstance(v, np.ndarray) else v.numpy() for v in (planes[k], fresh[k]))
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
    # without planes= the file reads as before; the planes are refused as a set, by shape and dtype, and for other settings
    assert io.load_checkpoint(ck, renderer()) == 17
    with pytest.raises(ValueError, match="planes"):
        io.load_checkpoint(ck, renderer(), planes={"shade": fresh["shade"]})
    with pytest.raises(ValueError, match="shape or dtype"):
        io.load_checkpoint(ck, renderer(), planes={**fresh, "ids": torch.zeros((2, 16, 16, 4))})
    untouched = {k: (v.copy() if isinstance(v, np.ndarray) else v.clone().zero_()) for k, v in fresh.items()}
    untouched["position"][...] = 0
    with pytest.raises(ValueError, match="other settings"):
        io.load_checkpoint(ck, renderer(spp=71), planes=untouched)
    assert all(not np.asarray(v).any() for v in untouched.values())
    # a checkpoint without planes, as before this argument existed
    ck2 = str(tmp_path / "ck2.npz")
    io.save_checkpoint(ck2, src, 3)
    with np.load(ck2) as z:
        assert sorted(z.files) == ["next_sample", "settings", "sums", "tiles"]
    with pytest.raises(ValueError, match="planes"):
        io.load_checkpoint(ck2, renderer(), planes=fresh)
