"""ray_math.h's short normalisation of a shading normal (unit_normal: sqrt_short, one div_rcp, three div_short with the numerator's
sign copied on) on the GPU through libmp_probe.so, bit for bit against sqrtf and the three `/` the compiler emits: random normals,
normals with +0 and -0 components (walls along the axes), waves in which one lane carries a component outside the window -- or three
zeros -- and which therefore must fall back as a whole, and components of random bits."""
import ctypes as C
import os

import pytest

SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minipath_amd", "csrc", "libmp_probe.so")
BLOCKS = 1 << 12  # x 256 normals: 2^14 waves, every kind of odd lane 2^10 times


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_unit_normal_against_plain_formulas(mode):
    import torch  # (before the probe: the probe's HIP runtime loaded first would hide the GPU from a torch imported later)

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run build() first")
    L = C.CDLL(SO)
    L.mp_probe_normal.argtypes = [C.c_uint64, C.c_int, C.c_uint64, C.c_void_p]
    o = (C.c_ulonglong * 4)()
    rc = L.mp_probe_normal(0xBEEF + mode, mode, BLOCKS, o)
    assert rc == 0, f"HIP error {rc}"
    waves = BLOCKS * 4
    print(f"mode {mode}: {o[1]} normals, {o[0]} mismatches, {o[3]} of {waves} waves short")
    assert o[1] == BLOCKS * 256
    assert o[0] == 0, f"{o[0]} mismatches, first normal {o[2]}"
    if mode in (0, 1):
        assert o[3] == waves  # inside the window, zeros of either sign included: every wave takes the short path
    elif mode == 2:
        assert o[3] == waves // 2  # exactly the waves with an odd lane fall back
    else:
        assert o[3] < waves // 100  # random bits: hardly a wave is all inside the window
