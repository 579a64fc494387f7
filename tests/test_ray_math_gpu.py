"""ray_math.h's short IEEE division / sqrt sequences on the GPU (libmp_probe.so, built with the library's device flags), bit for bit
against the compiler's `/` and sqrtf: every f32 input of sqrt and of the reciprocal inside their windows, 2^30 division pairs inside
the division window, and Ray::new's guarded form (ray_dir) against the plain formulas, with waves that must fall back."""
import ctypes as C
import os

import pytest

SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minipath_amd", "csrc", "libmp_probe.so")


def _lib():
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run build() first")
    L = C.CDLL(SO)
    L.mp_probe_unary.argtypes = [C.c_int, C.c_void_p]
    L.mp_probe_div.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    L.mp_probe_ray.argtypes = [C.c_uint64, C.c_int, C.c_uint64, C.c_void_p]
    return L


def _out():
    return (C.c_ulonglong * 4)()


# inputs inside the window: sqrt [2^-96, FLT_MAX], exponents -96..127; reciprocal |x| in [2^-94, 2^125], exponents -94..124 and
# 2^125 itself, both signs
@pytest.mark.gpu
@pytest.mark.parametrize("op,inside", [(0, (127 + 96 + 1) * 2**23), (1, 2 * ((124 + 94 + 1) * 2**23 + 1))])
def test_sqrt_and_reciprocal_every_input(op, inside):
    L = _lib()
    o = _out()
    rc = L.mp_probe_unary(op, o)
    assert rc == 0, f"HIP error {rc}"
    assert o[0] == 0, f"{o[0]} mismatches, first input bits {o[2]:#010x}"
    assert o[1] == inside


@pytest.mark.gpu
def test_division_window_pairs():
    L = _lib()
    o = _out()
    rc = L.mp_probe_div(0x5EED, 1 << 16, o)  # 2^16 blocks x 256 threads x 64 pairs = 2^30, in launches of 2^26
    assert rc == 0, f"HIP error {rc}"
    assert o[1] == 1 << 30
    assert o[0] == 0, f"{o[0]} mismatches, first pair index {o[2]}"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_ray_dir_against_plain_formulas(mode):
    L = _lib()
    o = _out()
    blocks = 1 << 16
    rc = L.mp_probe_ray(0xC0FFEE + mode, mode, blocks, o)
    assert rc == 0, f"HIP error {rc}"
    waves = blocks * 4
    assert o[1] == blocks * 256
    assert o[0] == 0, f"{o[0]} mismatches, first ray {o[2]}"
    if mode == 0:
        assert o[3] == waves  # every wave in the window takes the short path
    elif mode == 1:
        assert o[3] == waves // 2  # exactly the waves with an odd lane fall back
    else:
        assert o[3] < waves // 100  # random bits: hardly a wave is all inside the window
