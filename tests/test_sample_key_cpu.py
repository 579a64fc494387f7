"""The sample key as the cached packet kernels form it per pass -- the pixel's key at sample 0 plus the sample index, on 32-bit
halves (ray_math.h: sample_key_u64, key_add_sample; compiled for the host in libmp_rm_host.so) -- against the 64-bit formula
seed + ((y * width + x) * spp + s) in numpy: two million random tuples, and tuples chosen so that the low word of the key at sample 0
plus s carries into the high word, so that the whole key wraps 2^64, and so that the index part alone passes 2^32 and 2^64."""
import ctypes as C
import os

import numpy as np
import pytest

SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minipath_amd", "csrc", "libmp_rm_host.so")
U32, U64 = np.uint32, np.uint64


def _keys(seed, width, spp, x, y, s):
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run build() first")
    L = C.CDLL(SO)
    L.mp_rm_sample_keys.argtypes = [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_void_p]
    arrs = [np.ascontiguousarray(seed, U64)] + [np.ascontiguousarray(a, U32) for a in (width, spp, x, y, s)]
    n = len(arrs[0])
    assert all(len(a) == n for a in arrs)
    formula, stepped = np.zeros(n, U64), np.zeros(n, U64)
    L.mp_rm_sample_keys(*[a.ctypes.data for a in arrs], n, formula.ctypes.data, stepped.ctypes.data)
    return formula, stepped


def _formula(seed, width, spp, x, y, s):
    """the 64-bit formula in numpy (u64 arithmetic wraps mod 2^64, as the reference's wrapping adds and multiplies do)"""
    with np.errstate(over="ignore"):
        return seed.astype(U64) + ((y.astype(U64) * width.astype(U64) + x.astype(U64)) * spp.astype(U64) + s.astype(U64))


def _check(seed, width, spp, x, y, s):
    formula, stepped = _keys(seed, width, spp, x, y, s)
    want = _formula(seed, width, spp, x, y, s)
    assert np.array_equal(formula, want), "the host build's formula"
    bad = np.flatnonzero(stepped != want)
    assert bad.size == 0, (bad.size, [int(a[bad[0]]) for a in (seed, width, spp, x, y, s)])
    return want


def test_two_million_random_tuples():
    rng = np.random.default_rng(20)
    n = 2_000_000
    seed = rng.integers(0, 2**64 - 1, n, dtype=U64, endpoint=True)
    # images and sample counts of every size a u32 holds, half of them of plausible size
    big = rng.random(n) < 0.5
    width = np.where(big, rng.integers(0, 2**32, n, dtype=U64), rng.integers(1, 8192, n, dtype=U64)).astype(U32)
    spp = np.where(big, rng.integers(0, 2**32, n, dtype=U64), rng.integers(1, 4096, n, dtype=U64)).astype(U32)
    x = (rng.integers(0, 2**32, n, dtype=U64) % np.maximum(width, 1).astype(U64)).astype(U32)
    y = np.where(big, rng.integers(0, 2**32, n, dtype=U64), rng.integers(0, 8192, n, dtype=U64)).astype(U32)
    s = (rng.integers(0, 2**32, n, dtype=U64) % np.maximum(spp, 1).astype(U64)).astype(U32)
    _check(seed, width, spp, x, y, s)


def test_wraps_of_the_low_word_and_of_the_key():
    """seeds placed so that key(x, y, 0) sits just below a multiple of 2^32, or just below 2^64, and s steps across it"""
    rng = np.random.default_rng(21)
    n = 4096
    width, spp = rng.integers(1, 4096, n).astype(U32), rng.integers(1, 1024, n).astype(U32)
    x, y = rng.integers(0, 4096, n).astype(U32) % width, rng.integers(0, 4096, n).astype(U32)
    zero = np.zeros(n, U32)
    index0 = _formula(np.zeros(n, U64), width, spp, x, y, zero)  # (y * width + x) * spp
    s = rng.integers(0, 2048, n).astype(U32)
    back = rng.integers(0, 2048, n).astype(U64)  # key at sample 0 = boundary - back; the samples with s >= back are past it
    with np.errstate(over="ignore"):
        for boundary in (U64(1) << U64(32), U64(5) << U64(32), U64(0)):  # 2^32, a later multiple of it, and 2^64 = 0 mod 2^64
            seed = boundary - back - index0
            key = _check(seed, width, spp, x, y, s)
            key0 = _formula(seed, width, spp, x, y, zero)
            assert np.array_equal(key0, boundary - back)
            crossed = s.astype(U64) >= back
            assert crossed.any() and (~crossed).any(), "samples on both sides of the wrap"
            assert np.array_equal((key >> U64(32)) != (key0 >> U64(32)), crossed & (back > 0)), "the carry into the high word"
    # the largest operands: the index part alone wraps 2^64
    top = np.full(n, 0xFFFFFFFF, U32)
    _check(rng.integers(0, 2**64 - 1, n, dtype=U64, endpoint=True), top, top, top - rng.integers(0, 4, n).astype(U32), top,
           top - rng.integers(0, 4, n).astype(U32))


def test_index_part_around_two_to_the_32():
    """(y * width + x) * spp + s just below, at and above 2^32: where a lane offset of 32 bits would stop holding the index, the sum
    with the key at sample 0 still carries on"""
    n = 2048
    rng = np.random.default_rng(22)
    spp = np.full(n, 256, U32)
    width = np.full(n, 1 << 23, U32)
    y = np.full(n, 1, U32)  # y * width * spp = 2^31
    x = ((1 << 23) - 1 - rng.integers(0, 4, n)).astype(U32)  # (y * width + x) * spp = 2^32 - 256 * (1 + 0..3)
    s = rng.integers(0, 256, n).astype(U32)
    key = _check(np.zeros(n, U64), width, spp, x, y, s)
    assert key.max() < 2**32
    x2 = (x.astype(U64) + U64(4)).astype(U32)  # past the end of the row: the same integer as the next row's pixels, 2^32 and above
    key = _check(np.zeros(n, U64), width, spp, x2, y, s)
    assert key.min() >= 2**32 - 256 and (key >= 2**32).any()
