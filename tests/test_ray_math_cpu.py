"""ray_math.h's RNG on 32-bit halves (compiled for the host, v_alignbit_b32 emulated) against the plain 64-bit formulas of
SplitMix64 seeding and Xoshiro256++ in numpy, including keys that wrap 2^64 while seeding, and UnitDisc in both loop forms."""
import ctypes as C
import os

import numpy as np
import pytest

SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minipath_amd", "csrc", "libmp_rm_host.so")
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _lib():
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run build() first")
    L = C.CDLL(SO)
    L.mp_rm_draws.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.mp_rm_unit_disc.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    return L


def _rotl(x, k):
    return (x << np.uint64(k)) | (x >> np.uint64(64 - k))


def _seed(keys):
    st = keys.copy()
    s = []
    with np.errstate(over="ignore"):
        for _ in range(4):
            st = st + np.uint64(0x9E3779B97F4A7C15)
            z = st
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            s.append(z ^ (z >> np.uint64(31)))
    return s


def _next(s):
    with np.errstate(over="ignore"):
        res = _rotl(s[0] + s[3], 23) + s[0]
    t = s[1] << np.uint64(17)
    s[2] ^= s[0]
    s[3] ^= s[1]
    s[1] ^= s[2]
    s[0] ^= s[3]
    s[2] ^= t
    s[3] = _rotl(s[3], 45)
    return (res >> np.uint64(32)).astype(np.uint32)


def _keys(n, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)
    edge = np.concatenate([
        M64 - np.arange(4096, dtype=np.uint64),                                # wraps on the first add
        (np.uint64(2**64 - 4 * 0x9E3779B97F4A7C15 % 2**64) + np.arange(-2048, 2048).astype(np.int64).astype(np.uint64)),  # wraps on the 4th
        np.arange(4096, dtype=np.uint64),
        np.uint64(0xFFFFFFFF) + np.arange(-2048, 2048).astype(np.int64).astype(np.uint64),  # carries between the halves
    ])
    return np.concatenate([edge, k])


def test_draws_match_64bit_formulas():
    L = _lib()
    keys = _keys(2_000_000, 1)
    draws = 6
    out = np.zeros((keys.size, draws), np.uint32)
    L.mp_rm_draws(keys.ctypes.data, keys.size, draws, out.ctypes.data)
    s = _seed(keys)
    for j in range(draws):
        ref = _next(s)
        bad = np.flatnonzero(out[:, j] != ref)
        assert bad.size == 0, f"draw {j}: {bad.size} mismatches, first key {int(keys[bad[0]]):#x}"


def _f01(v):
    return ((np.uint32(0x3F800000) | (v >> np.uint32(9))).view(np.float32) - np.float32(1.0)).astype(np.float32)


def test_unit_disc_both_forms():
    L = _lib()
    keys = _keys(300_000, 2)
    n = keys.size
    xy = np.zeros((n, 4), np.float32)
    nxt = np.zeros((n, 2), np.uint32)
    L.mp_rm_unit_disc(keys.ctypes.data, n, xy.ctypes.data, nxt.ctypes.data)
    # numpy: the rejection loop on the streams not yet accepted (f32 products and sums, unfused)
    s = _seed(keys)
    x1 = np.zeros(n, np.float32)
    x2 = np.zeros(n, np.float32)
    after = np.zeros(n, np.uint32)
    todo = np.arange(n)
    for _ in range(64):
        sub = [v[todo] for v in s]
        a = _f01(_next(sub)) * np.float32(2.0) + np.float32(-1.0)
        b = _f01(_next(sub)) * np.float32(2.0) + np.float32(-1.0)
        acc = a * a + b * b <= np.float32(1.0)
        for i in range(4):
            s[i][todo] = sub[i]
        g = todo[acc]
        x1[g], x2[g] = a[acc], b[acc]
        after[g] = _next([v[acc] for v in sub])
        todo = todo[~acc]
        if todo.size == 0:
            break
    assert todo.size == 0
    assert np.array_equal(xy[:, 0].view(np.uint32), x1.view(np.uint32))
    assert np.array_equal(xy[:, 1].view(np.uint32), x2.view(np.uint32))
    assert np.array_equal(xy[:, 2:], xy[:, :2])
    assert np.array_equal(nxt[:, 0], after)
    assert np.array_equal(nxt[:, 1], after)
