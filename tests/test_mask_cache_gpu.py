"""The packet walk's mask-cache predicates (minipath_amd/csrc/mask_cache.h) on the GPU, through libmp_mask_probe.so (built with the
library's device flags).  Each probe generates its cases on the device and checks the very functions the walk inlines:

* tri_may_hit and bounds_may_hit<OCT> against the walk's per-ray arithmetic (Moeller-Trumbore with fms / fma_dot, the slab test) of
  192 rays inside the unit's bounds B: its 64 corners, those corners one ulp inward, and 64 interior points -- the predicate may
  reject a case only if none of them hits;
* mask_cache_ray_ok against its plain definition for every f32 bit pattern in each component, bounds_deviation against
  `v < lo || v > hi`;
* mask_cache_begin_pass against a serial restatement of its rule over sequences of passes;
* the per-ray reference itself against the CPU oracle's aabb8 / tri8 intersection, bit for bit, on dumped cases.

Coverage counters keep the probes from passing vacuously: cases some ray hits, cases the predicate rejects, and edge-only cases (hit
by a corner or inward ray and by no interior ray).  The lower bounds are a quarter of what the fixed seeds give, or less."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minipath_amd", "csrc", "libmp_mask_probe.so")
NCASES = 1 << 22
RAYS = 192
HEAD, RAY = 40, 10
FLT_MAX = np.float32(3.4028234663852886e38)


def _lib():
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run build() first")
    L = C.CDLL(SO)
    L.mp_mask_probe_tri.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    L.mp_mask_probe_box.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    L.mp_mask_probe_ray_ok.argtypes = [C.c_uint64, C.c_void_p]
    L.mp_mask_probe_dev.argtypes = [C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    L.mp_mask_probe_pass.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    L.mp_mask_probe_dump.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    L.mp_mask_probe_dump_dwords.restype = C.c_int
    return L


def _out():
    return (C.c_ulonglong * 8)()


def _report(name, o):
    print(f"{name}: violations {o[0]} cases {o[1]} first {o[2]:#x} hit {o[3]} rejected {o[4]} edge-only {o[5]} rewrites {o[6]}")


def test_tri_may_hit_corners():
    L = _lib()
    o = _out()
    rc = L.mp_mask_probe_tri(0x7A1, NCASES, o)
    assert rc == 0, f"HIP error {rc}"
    _report("tri_may_hit", o)
    assert o[1] == NCASES
    assert o[0] == 0, f"{o[0]} cases rejected although a ray inside B hits; first case {o[2]}"
    # (seed 0x7A1: 19.6 % hit, 10.6 % rejected, 4.7 % edge-only)
    assert o[3] >= NCASES // 24, "too few cases where some ray hits"
    assert o[4] >= NCASES // 40, "too few rejected cases"
    assert o[5] >= NCASES // 100, "too few edge-only cases"


def test_bounds_may_hit_corners_all_patterns():
    L = _lib()
    o = _out()
    rc = L.mp_mask_probe_box(0xB0C5, NCASES, o)
    assert rc == 0, f"HIP error {rc}"
    _report("bounds_may_hit", o)
    assert o[1] == NCASES
    assert o[0] == 0, f"{o[0]} cases rejected although a ray inside B passes the box; first case {o[2]} (pattern {o[2] & 7})"
    # (seed 0xB0C5: 71.8 % pass, 19.1 % rejected, 19.0 % edge-only)
    assert o[3] >= NCASES // 6, "too few cases where some ray passes"
    assert o[4] >= NCASES // 20, "too few rejected cases"
    assert o[5] >= NCASES // 20, "too few edge-only cases"


def _boundary_set():
    f = np.float32
    base = [0.0, 2.0**-149, f(2.0**-126) - f(2.0**-149), 2.0**-126, 0.5, 1.0, 2.0, 2.0**30, 2.0**31, float(FLT_MAX)]
    vals = set()
    for b in base:
        for s in (1.0, -1.0):
            x = f(s * b)
            with np.errstate(over="ignore"):  # FLT_MAX's upper neighbour is inf (dropped below)
                vals.update({x, np.nextafter(x, f(np.inf)), np.nextafter(x, f(-np.inf))})
    vals.update({f(-0.0)})
    arr = np.array(sorted(vals, key=lambda v: (float(v), np.signbit(v))), np.float32)
    arr = arr[np.isfinite(arr)]
    # +0 and -0 both (the set above holds one of them)
    return np.unique(np.concatenate([arr, np.array([0.0, -0.0], np.float32)]).view(np.uint32)).view(np.float32)


def test_pass_entry_ray_ok_and_deviation():
    L = _lib()
    o = _out()
    rc = L.mp_mask_probe_ray_ok(0x0C, o)
    assert rc == 0, f"HIP error {rc}"
    _report("mask_cache_ray_ok", o)
    assert o[1] == 9 << 32
    assert o[0] == 0, f"{o[0]} disagreements with the plain definition; first: component {o[2] >> 32}, bits {o[2] & 0xFFFFFFFF:#010x}"

    s = _boundary_set()
    assert np.any(s.view(np.uint32) == 0x80000000) and np.any(s.view(np.uint32) == 0)
    o = _out()
    nrand = 1 << 26
    rc = L.mp_mask_probe_dev(0xDE7, s.ctypes.data, len(s), nrand, o)
    assert rc == 0, f"HIP error {rc}"
    _report("bounds_deviation", o)
    n = len(s)
    valid = sum(1 for lo in s for hi in s if lo <= hi) * n
    assert o[1] >= valid + nrand // 2
    assert o[0] == 0, f"{o[0]} disagreements with v < lo || v > hi; first triple index {o[2]:#x}"


def test_begin_pass_rule():
    L = _lib()
    o = _out()
    nwaves = 1 << 14
    rc = L.mp_mask_probe_pass(0xBE61, nwaves, o)
    assert rc == 0, f"HIP error {rc}"
    _report("mask_cache_begin_pass", o)
    assert o[1] == nwaves * 64
    assert o[0] == 0, f"{o[0]} passes break the rule; first: wave {o[2] // 64}, pass {o[2] % 64}"
    assert o[1] // 8 <= o[6] <= o[1] - o[1] // 8, "both rewriting and keeping passes must occur often"


def _dump(L, kind, seed, n):
    dw = L.mp_mask_probe_dump_dwords()
    assert dw == HEAD + RAYS * RAY
    buf = np.zeros((n, dw), np.uint32)
    o = _out()
    rc = L.mp_mask_probe_dump(kind, seed, n, buf.ctypes.data, o)
    assert rc == 0, f"HIP error {rc}"
    assert o[1] == n and o[0] == 0
    return buf


def _same(a, b, zero_sign=False):
    """bitwise, NaN == NaN (payloads differ between the two ISAs); with zero_sign, +0 == -0"""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    eq = a.view(np.uint32) == b.view(np.uint32)
    eq |= np.isnan(a) & np.isnan(b)
    if zero_sign:
        eq |= (a == 0) & (b == 0)
    return eq


NDUMP = 2048


def test_per_ray_reference_matches_oracle(oracle):
    """The probes' per-ray reference is the oracle's arithmetic: every dumped ray replayed through aabb8 / tri8 intersect."""
    L = _lib()
    O = oracle.lib()
    ray = oracle.Ray()
    f8 = lambda: np.zeros((3, 8), np.float32)  # noqa: E731
    # triangles: the case's vertices in lane 0; the oracle forms the edges itself
    tri = _dump(L, 0, 0x7A1, NDUMP)
    v0, v1, v2 = f8(), f8(), f8()
    t, u, v = np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(8, np.float32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    pv0, pv1, pv2, pt, pu, pv = p(v0), p(v1), p(v2), p(t), p(u), p(v)
    hits = 0
    for c in range(NDUMP):
        head = tri[c, :HEAD].view(np.float32)
        v0[:, 0], v1[:, 0], v2[:, 0] = head[20:23], head[23:26], head[26:29]
        e1, e2 = head[29:32], head[32:35]
        assert np.array_equal((v1[:, 0] - v0[:, 0]).view(np.uint32), e1.view(np.uint32))
        assert np.array_equal((v2[:, 0] - v0[:, 0]).view(np.uint32), e2.view(np.uint32))
        rays = tri[c, HEAD:].reshape(RAYS, RAY)
        rf = rays.view(np.float32)
        got = np.zeros((RAYS, 3), np.float32)
        ghit = np.zeros(RAYS, bool)
        for j in range(RAYS):
            for k in range(3):
                ray.o[k] = float(rf[j, k])
                ray.d[k] = float(rf[j, 3 + k])
                ray.inv[k] = 0.0  # (not read by the triangle test)
            m = O.mpo_tri8_intersect(pv0, pv1, pv2, C.byref(ray), pt, pu, pv)
            got[j] = (t[0], u[0], v[0])
            ghit[j] = bool(m & 1) and t[0] >= 0
        ok = _same(rf[:, 6:9], got).all(axis=1) & (ghit == (rays[:, 9] == 1))
        hits += int(ghit.sum())
        if not ok.all():
            j = int(np.argmin(ok))
            pytest.fail(f"triangle case {c} ray {j}: device t,u,v,hit {rf[j, 6:9]} {rays[j, 9]} oracle {got[j]} {ghit[j]}")
    assert hits > 0
    # boxes: lane 0, limit FLT_MAX
    box = _dump(L, 1, 0xB0C5, NDUMP)
    bmin, bmax = f8(), f8()
    t1, t2 = np.zeros(8, np.float32), np.zeros(8, np.float32)
    pmin, pmax, pt1, pt2 = p(bmin), p(bmax), p(t1), p(t2)
    passes = 0
    for c in range(NDUMP):
        head = box[c, :HEAD].view(np.float32)
        bmin[:, 0], bmax[:, 0] = head[20:23], head[23:26]
        assert box[c, 26] == c & 7
        rf = box[c, HEAD:].reshape(RAYS, RAY).view(np.float32)
        got = np.zeros((RAYS, 2), np.float32)
        for j in range(RAYS):
            for k in range(3):
                ray.o[k] = float(rf[j, k])
                ray.inv[k] = float(rf[j, 3 + k])
                ray.d[k] = 0.0  # (not read by the slab test)
            O.mpo_aabb8_intersect(pmin, pmax, C.byref(ray), C.c_float(FLT_MAX), pt1, pt2)
            got[j] = (t1[0], t2[0])
        # the oracle's min / max are x86's (second operand on ties), the device's IEEE minNum / maxNum: +-0 may differ in sign only
        ok = _same(rf[:, 6:8], got, zero_sign=True).all(axis=1)
        gpass = got[:, 0] <= got[:, 1]
        ok &= gpass == (box[c, HEAD:].reshape(RAYS, RAY)[:, 9] == 1)
        passes += int(gpass.sum())
        if not ok.all():
            j = int(np.argmin(ok))
            pytest.fail(f"box case {c} ray {j}: device t1,t2 {rf[j, 6:8]} oracle {got[j]}")
    assert passes > 0
