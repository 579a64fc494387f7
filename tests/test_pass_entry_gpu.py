"""GPU tests (-m gpu) of the one-test pass entry of the cached packet kernels (mask_cache.h, mask_cache_pass_inside; packet_walk.h,
trace_packet): a pass whose every active ray lies inside a valid B enters the cached walk of B's pattern without mask_cache_ray_ok,
the sign ballots and mask_cache_begin_pass; every other pass takes the full route.

* The decision, through libmp_mask_probe.so (mp_mask_probe_entry: one wave per hand-made pass), against its plain definition --
  "the header is valid, and lo <= v <= hi for each of the nine components of every active ray" -- which a NaN fails by itself:
  all rays inside B (interior, on the faces, -0 where a bound is 0), one ray one ulp outside in each component on either side, a NaN
  and both infinities in each component, an origin of 1.5 x 2^30 inside B (a ray mask_cache_ray_ok refuses: it now takes the
  cached walk), an inverse direction of the wrong sign, inactive lanes holding garbage, no active lane, and headers that are not
  valid (none, a pattern without the valid bit, stray bits).  Under each of the eight patterns.
* Frames against the oracle's bits at 96 x 64, 64 samples, on render_tiles_packet_kernel<16, ..., true> (four passes per unit): the
  teapot (units that miss, silhouette units and interior units), the teapot's camera turned away, and the stand-in through a lens
  2.5 m across, whose units decline to set bounds from their corner rays or leave them (an invalid header at the first pass,
  escapes and mixed signs after).
* The same three frames in the counted build libminipath_hip_noskip.so (-DMP_PROF_MISSES; its own switch concerns the walk, not the
  entry), in a process of its own (tests/walk_frames.py, run_in_variant): `passes_bounds_entry` and `passes_full_entry` are the passes that
  enter the cached walk on the one bounds test and those that enter it through the full guards.  A unit has four passes here, so both are bounded by 4 x units.  The teapot:
  its units set B from their corner rays, so passes that reach the walk find themselves inside B: the short route occurs.  The
  wide lens: units that decline to set B send their first pass through the full guards, which sets B with a quarter of its extent
  to spare, so both routes occur.  The camera turned away: the per-ray pre-test stops every pass before the walk, neither occurs."""
import ctypes as C
import os

import numpy as np
import pytest

import minipath_amd as mp
from minipath_amd import _lib
from tests.walk_frames import CSRC, Counters, assert_same_bits, cameras, differing, frame, make_objects, oracle_frame, run_in_variant

pytestmark = pytest.mark.gpu

SO = os.path.join(CSRC, "libmp_mask_probe.so")
STATE, NO = 12, 8  # the header's state dword; "no pattern"
LO = {0: 0, 1: 6, 2: 13}  # header slot of group g's minima (origin, inverse direction, direction); the maxima follow at + 3
F = np.float32


def header(oct_, org=((-3.0, 1.0, -40.0), (5.0, 1.0, 2.5)), inv=((1.25, 1.5, 1.0), (4.0, 1.5, 900.0)), dirs=((0.25, -0.5, 0.0), (0.8, 0.75, 1.0)),
           state=None):
    """32 dwords: B under the pattern oct_ (inverse bounds given as magnitudes; the direction bounds need not match them: the test
    is per component)"""
    h = np.zeros(32, np.uint32)
    f = h.view(np.float32)
    f[0:3], f[3:6] = org
    for k in range(3):
        a, b = F(inv[0][k]), F(inv[1][k])
        f[6 + k], f[9 + k] = (-b, -a) if (oct_ >> k) & 1 else (a, b)
    f[13:16], f[16:19] = dirs
    h[19:] = 0xDEADBEEF
    h[STATE] = (oct_ | 0x100) if state is None else state
    return h


def inside_rays(h, rng, mode="interior"):
    """[9, 64]: rays inside the header's bounds: interior points, or points on its faces"""
    f = h.view(np.float32)
    out = np.zeros((9, 64), np.float32)
    for g in range(3):
        for k in range(3):
            lo, hi = f[LO[g] + k], f[LO[g] + 3 + k]
            t = rng.random(64).astype(np.float32)
            v = np.clip((lo + (hi - lo) * t).astype(np.float32), lo, hi)
            if mode == "faces":
                v = np.where(rng.random(64) < 0.5, lo, hi).astype(np.float32)
            out[g * 3 + k] = v
    return out


def ulp_out(x, up):
    return np.nextafter(F(x), F(np.inf) if up else F(-np.inf))


def wanted(h, rays, active):
    """the decision's plain definition"""
    if (int(h[STATE]) & ~7) != 0x100:
        return NO
    f = h.view(np.float32)
    for lane in range(64):
        if not (active >> lane) & 1:
            continue
        for g in range(3):
            for k in range(3):
                v = rays[g * 3 + k, lane]
                if not (f[LO[g] + k] <= v <= f[LO[g] + 3 + k]):  # (false for a NaN)
                    return NO
    return int(h[STATE]) & 7


def make_cases():
    """[(label, header, rays, active)]"""
    rng = np.random.default_rng(20)
    cases = []
    all_on = (1 << 64) - 1
    garbage = np.array([np.nan, np.inf, -np.inf, 3e38, -1e-30, 0.0], np.float32)
    for oct_ in range(8):
        h = header(oct_)
        f = h.view(np.float32)
        cases.append((f"inside/{oct_}", h, inside_rays(h, rng), all_on))
        cases.append((f"faces/{oct_}", h, inside_rays(h, rng, "faces"), all_on))
        r = inside_rays(h, rng)
        r[8, ::2] = F(-0.0)  # the z direction's lower bound is +0: -0 lies inside
        cases.append((f"minus-zero/{oct_}", h, r, all_on))
        for comp in range(9):
            g, k = divmod(comp, 3)
            for up in (False, True):
                r = inside_rays(h, rng)
                lane = int(rng.integers(64))
                r[comp, lane] = ulp_out(f[LO[g] + 3 + k] if up else f[LO[g] + k], up)
                cases.append((f"ulp/{oct_}/{comp}/{'hi' if up else 'lo'}", h, r, all_on))
                # ... the same ray in an inactive lane: masked
                cases.append((f"ulp-inactive/{oct_}/{comp}/{'hi' if up else 'lo'}", h, r, all_on & ~(1 << lane)))
            for bad in (np.nan, np.inf, -np.inf):
                r = inside_rays(h, rng)
                r[comp, int(rng.integers(64))] = bad
                cases.append((f"{bad}/{oct_}/{comp}", h, r, all_on))
        # an origin beyond 2^30 inside a B that reaches 2^31
        big = header(oct_, org=((-3.0, 1.0, -2.0 ** 31), (1.75 * 2.0 ** 30, 1.0, 2.5)))
        r = inside_rays(big, rng)
        r[0, 5] = F(1.5 * 2.0 ** 30)
        r[2, 9] = F(-1.5 * 2.0 ** 30)
        cases.append((f"origin-1.5x2^30/{oct_}", big, r, all_on))
        # a wrong-sign inverse direction, in each axis
        for k in range(3):
            r = inside_rays(h, rng)
            r[3 + k, int(rng.integers(64))] *= F(-1.0)
            cases.append((f"wrong-sign/{oct_}/{k}", h, r, all_on))
        # inactive lanes holding garbage; a single active lane; none
        act = int(rng.integers(1, 1 << 62)) | (1 << 63)
        r = inside_rays(h, rng)
        for lane in range(64):
            if not (act >> lane) & 1:
                r[:, lane] = rng.choice(garbage, 9)
        cases.append((f"garbage-inactive/{oct_}", h, r, act))
        one = 1 << int(rng.integers(64))
        r2 = np.tile(rng.choice(garbage, 9)[:, None], (1, 64)).astype(np.float32)
        lane = one.bit_length() - 1
        r2[:, lane] = inside_rays(h, rng)[:, lane]
        cases.append((f"one-active/{oct_}", h, r2, one))
        cases.append((f"none-active/{oct_}", h, r2, 0))
        # headers that are not valid, with every ray inside the bounds they hold
        for st in (0xFFFFFFFF, oct_, oct_ | 0x100 | 0x8, oct_ | 0x100 | 0x80000000, oct_ | 0x300, 0):
            hv = header(oct_, state=st)
            cases.append((f"state/{oct_}/{st:#x}", hv, inside_rays(hv, rng), all_on))
    return cases


def probe(cases):
    if not os.path.exists(SO):
        pytest.fail(f"{SO} missing: run build() first")
    import torch

    # (the renderer's HIP runtime is initialised before the probe's copy loads, the order the whole suite has)
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    torch.zeros(1, device="cuda")
    L = C.CDLL(SO)
    L.mp_mask_probe_entry.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    hdr = np.ascontiguousarray(np.stack([c[1] for c in cases]), np.uint32)
    rays = np.ascontiguousarray(np.stack([c[2] for c in cases]), np.float32)
    act = np.array([c[3] for c in cases], np.uint64)
    out = np.full(len(cases), 0xFFFFFFFF, np.uint32)
    none = C.c_uint32(0)
    rc = L.mp_mask_probe_entry(hdr.ctypes.data, rays.ctypes.data, act.ctypes.data, len(cases), out.ctypes.data, C.byref(none))
    assert rc == 0, f"HIP error {rc}"
    assert none.value == NO
    return out


def test_entry_decision_equals_its_definition():
    cases = make_cases()
    want = np.array([wanted(h, r, a) for _, h, r, a in cases], np.uint32)
    # the cases show what they are there for
    kind = lambda c: c[0].split("/")[0]
    enters = {"inside", "faces", "minus-zero", "ulp-inactive", "origin-1.5x2^30", "garbage-inactive", "one-active", "none-active"}
    for c, w in zip(cases, want):
        assert (w != NO) == (kind(c) in enters), (c[0], int(w))
        if w != NO:
            assert int(w) == int(c[0].split("/")[1]), c[0]
    assert len({kind(c) for c in cases}) == 14 and len(cases) == 8 * (3 + 9 * 7 + 1 + 3 + 3 + 6)
    got = probe(cases)
    bad = [(c[0], int(g), int(w)) for c, g, w in zip(cases, got, want) if g != w]
    print(f"{len(cases)} passes, {int(np.sum(want != NO))} enter the cached walk directly, {len(bad)} decided differently")
    assert not bad, bad[:10]


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
RES, TS, SPP, SEED = (96, 64), 32, 64, 57
PACKET = "render_tiles_packet_kernel<16, false, 8, false, true>"
VIEWS = ("teapot", "away", "wide")


@pytest.fixture(scope="module")
def world():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    ctx = mp.Context(0)
    return ctx, make_objects(ctx, VIEWS)


@pytest.mark.parametrize("name", VIEWS)
def test_frame_matches_the_oracle(oracle, world, name):
    ctx, objs = world
    of, ou8 = oracle_frame(oracle, name, RES, SPP, SEED, TS)
    alpha = of[..., 3]
    if name == "teapot":
        assert 0.0 < alpha.mean() < 1.0
    elif name == "away":
        assert not alpha.any(), "every ray misses"
    else:
        assert np.count_nonzero(alpha) > alpha.size // 2
    f, u8, names, _ = frame(ctx, objs[name], cameras()[name], mp.RenderSettings(TS, SPP, RES, seed=SEED))
    assert names == [PACKET], names
    print(f"{name}: {differing(f, of)} of {of.size} values differ from the oracle")
    assert_same_bits(f, of, name)
    assert np.array_equal(u8, ou8), name


def counted_frames():
    """{name: f32 frame, name + "_routes": (passes on the one bounds test, passes through the full guards)} in the library that is loaded"""
    prof = Counters(_lib.lib())
    ctx = mp.Context(0)
    cams, objs, out = cameras(), make_objects(ctx, VIEWS), {}
    for name in VIEWS:
        prof.reset()
        f, _, names, _ = frame(ctx, objs[name], cams[name], mp.RenderSettings(TS, SPP, RES, seed=SEED))
        assert names == [PACKET], names
        c = prof.read()
        out[name], out[name + "_routes"] = f, np.array([c["passes_bounds_entry"], c["passes_full_entry"]], np.uint64)
    return out


def test_both_entry_routes_occur(oracle, tmp_path):
    got = run_in_variant("noskip", "tests.test_pass_entry_gpu:counted_frames", tmp_path, timeout=600)
    passes = (RES[0] // 2) * (RES[1] // 2) * (SPP // 16)
    for name in VIEWS:
        assert_same_bits(got[name], oracle_frame(oracle, name, RES, SPP, SEED, TS)[0], name)
        short, full = (int(v) for v in got[name + "_routes"])
        print(f"{name}: {short} passes enter on the one bounds test, {full} through the full guards, of {passes}")
        assert short + full <= passes, name
    assert int(got["teapot_routes"][0]) > 0, "no pass of the teapot's frame took the short route"
    short, full = (int(v) for v in got["wide_routes"])
    assert short > 0 and full > 0, "both routes in the wide lens's frame"
    assert not got["away_routes"].any(), "a pass that the pre-test stops entered the walk"
