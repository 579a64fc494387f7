// The packet walk's per-work-unit mask cache (packet_walk.h, trace_packet_cached): the bounds B of a unit's rays, the predicates that
// prove a child box or a triangle missed by every ray inside B, and the pass-entry checks that keep B valid.  A header of its own so
// that a probe (mask_probe.hip, libmp_mask_probe.so) compiles the very functions the walk inlines and checks them against the
// per-ray arithmetic of the reference at the corners of B (tests/test_mask_cache_gpu.py).  Device code only; the includer may define
// MP_PROF_COUNT (profiling builds) and MP_MCACHE_PAD / MP_MCACHE_MARGIN / MP_NODE_ENTRIES / MP_LEAF_ENTRIES / MP_ARENA_ENTRIES / MP_NODE_SLOT_MASK / MP_NO_FAR_EXIT / MP_NO_MASK_FAR before including it.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "camera_rays.h"

#ifndef MP_PROF_COUNT
#define MP_PROF_COUNT(i) do { } while (0)
#endif

namespace mp {
namespace mc {
__device__ __forceinline__ float as_f(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ uint32_t as_u(float f) { return __float_as_uint(f); }

// LDS traffic between lanes of ONE wavefront: DS operations of a wave execute in issue order, so only the
// compiler has to be kept from reordering them.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct Ray {
    float ox, oy, oz, dx, dy, dz, ix, iy, iz;
};

// util/simba.rs:57-59
__device__ __forceinline__ float fma_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
}
// util/simba.rs:61-67 : mul_sub(a, b, c) = a*b - c, c rounded first
__device__ __forceinline__ float fms(float a, float b, float c) { return __builtin_fmaf(a, b, -c); }

// OCT >= 0: every ray of the wave has a finite inverse direction with the sign pattern OCT (bit 0: x < 0, bit 1: y < 0,
// bit 2: z < 0) and the box is ordered (min <= max, checked at upload).  IEEE subtraction and multiplication by a constant are
// monotone, so (bmin - o) * inv <= (bmax - o) * inv for inv > 0 and >= for inv < 0, and no 0 * inf can arise: the min / max of
// aabb.rs:269-271 select the near / far plane the sign names, and the six min/max drop out of the compiled code.
template <bool PATCH_NAN, int OCT>
__device__ __forceinline__ void slab(float bnx, float bny, float bnz, float bxx, float bxy, float bxz, const Ray& r,
                                     float limit, float& t1, float& t2) {
    // aabb.rs:254-284
    float ax = (bnx - r.ox) * r.ix, ay = (bny - r.oy) * r.iy, az = (bnz - r.oz) * r.iz;
    float cx = (bxx - r.ox) * r.ix, cy = (bxy - r.oy) * r.iy, cz = (bxz - r.oz) * r.iz;
    if (PATCH_NAN) {  // only rays with an infinite inverse direction component can produce 0*inf; maxNum/minNum drop a NaN operand
        ax = fmaxf(ax, -INFINITY); ay = fmaxf(ay, -INFINITY); az = fmaxf(az, -INFINITY);
        cx = fminf(cx, INFINITY); cy = fminf(cy, INFINITY); cz = fminf(cz, INFINITY);
    }
    float lox, loy, loz, hix, hiy, hiz;
    if (OCT >= 0) {
        lox = (OCT & 1) ? cx : ax; hix = (OCT & 1) ? ax : cx;
        loy = (OCT & 2) ? cy : ay; hiy = (OCT & 2) ? ay : cy;
        loz = (OCT & 4) ? cz : az; hiz = (OCT & 4) ? az : cz;
    } else {
        lox = fminf(ax, cx); loy = fminf(ay, cy); loz = fminf(az, cz);
        hix = fmaxf(ax, cx); hiy = fmaxf(ay, cy); hiz = fmaxf(az, cz);
    }
    t1 = fmaxf(fmaxf(lox, 0.0f), fmaxf(loy, loz));
    t2 = fminf(fminf(hix, limit), fminf(hiy, hiz));
}

// ---- packet-level child rejection with a per-unit mask cache (round 3) ----------------------------------------------------------
// Counted on the metric's frame (tools/sim_collapse.py --packet-studies; profiles/r03_notes.md): a 64-ray camera packet tests 110
// child boxes per pass and pushes 19; for 90 of the 91 others NO ray of the packet can pass, and a conservative test on bounds of
// the packet -- componentwise min / max of the origins and inverse directions -- proves it.  Evaluating that test per node visit
// (lane j = child j, the records through a vector load) was built first and ran slower than it saved (profiles/r03_notes.md).
// What pays is doing it ONCE PER WORK UNIT: a unit shoots 8-16 passes through the same 2-4 pixels, and one set of bounds B that
// contains every pass's rays gives one "children that may be hit" mask per node, from which the unit's child lists are built once and
// cached in LDS (unit_list_build below; the packet kernel uses no other LDS).  Every pass checks, lane by lane, that its ray lies inside B (no reduction), and while that holds and the sign
// pattern is the same, opening a node costs one LDS lookup and the exact per-ray slab tests of the surviving children only.  B starts
// as the bounds of the unit's corner rays, computed from the camera (mask_cache_begin_unit), or, where that declines, as the bounds
// of the first pass (wave reductions) widened by MP_MCACHE_PAD of their extent; a pass that does not fit widens B and clears the
// cache.
// Why skipping a child whose bit is clear is exact.  Only in the sign-specialised walks (OCT >= 0: every active ray has finite
// inverse directions of one sign pattern) and only if every active origin and inverse component is finite.  Axis with inv > 0
// (aabb.rs:257-271 gives lo = fl(fl(bmin - o) * inv), hi = fl(fl(bmax - o) * inv)): with omax >= o for every ray,
// y = fl(bmin - omax) <= fl(bmin - o) (IEEE subtraction is monotone), so lo >= fl(y * inv) (multiplication by a positive number is
// monotone) >= min(fl(y * imin), fl(y * imax)) =: L (x -> fl(y * x) is monotone on [imin, imax]: its minimum sits at an end);
// likewise hi <= max(fl(z * imin), fl(z * imax)) =: U with z = fl(bmax - omin).  Axis with inv < 0: lo comes from bmax and products
// decrease with the first factor: L from z, U from y.  Every ray's t1 = max(lo.x, 0, lo.y, lo.z) >= T1 = max(L.x, L.y, L.z, 0) and
// its t2 = min(hi.x, limit, hi.y, hi.z) <= T2 = min(U.x, U.y, U.z); T1 > T2 therefore means t1 > t2 for every ray whose origin and
// inverse direction lie in B: the reference pushes the child for none of them (ray_bvh_intersection.rs:158).  No NaN can arise: all
// inputs are finite, inv is never 0, and B's inverse bounds keep the sign of the pattern.
#ifndef MP_MCACHE_PAD
#define MP_MCACHE_PAD 0.25f  // widening of the unit's bounds on either side, in extents of the pass that sets them (A/B: 0.0625 .. 1, profiles/r03_notes.md)
#endif
// Table sizes.  The node table (per-unit child LISTS: see unit_list_build below) is a direct-mapped table of MP_NODE_ENTRIES tags
// (node index; slot = node_slot(node)) with one value dword each (list offset << 16 | entries) and an arena of MP_ARENA_ROOM list
// entries; together they take the 512 dwords the node masks had, so that the wave's LDS stays at 928 dwords (launch_plan.h).
// How the split follows from the counts (tools/unit_list_count.py, tests/test_unit_lists_cpu.py): a unit of the metric's frame builds
// 1.20 lists (1.55 on the wide tree), the longest 29 entries; units of the small eviction frame, whose pixels cover more of the
// scene, 1.4 lists, the longest 129 entries, and 34 evictions in 512 units at 64 slots on the wide tree.  So the table is small --
// 64 slots are forty times the lists of a unit, and fewer would only add evictions -- and everything else goes to the arena: 384
// entries are three times the longest list counted, so that a unit's lists fit without a reset.  The leaf table is as before
// (tools/cache_miss_count.py: 5.8 leaf-mask slow paths per unit at 128 entries).
#ifndef MP_NODE_ENTRIES
#define MP_NODE_ENTRIES 64
#endif
#ifndef MP_LEAF_ENTRIES
#define MP_LEAF_ENTRIES 128
#endif
#ifndef MP_ARENA_ENTRIES
#define MP_ARENA_ENTRIES 384  // list entries a unit may hold (test builds: fewer, the LDS layout stays)
#endif
#ifndef MP_ARENA_ROOM
#define MP_ARENA_ROOM 384  // dwords of the arena in the layout
#endif
#ifndef MP_NODE_SLOT_MASK
#define MP_NODE_SLOT_MASK 0xFFFFFFFFu  // test builds: 3 makes a table of four slots (all-ones: the AND folds away)
#endif
constexpr int kMaskCacheEntries = MP_NODE_ENTRIES;                      // node tags: slot node_slot(node) holds the node's index; the LAST tag dword holds ~(arena entries in use)
constexpr int kMaskCacheHeader = 32;                        // B: [0..11] origin / inverse-direction bounds, [12] = sign pattern | 0x100 when valid (0xFFFFFFFF: none), [13..18] direction bounds
constexpr int kLeafCacheEntries = MP_LEAF_ENTRIES;                      // direct-mapped: first packet of the leaf & 127 ; tag = first packet, mask = 64 bits (triangle i of the leaf)
constexpr int kLeafTagBase = kMaskCacheHeader + kMaskCacheEntries;
constexpr int kLeafMaskBase = kLeafTagBase + kLeafCacheEntries;   // uint2 per entry (8-byte aligned)
// [kMaskCacheHeader, kLeafMaskBase) is what the clears of mask_cache_begin_pass / mask_cache_begin_unit set to all-ones: no node and
// no leaf has that tag, and the arena is empty (~0xFFFFFFFF = 0 entries in use).  Behind the leaf masks, untouched by the clears:
constexpr int kNodeListBase = kLeafMaskBase + 2 * kLeafCacheEntries;  // value of node slot i: (first entry's dword index in the wave's cache) << 16 | entries ; the LAST value dword holds the root's record index (the walk's first frame)
constexpr int kArenaBase = kNodeListBase + kMaskCacheEntries;         // list entries: record indices node * slots + slot into the walked tree
constexpr int kArenaRoom = MP_ARENA_ROOM;
constexpr int kArenaEntries = MP_ARENA_ENTRIES;
constexpr int kMaskCacheDwords = kArenaBase + kArenaRoom;
constexpr int kArenaTopSlot = kMaskCacheHeader + kMaskCacheEntries - 1;
constexpr int kRootListSlot = kNodeListBase + kMaskCacheEntries - 1;
static_assert((kMaskCacheEntries & (kMaskCacheEntries - 1)) == 0 && kMaskCacheEntries >= 4, "the node table's slot mask");
static_assert(kArenaEntries >= 16 && kArenaEntries <= kArenaRoom, "an unexpanded list (at most 16 entries) fits the empty arena");
static_assert((kLeafMaskBase % 2) == 0 && (kMaskCacheDwords % 4) == 0, "LDS alignment of the leaf masks / of the next wave's header");
constexpr float kCoordCap = 1073741824.0f;                  // 2^30: magnitude bound of ray origins and triangle vertices for the triangle masks (see tri_may_hit)
struct MaskCache {
    uint32_t* lds;  // this wave's header + entries, or nullptr: no packet-level rejection
};
// Wave-wide minima of N values and maxima of N values at once (every lane takes part; inactive rays hold the neutral element):
// four DPP steps inside each row of 16, row_bcast15 / row_bcast31 across the rows, the totals end in LANE 63's registers (the
// caller goes on in the vector domain and takes lane 63's verdict: the scalar registers would not fit beside the walk's).  The
// independent chains are interleaved step by step, so no instruction reads a register the previous two instructions wrote (the
// DPP read-after-VALU-write hazard needs two wait states) and no s_nop is spent.
#define MP_DPP_STEP6(CTRL)                                                                                              \
    "v_min_f32_dpp %0, %0, %0 " CTRL "\n\tv_min_f32_dpp %1, %1, %1 " CTRL "\n\tv_min_f32_dpp %2, %2, %2 " CTRL "\n\t"         \
    "v_max_f32_dpp %3, %3, %3 " CTRL "\n\tv_max_f32_dpp %4, %4, %4 " CTRL "\n\tv_max_f32_dpp %5, %5, %5 " CTRL "\n\t"
__device__ __forceinline__ void wave_min3_max3(float (&mn)[3], float (&mx)[3]) {
    asm volatile("s_nop 1\n\t"  // the operands may come straight out of VALU instructions
                 MP_DPP_STEP6("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf")
                 MP_DPP_STEP6("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")
                 MP_DPP_STEP6("row_half_mirror row_mask:0xf bank_mask:0xf")
                 MP_DPP_STEP6("row_mirror row_mask:0xf bank_mask:0xf")
                 MP_DPP_STEP6("row_bcast:15 row_mask:0xa bank_mask:0xf")
                 MP_DPP_STEP6("row_bcast:31 row_mask:0xc bank_mask:0xf")
                 : "+v"(mn[0]), "+v"(mn[1]), "+v"(mn[2]), "+v"(mx[0]), "+v"(mx[1]), "+v"(mx[2]));
}
// Whether a ray may use the cached walk: every origin component within 2^30, every inverse-direction component finite and every
// direction component within 2 in magnitude (tri_may_hit's no-overflow argument).  In the vector domain, branch-free: for any f32 x
// (NaN included: its magnitude bits lie above +inf's) and any c >= 0, |x| <= c  <=>  (bits(x) & 0x7FFFFFFF) <= bits(c), and for
// m, C in [0, 2^31 - 1), m <= C  <=>  m - (C + 1) is negative as a 32-bit integer: the three tests are the sign of one AND.
__device__ __forceinline__ bool mask_cache_ray_ok(const Ray& r) {
    constexpr uint32_t kMag = 0x7FFFFFFFu;
    const uint32_t mo = max(max(as_u(r.ox) & kMag, as_u(r.oy) & kMag), as_u(r.oz) & kMag);
    const uint32_t mi = max(max(as_u(r.ix) & kMag, as_u(r.iy) & kMag), as_u(r.iz) & kMag);
    const uint32_t md = max(max(as_u(r.dx) & kMag, as_u(r.dy) & kMag), as_u(r.dz) & kMag);
    constexpr uint32_t kCapO = 0x4E800000u /* 2^30 */, kCapI = 0x7F7FFFFFu /* FLT_MAX */, kCapD = 0x40000000u /* 2.0 */;
    static_assert(kCoordCap == 1073741824.0f, "kCapO is kCoordCap's bit pattern");
    return static_cast<int32_t>((mo - (kCapO + 1u)) & (mi - (kCapI + 1u)) & (md - (kCapD + 1u))) < 0;
}
// Called once per pass, before a sign-specialised walk with pattern `oct`, for a pass whose every active ray passed
// mask_cache_ray_ok: makes the cache's bounds B contain this pass's rays (widening B and clearing the masks if they do not).
// B = origin, inverse-direction and direction bounds; three groups of (3 minima, 3 maxima) in header slots hdr_lo(g) .. + 5.
// The header (slots 0..19) is read with five 16-byte LDS loads (the wave's base is 16-byte aligned: kMaskCacheDwords % 4 == 0, the
// per-wave LDS sizes of both cached kernels are multiples of 16 bytes, and smem is __align__(16)).
constexpr int kHdrState = 12;                     // sign pattern | 0x100 while B is valid (0xFFFFFFFF: none)
constexpr int hdr_lo(int g) { return g == 2 ? kHdrState + 1 : g * 6; }  // group g's minima; its maxima follow at + 3
// P inside B ?  Every active lane compares its own ray with the header: no reduction in the common case.  For finite v and finite
// lo <= hi, med3(v, lo, hi) is v itself when lo <= v <= hi (up to the sign of a zero) and lo or hi otherwise, and the difference of
// two finite numbers is +-0 exactly when they are equal (denormals are kept): v < lo || v > hi  <=>  bounds_deviation(v, lo, hi) != 0.
// mask_cache_begin_pass folds the nine deviations with maxNum (never NaN: all operands finite).  (The fold stays in the caller: as a
// function of the nine values it schedules the flagship kernel's pass entry differently.)
__device__ __forceinline__ float bounds_deviation(float v, float lo, float hi) {
    return fabsf(v - __builtin_amdgcn_fmed3f(v, lo, hi));
}
__device__ __forceinline__ void mask_cache_begin_pass(const MaskCache& mc, const Ray& r, bool active, uint32_t oct) {
    const int lane = static_cast<int>(threadIdx.x) & 63;
    float* hdr = reinterpret_cast<float*>(mc.lds);
    float h[20];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const float4 q = reinterpret_cast<const float4*>(mc.lds)[i];
        h[4 * i] = q.x; h[4 * i + 1] = q.y; h[4 * i + 2] = q.z; h[4 * i + 3] = q.w;
    }
    const uint32_t state = __builtin_amdgcn_readfirstlane(as_u(h[kHdrState]));
    const bool same = state == (oct | 0x100u);
    const float val[3][3] = {{r.ox, r.oy, r.oz}, {r.ix, r.iy, r.iz}, {r.dx, r.dy, r.dz}};
    float dev = 0.0f;
#pragma unroll
    for (int g = 0; g < 3; g++) {
#pragma unroll
        for (int k = 0; k < 3; k++) dev = fmaxf(dev, bounds_deviation(val[g][k], h[hdr_lo(g) + k], h[hdr_lo(g) + 3 + k]));
    }
    if (__ballot(active && (!same || dev != 0.0f)) != 0) {
        float pmin[3][3], pmax[3][3];  // after the reductions: lane 63 holds the wave's bounds
#pragma unroll
        for (int g = 0; g < 3; g++) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                pmin[g][k] = active ? val[g][k] : INFINITY;
                pmax[g][k] = active ? val[g][k] : -INFINITY;
            }
            wave_min3_max3(pmin[g], pmax[g]);
        }
        // new bounds: this pass's, united with the old ones when they belong to the same sign pattern, widened by MP_MCACHE_PAD of the extent
        // (an inverse-direction bound never crosses zero: the sign pattern is part of the node masks' meaning; origin bounds stay
        // within 2^31 and direction bounds within 2: every pass that gets here lies well inside)
#pragma unroll
        for (int g = 0; g < 3; g++) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                float lo = pmin[g][k], hi = pmax[g][k];
                if (same) { lo = fminf(lo, h[hdr_lo(g) + k]); hi = fmaxf(hi, h[hdr_lo(g) + 3 + k]); }
                const float pad = (hi - lo) * MP_MCACHE_PAD;
                float wlo = lo - pad, whi = hi + pad;
                if (g == 1) {  // same sign as the pass's inverse directions (all of one sign, finite, non-zero)
                    if ((wlo < 0.0f) != (lo < 0.0f) || wlo == 0.0f) wlo = lo;
                    if ((whi < 0.0f) != (hi < 0.0f) || whi == 0.0f) whi = hi;
                    if (!(fabsf(wlo) < INFINITY)) wlo = lo;
                    if (!(fabsf(whi) < INFINITY)) whi = hi;
                } else {
                    const float cap = g == 0 ? 2.0f * kCoordCap : 2.0f;
                    wlo = fmaxf(wlo, -cap); whi = fminf(whi, cap);
                }
                pmin[g][k] = wlo; pmax[g][k] = whi;
            }
        }
        MP_PROF_COUNT(3);
        wave_lds_sync();  // the reads above before the header is rewritten
        if (lane == 63) {
#pragma unroll
            for (int g = 0; g < 3; g++) {
#pragma unroll
                for (int k = 0; k < 3; k++) { hdr[hdr_lo(g) + k] = pmin[g][k]; hdr[hdr_lo(g) + 3 + k] = pmax[g][k]; }
            }
            mc.lds[kHdrState] = oct | 0x100u;
        }
        int l_ = lane;  // (re-derived here: the clear runs once per unit, its address is not worth a register across the walk)
        asm volatile("" : "+v"(l_));
#pragma unroll
        for (int i = 0; i < (kMaskCacheEntries + kLeafCacheEntries) / 64; i++) mc.lds[kMaskCacheHeader + i * 64 + l_] = 0xFFFFFFFFu;  // no node / leaf has this tag
        wave_lds_sync();
    }
}
// ---- pass entry in one test: is the whole pass inside a valid B? ------------------------------------------------------------------
// Called by every lane before anything else of a pass (packet_walk.h, trace_packet).  Returns B's sign pattern (0..7) when the
// header holds a valid B (state = pattern | 0x100; no other bit, so not 0xFFFFFFFF) and no active lane's ray deviates from B in any of
// its nine components; kNoPattern otherwise, and the pass takes the full route: mask_cache_ray_ok, the sign ballots,
// mask_cache_begin_pass.  With a pattern the caller enters the cached walk of that pattern directly.  What the skipped guards would
// have established follows from "inside a valid B":
//   * Sign and finiteness.  A valid B was written by mask_cache_begin_unit or mask_cache_begin_pass from rays that had passed
//     mask_cache_ray_ok and shared one sign pattern, and the widening of both keeps each inverse-direction bound finite, non-zero
//     and of that sign (a widened bound that crosses or reaches zero, or overflows, is replaced by the unwidened one).  A component
//     with lo <= v <= hi between two finite non-zero numbers of one sign is finite, non-zero and of that sign: no infinite inverse
//     (the literal walk is not needed), every sign ballot uniform and equal to the header's pattern.
//   * tri_may_hit's and bounds_may_hit's no-overflow bounds are bounds on B, not on the rays: B's direction bounds stay within 2 and
//     its origin bounds within 2^31 (the caps of the same two widenings), whichever route the pass took.
//   * A ray with an origin component between 2^30 and 2^31 in magnitude that lies inside B fails mask_cache_ray_ok and took a
//     generic walk; here it takes the cached one.  The hits are the same: every walk computes the reference's, and the cached walk's
//     exactness argument asks for rays inside B, nothing about 2^30.
//   * NaN and infinity.  A deviation |v - med3(v, lo, hi)| is NaN for a NaN v and +inf for an infinite v (lo and hi are finite).  The
//     nine are folded by ADDITION, not by maxNum as in mask_cache_begin_pass: maxNum drops a NaN operand, a sum keeps it, and a sum of
//     non-negative terms is zero only if every term is (an overflow gives +inf).  The test is !(sum == 0), true for NaN: such a ray
//     never enters here.  No separate NaN guard.
// Inactive lanes may hold anything; their verdict is masked.  The decision steers work only.
constexpr uint32_t kNoPattern = 8u;
__device__ __forceinline__ uint32_t mask_cache_pass_inside(const MaskCache& mc, const Ray& r, bool active) {
    float h[20];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const float4 q = reinterpret_cast<const float4*>(mc.lds)[i];
        h[4 * i] = q.x; h[4 * i + 1] = q.y; h[4 * i + 2] = q.z; h[4 * i + 3] = q.w;
    }
    const uint32_t state = __builtin_amdgcn_readfirstlane(as_u(h[kHdrState]));
    const float val[3][3] = {{r.ox, r.oy, r.oz}, {r.ix, r.iy, r.iz}, {r.dx, r.dy, r.dz}};
    float dev = 0.0f;
#pragma unroll
    for (int g = 0; g < 3; g++) {
#pragma unroll
        for (int k = 0; k < 3; k++) dev += bounds_deviation(val[g][k], h[hdr_lo(g) + k], h[hdr_lo(g) + 3 + k]);
    }
    const bool inside = __ballot(active && !(dev == 0.0f)) == 0;
    return ((state & ~7u) == 0x100u && inside) ? (state & 7u) : kNoPattern;
}
// ---- B from the camera: the unit's bounds before its first pass ------------------------------------------------------------------
// A unit's rays are a closed-form function of the camera (camera_rays.h): film points inside its pixel block (widened by the jitter) and lens points
// inside the lens disc.  Origins and unnormalised directions are linear in (film_u, film_v, lens a, lens b), so over the box
// [u0, u1] x [v0, v1] x [-lens_radius, lens_radius]^2 their extremes sit at its 16 corners; a normalised direction component is not
// monotone in the other two, so its extreme can lie off a corner by a term of second order in the footprint's angle, which
// MP_MCACHE_MARGIN covers (counted: profiles/analytic_bounds_notes.md).  B is a guess that every pass verifies
// (mask_cache_begin_pass): a ray outside it costs a widen-and-clear, never a result.
#ifndef MP_MCACHE_MARGIN
#define MP_MCACHE_MARGIN 0.015625f  // widening of the corner rays' bounds on either side, in their own extents (A/B: 1/64 .. 1/8, profiles/analytic_bounds_notes.md)
#endif
// Called once per work unit, by every lane of the wave, before the unit's first pass.  The unit's pixels are [x0, x1] x [y0, y1]
// (inclusive) and a sample's film point is pixel + (u * jitter_scale - 0.5) with u in [0, 1).  Lane l builds corner l & 15 (bit 0:
// film_u high, bit 1: film_v high, bit 2 / 3: lens a / b high; the four copies of a corner reduce like one).  If every corner may
// use the cached walk and their inverse directions share one sign pattern, B = the corners' bounds widened by MP_MCACHE_MARGIN of
// their extent under the guards of mask_cache_begin_pass, and the node and leaf tags are cleared (the clear the first pass's set
// would do).  Otherwise no B: the first pass sets it by reduction, as it does for a pass of another sign pattern.
__device__ __forceinline__ void mask_cache_begin_unit(const MaskCache& mc, const mp_camera_sampler& s, float jitter_scale, uint32_t x0,
                                                      uint32_t x1, uint32_t y0, uint32_t y1) {
    const int lane = static_cast<int>(threadIdx.x) & 63;
    Ray r;
    float f[3];
    camera_film(s, (lane & 1) ? static_cast<float>(x1) + (jitter_scale + (-0.5f)) : static_cast<float>(x0) + (-0.5f),
                (lane & 2) ? static_cast<float>(y1) + (jitter_scale + (-0.5f)) : static_cast<float>(y0) + (-0.5f), f);
    camera_lens_ray(s, f, (lane & 4) ? 1.0f : -1.0f, (lane & 8) ? 1.0f : -1.0f, r);
    const uint64_t nx = __ballot(r.ix < 0.0f), ny = __ballot(r.iy < 0.0f), nz = __ballot(r.iz < 0.0f);
    const bool adopt = __ballot(!mask_cache_ray_ok(r)) == 0 && (nx == 0 || ~nx == 0) && (ny == 0 || ~ny == 0) && (nz == 0 || ~nz == 0);
    if (!adopt) {
        if (lane == 0) mc.lds[kHdrState] = 0xFFFFFFFFu;
        wave_lds_sync();
        return;
    }
    const uint32_t oct = (nx ? 1u : 0u) | (ny ? 2u : 0u) | (nz ? 4u : 0u);
    float pmin[3][3] = {{r.ox, r.oy, r.oz}, {r.ix, r.iy, r.iz}, {r.dx, r.dy, r.dz}}, pmax[3][3];  // after the reductions: lane 63 holds the bounds
#pragma unroll
    for (int g = 0; g < 3; g++) {
#pragma unroll
        for (int k = 0; k < 3; k++) pmax[g][k] = pmin[g][k];
        wave_min3_max3(pmin[g], pmax[g]);
    }
    float* hdr = reinterpret_cast<float*>(mc.lds);
    if (lane == 63) {
#pragma unroll
        for (int g = 0; g < 3; g++) {
#pragma unroll
            for (int k = 0; k < 3; k++) {  // mask_cache_begin_pass's widening, with the margin for the pad
                const float lo = pmin[g][k], hi = pmax[g][k];
                const float pad = (hi - lo) * MP_MCACHE_MARGIN;
                float wlo = lo - pad, whi = hi + pad;
                if (g == 1) {
                    if ((wlo < 0.0f) != (lo < 0.0f) || wlo == 0.0f) wlo = lo;
                    if ((whi < 0.0f) != (hi < 0.0f) || whi == 0.0f) whi = hi;
                    if (!(fabsf(wlo) < INFINITY)) wlo = lo;
                    if (!(fabsf(whi) < INFINITY)) whi = hi;
                } else {
                    const float cap = g == 0 ? 2.0f * kCoordCap : 2.0f;
                    wlo = fmaxf(wlo, -cap); whi = fminf(whi, cap);
                }
                hdr[hdr_lo(g) + k] = wlo; hdr[hdr_lo(g) + 3 + k] = whi;
            }
        }
        mc.lds[kHdrState] = oct | 0x100u;
    }
    MP_PROF_COUNT(3);
#pragma unroll
    for (int i = 0; i < (kMaskCacheEntries + kLeafCacheEntries) / 64; i++) mc.lds[kMaskCacheHeader + i * 64 + lane] = 0xFFFFFFFFu;  // no node / leaf has this tag
    wave_lds_sync();
}
// lane j (0..7): can any ray with origin / inverse direction inside the bounds `b` (omin[3], omax[3], imin[3], imax[3]) pass child
// j's box {bmn, bmx}?  (see above)
template <int OCT>
__device__ __forceinline__ bool bounds_may_hit(const float* b, const float bmn[3], const float bmx[3]) {
    float L[3], U[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float y = bmn[k] - b[3 + k], z = bmx[k] - b[k];
        const float lo_src = ((OCT >> k) & 1) ? z : y, hi_src = ((OCT >> k) & 1) ? y : z;
        L[k] = fminf(lo_src * b[6 + k], lo_src * b[9 + k]);
        U[k] = fmaxf(hi_src * b[6 + k], hi_src * b[9 + k]);
    }
    const float t1 = fmaxf(fmaxf(L[0], 0.0f), fmaxf(L[1], L[2])), t2 = fminf(U[0], fminf(U[1], U[2]));
    return !(t1 > t2);
}
// ---- the scene pre-test, decided once per unit ----------------------------------------------------------------------------------
// may_hit_scene (group_walk.h) tests every ray of every pass against the union box of the root's children.  Called by every lane
// after mask_cache_begin_unit: if the unit adopted bounds B from its corner rays, the box {pre_min, pre_max} is put to
// bounds_may_hit's corner evaluation under B's sign pattern (read from the header: a run-time OCT, otherwise the same arithmetic;
// no upper limit on t2, which only errs towards "may").  True: some ray inside B may reach the box -- in an interior frame every
// ray does -- and the unit's passes enter the walk without the per-ray test.  False (no B, or B cannot reach the box): the caller
// keeps the per-ray test, which for rays inside such a B fails for every ray and skips the walk.
//   The answer steers work only, never a result, whatever B later becomes (a pass that widens B keeps "may" true, the union
// containing the old B; a pass of another sign pattern replaces B, and the unit goes on without the per-ray test).  Skipping the
// pre-test is exact by the argument above may_hit_scene: a ray whose interval against the union box U is empty passes the slab
// test of no child box of the root, each being inside U with its interval inside U's in floating point too.  The cached walk
// starts from the root's unit list, whose every entry is such a child or a descendant nested in one (absorbed under
// unit_list_build's rule, or collapsed into the record by device_tree.cpp's, both of which require the nesting on the floats the
// walk loads), so its interval is inside U's as well: the ray is live in no frame, tests no triangle and leaves the walk as a
// miss, as the skipped walk would have left it.  The uncached walks a pass may fall back to open the root's children with the
// same slab test.  (Scenes without a pre-test box, has_pre == 0, run every ray through the walks in just this way.)
__device__ __forceinline__ bool mask_cache_unit_reaches(const MaskCache& mc, const float pre_min[3], const float pre_max[3]) {
    const uint32_t state = __builtin_amdgcn_readfirstlane(mc.lds[kHdrState]);
    if (state == 0xFFFFFFFFu) return false;
    const float* b = reinterpret_cast<const float*>(mc.lds);
    float L[3], U[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float y = pre_min[k] - b[3 + k], z = pre_max[k] - b[k];
        const bool neg = ((state >> k) & 1u) != 0u;
        const float lo_src = neg ? z : y, hi_src = neg ? y : z;
        L[k] = fminf(lo_src * b[6 + k], lo_src * b[9 + k]);
        U[k] = fmaxf(hi_src * b[6 + k], hi_src * b[9 + k]);
    }
    const float t1 = fmaxf(fmaxf(L[0], 0.0f), fmaxf(L[1], L[2])), t2 = fminf(U[0], fminf(U[1], U[2]));
    return __ballot(!(t1 > t2)) != 0;  // (the same value in every lane: a scalar for the caller)
}

// ---- per-unit child LISTS: the kept children of a node, with kept descendants in place of the children that need no test --------
// Counted (tools/unit_list_count.py, profiles/unit_lists_notes.md): under a unit's masks a node keeps 1.43 children, so the walk
// mostly steps down chains of inner nodes, each step a pop, a record load, a slab test and a table lookup.  device_tree.cpp proves
// when such a step is redundant and applies it to all of a node's children up to 16 slots; per unit only the KEPT children matter.
// The list of node N under the bounds B is built depth-first over kept children in ascending slot order:
//   * a kept leaf child is an entry (its record index, node * slots + slot: what the walk loads when it pops the entry);
//   * a kept inner child M none of whose children is kept is dropped: the walk would test M's box and then open nothing;
//   * a kept inner child M is ABSORBED -- its kept children take its place, recursively -- when every kept child g of M is
//     FP-nested in M's box as N's record states it (M.min <= g.min and g.max <= M.max per axis, on the floats the walk loads);
//   * any other kept inner child is an entry; it gets a list of its own when a pass opens it.
// Why absorbing is exact (device_tree.cpp's argument with "children" read as "children the unit keeps"; rays are inside B, so
// neither walk visits a child that is not kept).  Let ray r be live in N's frame.  The mask walk tests g for r iff r passes M's
// slab test when M is popped (t1(M) <= min(hi(M), best.t then)), and then tests g against best.t at g's pop.  IEEE subtraction and
// multiplication by the ray's inverse direction are monotone, so g nested in M gives lo(M) <= lo(g) and hi(g) <= hi(M) per axis,
// hence t1(M) <= t1(g) and hi(g) <= hi(M); best.t never grows, so best.t at g's pop <= best.t at M's pop.  A ray that passes g's
// test, t1(g) <= min(hi(g), best.t at g's pop), therefore passes M's: testing g directly, for the rays live in N's frame, accepts
// exactly the rays the two-step walk accepts, with the same limit.  Between M's pop and its children's pops the mask walk does
// nothing else (M's frame goes on top), and the children of M stand where M stood, ascending, so a list walked last-to-first
// visits the leaves in the mask walk's order: the same triangle tests in the same order, the same best.t throughout.
// The arena: lists are appended and never freed; a list that does not fit resets the node table and the arena (the caller then
// either builds it again or, if frames of the running walk still point into the arena, leaves that pass to a walk without a
// cache).  Absorbing stops where the space left could not hold the entries still pending, each taken as one unexpanded entry.
constexpr uint32_t kNullLink = 0xFFFFFFF8u;      // MP_LINK_NULL
constexpr uint32_t kListOverflow = 0xFFFFFFFFu;  // unit_list_build: the list did not fit, table and arena were reset
constexpr uint32_t kEmptyLeafBit = 0x80000000u;  // set by the WALK in an arena entry (never by the builder): a leaf whose unit triangle mask is empty
constexpr int kListDepth = 64;                  // continuation stack of the depth-first pass (lane registers)
__device__ __forceinline__ uint32_t node_slot(uint32_t node) {
    return min(node & static_cast<uint32_t>(kMaskCacheEntries - 1) & MP_NODE_SLOT_MASK, static_cast<uint32_t>(kMaskCacheEntries - 2));
}
// Every lane of the wave calls it.  recs: the walked tree, `slots` (8 or 16) records of 32 bytes per node; kept(b, bmn, bmx): the
// unit's rejection test under the pattern of B (bounds_may_hit<OCT>).  Returns the table value of the list (first entry's dword
// index << 16 | entries; no entries: nothing to open) after storing it under the node's tag, or kListOverflow.
template <class Kept>
__device__ __forceinline__ uint32_t unit_list_build(const float4* __restrict__ recs, uint32_t* mcache, uint32_t node, uint32_t slots, Kept kept) {
    const uint32_t lane = threadIdx.x & 63u;
    const float* b = reinterpret_cast<const float*>(mcache);
    node = __builtin_amdgcn_readfirstlane(node);  // (wave-uniform, which the arguments of a real call are not known to be)
    slots = __builtin_amdgcn_readfirstlane(slots);
    // lane j = child j of node n: its record and whether the unit keeps it
    auto kept_of = [&](uint32_t n, float4& c0, float4& c1) -> uint32_t {
        bool keep = false;
        c0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f); c1 = c0;
        if (lane < slots) {
            const float4* r = recs + (static_cast<size_t>(n) * slots + lane) * 2;
            c0 = r[0]; c1 = r[1];  // {min.xyz, max.x} {max.yz, link, n}
            const float bmn[3] = {c0.x, c0.y, c0.z}, bmx[3] = {c0.w, c1.x, c1.y};
            keep = as_u(c1.z) != kNullLink && kept(b, bmn, bmx);
        }
        return __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(__ballot(keep)));
    };
    float4 c0, c1;  // the records of `cur`, lane j = child j: a child's box and link are read from its lane, not loaded again
    uint32_t mask = kept_of(node, c0, c1);
    const uint32_t top = ~__builtin_amdgcn_readfirstlane(mcache[kArenaTopSlot]);
    if (top > static_cast<uint32_t>(kArenaEntries) || top + static_cast<uint32_t>(__popc(mask)) > static_cast<uint32_t>(kArenaEntries)) {
        MP_PROF_COUNT(5);
        wave_lds_sync();
#pragma unroll
        for (int i = 0; i < (kMaskCacheEntries + 63) / 64; i++)
            if (i * 64 + static_cast<int>(lane) < kMaskCacheEntries) mcache[kMaskCacheHeader + i * 64 + static_cast<int>(lane)] = 0xFFFFFFFFu;
        wave_lds_sync();
        return kListOverflow;
    }
    const uint32_t room = static_cast<uint32_t>(kArenaEntries) - top;
    uint32_t used = 0u, pend = static_cast<uint32_t>(__popc(mask)), cur = node;  // invariant: used + pend <= room
    int st_node = 0, st_mask = 0, depth = 0;  // (node, kept children still to take) of the nodes above `cur`: entry i in lane i
    for (;;) {
        if (mask == 0u) {
            while (mask == 0u && depth > 0) {
                depth--;
                cur = static_cast<uint32_t>(__builtin_amdgcn_readlane(st_node, depth));
                mask = static_cast<uint32_t>(__builtin_amdgcn_readlane(st_mask, depth));
            }
            if (mask == 0u) break;
            if (lane < slots) {  // back at a node above: its records again
                const float4* r = recs + (static_cast<size_t>(cur) * slots + lane) * 2;
                c0 = r[0]; c1 = r[1];
            }
        }
        const uint32_t j = static_cast<uint32_t>(__builtin_ctz(mask));
        mask &= mask - 1u;
        pend--;
        const uint32_t rec = cur * slots + j;
        auto from_lane = [&](float v) { return as_f(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(as_u(v)), static_cast<int>(j)))); };
        const float4 p0 = make_float4(from_lane(c0.x), from_lane(c0.y), from_lane(c0.z), from_lane(c0.w));
        const float4 p1 = make_float4(from_lane(c1.x), from_lane(c1.y), from_lane(c1.z), 0.0f);
        const uint32_t link = as_u(p1.z);
        bool emit = true;
        if ((link & 63u) == 0u) {
            const uint32_t m = link >> 6;
            float4 g0, g1;
            const uint32_t km = kept_of(m, g0, g1);
            const bool sticks_out = ((km >> lane) & 1u) != 0u && lane < slots &&
                                    !(p0.x <= g0.x && p0.y <= g0.y && p0.z <= g0.z && g0.w <= p0.w && g1.x <= p1.x && g1.y <= p1.y);
            if (km == 0u) {
                emit = false;
            } else if (__ballot(sticks_out) == 0 && depth < kListDepth && used + pend + static_cast<uint32_t>(__popc(km)) <= room) {
                if (mask != 0u) {
                    // (v_writelane_b32 takes its lane select from M0 here, as the walk's frame stack does: one SGPR operand per VALU instruction)
                    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tv_writelane_b32 %0, %3, m0\n\tv_writelane_b32 %1, %4, m0"
                                 : "+v"(st_node), "+v"(st_mask) : "s"(depth), "s"(__builtin_amdgcn_readfirstlane(cur)), "s"(__builtin_amdgcn_readfirstlane(mask)) : "m0");
                    depth++;
                }
                cur = m; mask = km; pend += static_cast<uint32_t>(__popc(km));
                c0 = g0; c1 = g1;
                emit = false;
            }
        }
        if (emit) {
            if (lane == 0u) mcache[static_cast<uint32_t>(kArenaBase) + top + used] = rec;
            used++;
        }
    }
    const uint32_t val = ((static_cast<uint32_t>(kArenaBase) + top) << 16) | used;
    if (lane == 0u) {
        const uint32_t slot = node_slot(node);
        mcache[static_cast<uint32_t>(kMaskCacheHeader) + slot] = node;
        mcache[static_cast<uint32_t>(kNodeListBase) + slot] = val;
        mcache[kArenaTopSlot] = ~(top + used);
    }
    wave_lds_sync();
    return val;
}

// ---- ... and packet-level TRIANGLE rejection with the same bounds --------------------------------------------------------------------
// Counted on the metric's frame (tools/sim_tri_reject.py): a pass of 64 rays through two pixels tests 53 triangles and 3.8 of them are
// hit by some ray; with the unit's bounds B (origins, directions) 41 of the 53 can be PROVEN missed by every ray inside B, once per
// work unit and leaf: the leaf's 64-bit mask "triangle i may be hit" is cached next to the node masks and a pass tests the survivors.
// The proof is the Moeller-Trumbore expression sequence of triangle.rs:183-217 itself, evaluated on intervals: every operation of
// it (fl(a*b), fl(a*b+c), fl(a-b), fl(1/x) on an interval without zero) is monotone in each operand while the others are fixed, so
// the same f32 operation evaluated at the corners of the operand intervals bounds the operation's result for every ray inside B --
// no error analysis, the bounds contain the very f32 values the per-ray test computes.  A triangle is skipped when the bounds show
// u < 0, v < 0, u + v > 1 or t < 0 for all of them (:125 then accepts for no ray).  No NaN can arise on the way: every origin bound
// is within 2^31, every direction bound within 2, every vertex within 2^30 and every edge within 2^31 (DevScene::tris_bounded,
// mask_cache_begin_pass), which keeps all intermediate bounds finite up to the reciprocal (|t numerator| < 2^98); a determinant
// interval that touches zero or has an infinite reciprocal keeps the triangle; after that every value is one product of finite
// numbers (never NaN), and the only sum (u + v) can at worst be inf - inf = NaN, which compares false and keeps the triangle.
// The far side alone: u.lo > 1 or v.lo > 1 also skips the triangle.  `u.lo + v.lo > 1` does not cover it: where v.lo is negative
// the sum can stay at or below 1 although every ray of the unit has u > 1, and each pass then loads the record only to leave at an
// early-out.  u.lo bounds from below the very f32 u of every ray inside B (the corner argument above), so u.lo > 1 gives u > 1 for
// all of them, and the walk accepts a ray only with !(min(u, v, t) < 0) & (u + v <= 1) (packet_walk.h, triangle.rs:125-129): with
// u > 1, a negative v fails the first test; a NaN v fails it as triangle.rs writes it (v >= 0) and, where a minNum chain drops it,
// makes u + v NaN, which fails the second; a v >= 0 (-0 included, u + -0 = u) gives fl(u + v) >= fl(u + 0) = u > 1, rounding being
// monotone, and fails the second.  The same with u and v exchanged.  The comparisons are strict: a ray through v1
// (u == 1, v == 0), through v2 (u == 0, v == 1) or on the far edge (u + v == 1) is accepted, and u.lo <= 1, v.lo <= 1 and
// u.lo + v.lo <= 1 there keep the triangle.  A NaN bound compares false and keeps it.  Counted (tools/tri_exit_count.py,
// profiles/mask_far_notes.md): the two terms take 11.6 surviving triangle tests per pass of the metric's frame to 9.6, none of the
// dropped ones accepted by any ray of its unit.  -DMP_NO_MASK_FAR: the rule without them (A/B builds, tools/build_variant.sh).
struct Iv {
    float lo, hi;
};
__device__ __forceinline__ Iv iv_neg(const Iv a) { return Iv{-a.hi, -a.lo}; }
__device__ __forceinline__ Iv iv_mul_c(const Iv a, const float c) {  // fl(a * c)
    const float p = a.lo * c, q = a.hi * c;
    return Iv{fminf(p, q), fmaxf(p, q)};
}
__device__ __forceinline__ Iv iv_mul(const Iv a, const Iv b) {  // fl(a * b)
    const float p1 = a.lo * b.lo, p2 = a.lo * b.hi, p3 = a.hi * b.lo, p4 = a.hi * b.hi;
    return Iv{fminf(fminf(p1, p2), fminf(p3, p4)), fmaxf(fmaxf(p1, p2), fmaxf(p3, p4))};
}
__device__ __forceinline__ Iv iv_fma_c(const Iv a, const float c, const Iv z) {  // fl(a * c + z)
    return Iv{fminf(__builtin_fmaf(a.lo, c, z.lo), __builtin_fmaf(a.hi, c, z.lo)), fmaxf(__builtin_fmaf(a.lo, c, z.hi), __builtin_fmaf(a.hi, c, z.hi))};
}
__device__ __forceinline__ Iv iv_fma(const Iv a, const Iv b, const Iv z) {  // fl(a * b + z)
    const float l1 = __builtin_fmaf(a.lo, b.lo, z.lo), l2 = __builtin_fmaf(a.lo, b.hi, z.lo), l3 = __builtin_fmaf(a.hi, b.lo, z.lo), l4 = __builtin_fmaf(a.hi, b.hi, z.lo);
    const float h1 = __builtin_fmaf(a.lo, b.lo, z.hi), h2 = __builtin_fmaf(a.lo, b.hi, z.hi), h3 = __builtin_fmaf(a.hi, b.lo, z.hi), h4 = __builtin_fmaf(a.hi, b.hi, z.hi);
    return Iv{fminf(fminf(l1, l2), fminf(l3, l4)), fmaxf(fmaxf(h1, h2), fmaxf(h3, h4))};
}
// can any ray with origin / direction inside the bounds `b` (mask-cache header) hit the triangle {v0, e1, e2}?  far_only (the probe's;
// the walk passes none and the stores fold away): set when the far-side terms alone say no
__device__ __forceinline__ bool tri_may_hit(const float* b, const float (&v0)[3], const float (&e1)[3], const float (&e2)[3], bool* far_only = nullptr) {
    if (far_only) *far_only = false;
    const Iv d[3] = {Iv{b[13], b[16]}, Iv{b[14], b[17]}, Iv{b[15], b[18]}};
    // h = (fms(dy, e2z, dz * e2y), fms(dz, e2x, dx * e2z), fms(dx, e2y, dy * e2x)) ; fms(a, b, c) = fma(a, b, -c)
    const Iv h[3] = {iv_fma_c(d[1], e2[2], iv_neg(iv_mul_c(d[2], e2[1]))), iv_fma_c(d[2], e2[0], iv_neg(iv_mul_c(d[0], e2[2]))),
                     iv_fma_c(d[0], e2[1], iv_neg(iv_mul_c(d[1], e2[0])))};
    // fma_dot(a, b) = fma(az, bz, fma(ay, by, ax * bx))
    const Iv det = iv_fma_c(h[2], e1[2], iv_fma_c(h[1], e1[1], iv_mul_c(h[0], e1[0])));
    if (!(det.lo > 0.0f || det.hi < 0.0f)) return true;
    const Iv inv = Iv{1.0f / det.hi, 1.0f / det.lo};
    if (!(fabsf(inv.lo) < INFINITY && fabsf(inv.hi) < INFINITY)) return true;
    const Iv s[3] = {Iv{b[0] - v0[0], b[3] - v0[0]}, Iv{b[1] - v0[1], b[4] - v0[1]}, Iv{b[2] - v0[2], b[5] - v0[2]}};
    const Iv u = iv_mul(inv, iv_fma(s[2], h[2], iv_fma(s[1], h[1], iv_mul(s[0], h[0]))));
    const Iv q[3] = {iv_fma_c(s[1], e1[2], iv_neg(iv_mul_c(s[2], e1[1]))), iv_fma_c(s[2], e1[0], iv_neg(iv_mul_c(s[0], e1[2]))),
                     iv_fma_c(s[0], e1[1], iv_neg(iv_mul_c(s[1], e1[0])))};
    const Iv v = iv_mul(inv, iv_fma(d[2], q[2], iv_fma(d[1], q[1], iv_mul(d[0], q[0]))));
    const Iv t = iv_mul(inv, iv_fma_c(q[2], e2[2], iv_fma_c(q[1], e2[1], iv_mul_c(q[0], e2[0]))));
    const bool miss = u.hi < 0.0f || v.hi < 0.0f || (u.lo + v.lo) > 1.0f || t.hi < 0.0f;
#ifndef MP_NO_MASK_FAR
    const bool far = u.lo > 1.0f || v.lo > 1.0f;
#else
    const bool far = false;
#endif
    if (far_only) *far_only = far && !miss;
    return !(miss || far);
}

// ---- the per-ray early-outs of a triangle test: "surely rejected" before the division ------------------------------------------------
// The walk computes det, then the numerators un, vn, tn of u = fl(inv_det * un), v, t (triangle.rs:183-217, inv_det = fl(1 / det):
// correctly rounded; rm::rcp_short is the same number) and accepts a ray iff u >= 0, v >= 0, fl(u + v) <= 1, t >= 0, t < limit.
// A wave leaves a triangle after un (stage 1) or after vn and tn (stage 2) when EVERY lane is surely rejected; a lane is surely
// rejected when its key is <= its threshold `thr`: -2^-40 for a live ray, +inf for a disabled one (always rejected).  The keys are
// minNum chains, so a NaN operand drops out and an all-NaN key compares false: NaN never rejects.
//   x = tri_flipped(det, num): the numerator with det's sign flipped in, or +1 where |det| > 2^40 or det is NaN (no verdict there).
// NEAR side (x <= -2^-40): num's sign differs from det's, |num| >= 2^-40 and |det| <= 2^40, so the quotient fl(fl(1/det) * num) is a
//   non-zero negative number (|quotient| >= 2^-80 (1 - eps): no underflow to -0, which would pass `>= 0`); det = +-0 or a denormal
//   with an infinite reciprocal gives -inf.  u >= 0 (v >= 0, t >= 0) fails.
// FAR side: f(x) = fl(|det| * (1 + 2^-20) - x), ONE rounding (fma).  f(x) <= -2^-40 means the exact difference is negative (a
//   non-negative real never rounds below zero): x > |det| (1 + 2^-20) =: A.  (The rule is x > A; demanding 2^-40 of the difference
//   lets the far side share the near side's threshold, hence its compare, and gives up only numerators within 2^-40 of A.)
//   * f(xu) <= -2^-40.  |det| is not above 2^40 here (x would be 1 and f positive or NaN).  If inv_det is finite, u = xu / |det|
//     (1 + d1)(1 + d2) with |d| <= 2^-24 (u is above 1: no underflow; an overflow gives +inf), so u > (1 + 2^-20)(1 - 2^-24)^2 >
//     1 + 2^-21.  If inv_det is infinite (det = +-0 or a small denormal), xu > 0 makes u = +inf.  Then v < 0 is rejected; v NaN
//     makes u + v NaN, and `<= 1` is false; v >= 0 gives fl(u + v) >= u > 1 (rounding is monotone).  The acceptance fails.
//   * f(fl(xu + xv)) <= -2^-40.  If the computed u or v is negative or NaN the acceptance fails by itself.  Otherwise each is the
//     rounded quotient of a numerator that is non-negative or so small that the quotient underflowed to -0 (it is then above
//     -2^-149 |det|); with xu + xv >= fl(xu + xv)(1 - 2^-24) > A (1 - 2^-24): u + v >= (xu + xv) / |det| (1 - 2^-24)^2 - 2^-148 >
//     (1 + 2^-20)(1 - 2^-24)^3 - 2^-148 > 1 + 2^-21, and its rounding is above 1.  With an infinite inv_det one of u, v is +inf
//     (the positive numerator's) and the sum is +inf or NaN.  The acceptance fails.
//   * |det| > 2^40 or NaN: x = 1 for every numerator, f = fl(|det| (1 + 2^-20) - 1 or - 2) is positive, +inf or NaN: never rejects,
//     as on the near side.
// Disabled lanes: thr = +inf, and every key that is not NaN is <= +inf; a NaN key (a disabled lane's garbage) keeps the wave at the
// triangle, which costs time and decides nothing -- as before.
// Counted (tools/tri_exit_count.py, profiles/tri_exits_notes.md): of the 8.3 triangles per pass of the metric's frame that reach the
// division, 3.6 are accepted by no ray, all of them on the far side; the far keys take them out at stage 1 or 2.
// -DMP_NO_FAR_EXIT: the near side alone (A/B builds, tools/build_variant.sh).
constexpr float kExitTiny = 9.094947017729282e-13f;  // 2^-40
constexpr float kExitHuge = 1099511627776.0f;        // 2^40
constexpr float kFarSlack = 1.00000095367431640625f; // 1 + 2^-20
__device__ __forceinline__ float tri_flipped(float det, float num) {
    return fabsf(det) <= kExitHuge ? as_f(as_u(num) ^ (as_u(det) & 0x80000000u)) : 1.0f;
}
__device__ __forceinline__ float tri_far_key(float det, float x) { return __builtin_fmaf(fabsf(det), kFarSlack, -x); }
__device__ __forceinline__ float tri_exit1_key(float det, float xu) {
#ifdef MP_NO_FAR_EXIT
    return xu;
#else
    return fminf(xu, tri_far_key(det, xu));
#endif
}
__device__ __forceinline__ float tri_exit2_key(float det, float xu, float xv, float xt) {
    const float near_key = fminf(fminf(xu, xv), xt);
#ifdef MP_NO_FAR_EXIT
    return near_key;
#else
    return fminf(fminf(near_key, tri_far_key(det, xu)), tri_far_key(det, xu + xv));
#endif
}

}  // namespace mc
}  // namespace mp
