// The ray-packet walks (DESIGN.md "Kernels"): one ray per lane, 64 rays share one traversal.  trace_packet_impl (the generic and the
// sign-specialised uncached walks over the register / LDS stacks), trace_packet_cached (the walk of the kernels with a per-unit
// mask cache, mask_cache.h, with its slow paths leaf_mask_slow and unit_list_slow), the dispatch between them (trace_packet) and
// the walk over the members of an object group (trace_packet_objects).  Used by kernels_tiles.hip, kernels_aov.hip,
// kernels_paths.hip and kernels_staged.hip (its camera stage), each of which compiles its own copy: a change here rebuilds those
// four units.  The walk with two rays per lane has one user and stands in kernels_tiles.hip.
#pragma once

#include "prof_counters.h"  // (before mask_cache.h: MP_PROF_COUNT)

#include "group_walk.h"
#include "launch_plan.h"

namespace mp {
namespace {

// ---- ray-packet traversal (coherent rays) --------------------------------------------------------------------
// One ray per lane, 64 rays share ONE traversal: the wavefront walks the BVH in the reference's canonical order
// (children pushed in ascending index, popped in descending, ray_bvh_intersection.rs:52-54,161 -- the reference
// never orders children by distance, so every ray's own visit sequence is a subsequence of this walk) and each lane
// applies its own ray's tests: the pop-time cull `node_t1 > best.t` (:40), the slab test against its own best.t
// (:149-162) and the triangle acceptance (:118-136).  A node / leaf is visited when at least one lane still needs
// it; lanes that the reference would not take there are masked.  Node and triangle data are wave-uniform and come
// through the scalar unit (s_load into SGPRs) from AoS copies of the scene; the per-lane entry distances of the
// shared stack live in LDS.
typedef const __attribute__((address_space(4))) float* kfp;      // constant address space => scalar loads
typedef const __attribute__((address_space(4))) uint32_t* kup;
typedef float krec8 __attribute__((ext_vector_type(8)));      // one 32-byte child record

constexpr float kTiny = 9.094947017729282e-13f;  // 2^-40
constexpr float kHuge = 1099511627776.0f;        // 2^40

// Early-out argument of the triangle tests (trace_packet_impl): a numerator whose sign differs from det's, with |num| >= 2^-40 and
// |det| <= 2^40, gives a quotient fl(fl(1/det) * num) that is certainly a non-zero negative number (|quotient| >= 2^-80(1-eps): no
// underflow to -0, which would pass `>= 0`).  det = +-0 or subnormal gives an infinite reciprocal whose sign still follows det.
// Flipping num's sign by det's turns "signs differ and |num| >= 2^-40" into one ordered compare against -2^-40; NaN never rejects.

struct PacketHit {
    float t, u, v;
    uint32_t prim;
};

// The shared traversal stack is wave-uniform and lives in four VGPRs used as 64-entry arrays (entry k = lane k, written with
// v_writelane, read with v_readlane, both with a scalar index and both regardless of EXEC): link, source slot (node*8+child, to
// re-derive the entry distance) and the 64-bit mask of lanes that passed the slab test when the entry was pushed.
// The pop-time cull `node_t1 > best.t` (:40) needs the ray's own entry distance t1: it can only fire for a lane whose best.t
// shrank after the push, so while no lane accepted a hit since then (entry not "stale") the pushed mask is the answer; otherwise
// t1 is recomputed from the child's box (same operations, same bits as at push time).  Staleness needs no per-entry state: the
// entries that predate the last change of any best.t are exactly those below a low-water mark of the stack pointer
// (`stale_top` in trace_packet_impl: set to sp when a leaf changed a best.t, lowered by every pop).
constexpr uint32_t kSrcRoot = 0xFFFFFFFFu;

template <bool PATCH_NAN, int OCT>
__device__ __forceinline__ float slab_entry(float bnx, float bny, float bnz, float bxx, float bxy, float bxz, const Ray& r) {
    float t1, t2;
    slab<PATCH_NAN, OCT>(bnx, bny, bnz, bxx, bxy, bxz, r, FLT_MAX, t1, t2);
    return t1;
}

// Wave-uniform stack in registers: four VGPRs used as 64-entry arrays.
struct RegStack {
    int link, src, mlo, mhi;
    __device__ __forceinline__ RegStack(float*, int) : link(0), src(0), mlo(0), mhi(0) {}
    // v_writelane_b32 ignores EXEC: a push made while only the rays of the current node are enabled still lands in lane `sp`
    // (gfx9 allows one SGPR operand per VALU instruction: the lane select goes through M0, which nothing else in these kernels uses)
    __device__ __forceinline__ void push(int sp, uint32_t l, uint32_t s, uint64_t m) {
        asm volatile(
            "s_mov_b32 m0, %4\n\ts_nop 0\n\t"
            "v_writelane_b32 %0, %5, m0\n\tv_writelane_b32 %1, %6, m0\n\tv_writelane_b32 %2, %7, m0\n\tv_writelane_b32 %3, %8, m0"
            : "+v"(link), "+v"(src), "+v"(mlo), "+v"(mhi)
            : "s"(sp), "s"(l), "s"(s), "s"(static_cast<uint32_t>(m)), "s"(static_cast<uint32_t>(m >> 32))
            : "m0");
    }
    __device__ __forceinline__ void pop(int sp, uint32_t& l, uint32_t& s, uint64_t& m) const {
        l = static_cast<uint32_t>(__builtin_amdgcn_readlane(link, sp));
        s = static_cast<uint32_t>(__builtin_amdgcn_readlane(src, sp));
        m = static_cast<uint32_t>(__builtin_amdgcn_readlane(mlo, sp)) |
            (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(mhi, sp))) << 32);
    }
    __device__ __forceinline__ void sync(int) {}
};

// Trees deeper than 9 levels (7*depth+1 > 64) can in principle need more entries: those above 63 go to LDS (one uint4
// {link, src, mask} per entry, written by lane 0, read back as a broadcast).  Real walks rarely get there
// (the 28-level atrium tree peaks at 16 entries per ray), so the register path stays the common one.
struct HybridStack {
    RegStack reg;
    uint4* ent;
    int lane;
    int nreg;  // entries kept in registers (<= 64; lowered only by the mp_ctx_set_option test knob)
    __device__ __forceinline__ HybridStack(float* lds, int lane_, uint32_t, uint32_t nreg_)
        : reg(nullptr, lane_), ent(reinterpret_cast<uint4*>(lds)), lane(lane_), nreg(static_cast<int>(nreg_)) {}
    __device__ __forceinline__ void push(int sp, uint32_t l, uint32_t s, uint64_t m) {
        if (sp < nreg) {
            reg.push(sp, l, s, m);
        } else if (lane == 0) {
            ent[sp - nreg] = make_uint4(l, s, static_cast<uint32_t>(m), static_cast<uint32_t>(m >> 32));
        }
    }
    __device__ __forceinline__ void pop(int sp, uint32_t& l, uint32_t& s, uint64_t& m) const {
        if (sp < nreg) {
            reg.pop(sp, l, s, m);
        } else {
            const uint4 e = ent[sp - nreg];
            l = __builtin_amdgcn_readfirstlane(e.x);
            s = __builtin_amdgcn_readfirstlane(e.y);
            m = __builtin_amdgcn_readfirstlane(e.z) | (static_cast<uint64_t>(__builtin_amdgcn_readfirstlane(e.w)) << 32);
        }
    }
    __device__ __forceinline__ void sync(int sp) { if (sp > nreg) wave_lds_sync(); }
};

__device__ __forceinline__ uint32_t uniform_u(float f) { return __builtin_amdgcn_readfirstlane(as_u(f)); }
// a wave-uniform 32-bit value the compiler must not fold into 64-bit address arithmetic (it would leave the scalar unit: v_mad_u64_u32)
__device__ __forceinline__ uint32_t scalar_u(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
// record i of a leaf whose first record is tp: base + a 32-bit byte offset (s_load's register-offset form: one s_mul_i32)
__device__ __forceinline__ kfp tri_record(kfp tp, uint32_t i) {
    return reinterpret_cast<kfp>(reinterpret_cast<const __attribute__((address_space(4))) char*>(tp) + scalar_u(i * static_cast<uint32_t>(kTriDwords * 4)));
}

// The triangle masks of one leaf (first packet `first`, n_real triangles), computed and stored in the unit's cache: lane j = triangle
// j, one coalesced read of the leaf's records.  A real call: its registers are needed once per unit and leaf, and inlined they
// would push the walk's per-ray state out of the 64 registers an 8-wave kernel has.
__device__ __noinline__ uint64_t leaf_mask_slow(const float* __restrict__ tris_aos, uint32_t* mcache, uint32_t first, uint32_t n_real) {
    const uint32_t j = threadIdx.x & 63u;
    bool keep = false;
    if (j < n_real) {
        const float* tv = tris_aos + (static_cast<size_t>(first) * 8 + j) * kTriDwords;
        const float v0[3] = {tv[0], tv[1], tv[2]}, e1[3] = {tv[3], tv[4], tv[5]}, e2[3] = {tv[6], tv[7], tv[8]};
        keep = tri_may_hit(reinterpret_cast<const float*>(mcache), v0, e1, e2);
    }
    const uint64_t todo = __ballot(keep);
#if defined(MP_PROF_MISSES) && defined(MP_PROF_MASK_TRIS)
    // counted builds with -DMP_PROF_MASK_TRIS: slot 2 is the number of triangles the built masks keep (not the inner links followed),
    // so slot 2 / slot 1 is the mean popcount of a stored mask (tools/cache_miss_count.py, tests/test_mask_far_side_gpu.py)
    if (j == 0u) atomicAdd(&g_prof[2], static_cast<unsigned long long>(__popcll(todo)));
#endif
    if (j == 0u) {
        const uint32_t ls = first & static_cast<uint32_t>(kLeafCacheEntries - 1);
        mcache[kLeafTagBase + ls] = first;
        reinterpret_cast<uint2*>(mcache + kLeafMaskBase)[ls] = make_uint2(static_cast<uint32_t>(todo), static_cast<uint32_t>(todo >> 32));
    }
    return todo;
}

// MODE 1: every active ray has finite inverse directions (no 0*inf, so the NaN patches of aabb.rs:262-267 are dead code).
// MODE 2: literal aabb.rs:254-284.
//
// The walk is fed by the scalar unit (wave-uniform node / triangle records through s_load), and measured on MI355X it is the
// SCALAR ALU, one per CU, that saturates first (profiles/r02_notes.md: an extra SALU instruction per triangle costs 4x what an
// extra VALU instruction costs).  So per-ray predicates that used to be combined as lane masks with s_and / s_andn2 / s_cmp are
// folded into the vector domain: the rays a popped entry is NOT live for are disabled through two per-lane operands -- `lim`
// (best.t, or -1 for a disabled ray: no slab interval and no hit distance passes) and `thr` (the early-out threshold -2^-40, or
// +inf: a disabled ray is always "surely rejected") -- so every ballot below is already the masked result and "no ray left" is a
// branch on VCC; det's magnitude guard is a v_cndmask, the three sign tests one minNum chain; loops are single-exit pair loops
// with a scalar countdown; pushes are v_writelane; staleness is a low-water mark instead of a 64-bit mask.
template <int MODE, int OCT, class Stack>
__device__ __forceinline__ void trace_packet_impl(const DevScene& sc, const Ray& r, bool active, Stack& st, PacketHit& hit) {
    constexpr bool PATCH_NAN = MODE == 2;
    // MODE 2 walks the literal reference tree, MODE 1 the wide tree (thin nodes absorbed into their parents: bit-identical hits
    // for rays with finite inverse directions, device_tree.cpp)
    kfp nodes = (kfp)(uintptr_t)(PATCH_NAN ? sc.nodes_lit : sc.nodes_aos);
    kfp tris = (kfp)(uintptr_t)sc.tris_aos;
    float best_t = FLT_MAX, bu = 0.0f, bv = 0.0f;  // best (:34-37)
    uint32_t bprim = kNoPrim;
    // entry 0 = root (:28-32), t1 = -inf: never culled
    st.push(0, PATCH_NAN ? sc.root_lit : sc.root, kSrcRoot, __ballot(active));
    st.sync(1);
    int sp = 1;
    int stale_top = 0;  // entries [0, stale_top) were pushed before some ray's best.t last changed
    while (sp > 0) {
        sp--;
        uint32_t link, src;
        uint64_t onm;  // rays this entry is still live for
        st.pop(sp, link, src, onm);
        if (sp < stale_top) {  // :40-44, per ray (the root is popped first, before anything can be stale)
            stale_top = sp;
            const krec8 bx = *reinterpret_cast<const __attribute__((address_space(4))) krec8*>(nodes + static_cast<size_t>(src) * 8);  // one load
            const float node_t1 = slab_entry<PATCH_NAN, OCT>(bx[0], bx[1], bx[2], bx[3], bx[4], bx[5], r);
            onm &= ~mask_gt(node_t1, best_t);
        }
        if (onm == 0) continue;
        const bool on = __builtin_amdgcn_inverse_ballot_w64(onm);
        float lim = on ? best_t : -1.0f;          // slab limit / hit-distance bound: nothing passes for a disabled ray
        if ((link & 63u) == 0u) {  // device link (mp_internal.h): inner = index << 6, leaf = first packet << 6 | real triangles
            // InnerNode::intersect :149-162, children ascending.  Child record = {min.xyz, max.xyz, link, n}: n (record 0 only)
            // = index of the node's last real child + 1.  Two SGPR sets alternate: B is fetched while A is tested.
            const uint32_t node = link >> 6;
            kfp nd = nodes + static_cast<size_t>(node) * 64;
            auto child = [&](const float b0, const float b1, const float b2, const float b3, const float b4, const float b5,
                             const float blink, const uint32_t cslot) {
                const uint32_t cl = uniform_u(blink);
                if (cl == MP_LINK_NULL) return;  // Null links are skipped at pop in the reference (:49)
                float t1, t2;
                if (PATCH_NAN) {
                    slab<PATCH_NAN, OCT>(b0, b1, b2, b3, b4, b5, r, lim, t1, t2);
                } else {
                    // aabb.rs:254-284 in two stages (round 3): t1 = max(lo.x, 0, lo.y, lo.z) and t2 = min(hi.x, limit, hi.y, hi.z) are
                    // the same numbers in any order of evaluation (max / min of the same operands), and max(lo.x, lo.y, 0) >
                    // min(hi.x, hi.y, limit) already decides t1 > t2.  Counted on the metric's frame (profiles/r03_notes.md): for
                    // 60 % of the child boxes a packet tests, no ray survives the x and y slabs -- the z slab and the rest are
                    // skipped for the whole wave (11 instead of 17 VALU).  Which two axes go first is a compile-time choice.
#ifndef MP_SLAB_LAST
#define MP_SLAB_LAST 2  // the axis whose slab is tested last (A/B-measured: profiles/r03_notes.md)
#endif
                    constexpr int A2 = MP_SLAB_LAST, A0 = (A2 + 1) % 3, A1 = (A2 + 2) % 3;
                    const float bn[3] = {b0, b1, b2}, bx3[3] = {b3, b4, b5}, ro[3] = {r.ox, r.oy, r.oz}, ri[3] = {r.ix, r.iy, r.iz};
                    const float a0_ = (bn[A0] - ro[A0]) * ri[A0], c0_ = (bx3[A0] - ro[A0]) * ri[A0];
                    const float a1_ = (bn[A1] - ro[A1]) * ri[A1], c1_ = (bx3[A1] - ro[A1]) * ri[A1];
                    float lo0, hi0, lo1, hi1;
                    if (OCT >= 0) {
                        lo0 = ((OCT >> A0) & 1) ? c0_ : a0_; hi0 = ((OCT >> A0) & 1) ? a0_ : c0_;
                        lo1 = ((OCT >> A1) & 1) ? c1_ : a1_; hi1 = ((OCT >> A1) & 1) ? a1_ : c1_;
                    } else {
                        lo0 = fminf(a0_, c0_); hi0 = fmaxf(a0_, c0_); lo1 = fminf(a1_, c1_); hi1 = fmaxf(a1_, c1_);
                    }
                    const float t1p = fmaxf(fmaxf(lo0, 0.0f), lo1), t2p = fminf(fminf(hi0, lim), hi1);
                    if (__ballot(t1p <= t2p) == 0) return;
                    const float a2_ = (bn[A2] - ro[A2]) * ri[A2], c2_ = (bx3[A2] - ro[A2]) * ri[A2];
                    float lo2, hi2;
                    if (OCT >= 0) { lo2 = ((OCT >> A2) & 1) ? c2_ : a2_; hi2 = ((OCT >> A2) & 1) ? a2_ : c2_; }
                    else { lo2 = fminf(a2_, c2_); hi2 = fmaxf(a2_, c2_); }
                    t1 = fmaxf(t1p, lo2);
                    t2 = fminf(t2p, hi2);
                }
                const uint64_t okm = __ballot(t1 <= t2);
                if (okm != 0) {
                    st.push(sp, cl, cslot, okm);
                    sp++;
                }
            };
            float a0 = nd[0], a1 = nd[1], a2 = nd[2], a3 = nd[3], a4 = nd[4], a5 = nd[5], a6 = nd[6];
            const uint32_t nchild = uniform_u(nd[7]);
            uint32_t slot = node * 8u;
            for (uint32_t p = nchild >> 1; p > 0; p--) {
                const float b0 = nd[8], b1 = nd[9], b2 = nd[10], b3 = nd[11], b4 = nd[12], b5 = nd[13], b6 = nd[14];
                child(a0, a1, a2, a3, a4, a5, a6, slot);
                a0 = nd[16]; a1 = nd[17]; a2 = nd[18]; a3 = nd[19]; a4 = nd[20]; a5 = nd[21]; a6 = nd[22];
                child(b0, b1, b2, b3, b4, b5, b6, slot + 1u);
                slot += 2u;
                nd += 16;
            }
            if (nchild & 1u) child(a0, a1, a2, a3, a4, a5, a6, slot);
            st.sync(sp);
        } else {
            // intersect_triangles :104-140 ; every lane walks the leaf's triangles in (packet, lane) order with a
            // strict `<`.  Padding (only at the tail of the last packet) can never be accepted and is not visited.
            const uint32_t first = link >> 6, n_real = link & 63u;  // the count travels in the link: no dependent load before the first triangle
            kfp tp = tris + static_cast<size_t>(first) * (8 * kTriDwords);
            const float thr = on ? -kTiny : INFINITY;  // early-out threshold: a disabled ray is always "surely rejected"
            uint64_t changed = 0;  // lanes that accepted a hit in this leaf
            auto test = [&](const float v0x, const float v0y, const float v0z, const float e1x, const float e1y, const float e1z,
                            const float e2x, const float e2y, const float e2z, const uint32_t tri) {
                // triangle.rs:183-217
                const float hx = fms(r.dy, e2z, r.dz * e2y), hy = fms(r.dz, e2x, r.dx * e2z), hz = fms(r.dx, e2y, r.dy * e2x);
                const float det = fma_dot(e1x, e1y, e1z, hx, hy, hz);
                const float sx = r.ox - v0x, sy = r.oy - v0y, sz = r.oz - v0z;
                const float un = fma_dot(sx, sy, sz, hx, hy, hz);
                // Exact early-outs.  A numerator whose sign differs from det's, with |num| >= 2^-40 and |det| <= 2^40, gives a
                // non-zero negative quotient fl(fl(1/det) * num) (no underflow to -0, which would pass `>= 0`): u >= 0 (v >= 0,
                // t >= 0) cannot hold.  x = num with its sign flipped by det's (or +1 where |det| is too large to tell):
                // "surely negative" is the single ordered compare x <= -2^-40; NaN never rejects.
                const uint32_t det_sign = as_u(det) & 0x80000000u;
                const bool det_ok = fabsf(det) <= kHuge;
                const float xu = det_ok ? as_f(as_u(un) ^ det_sign) : 1.0f;
                if (__ballot(!(xu <= thr)) == 0) return;  // no live ray can have u >= 0
                const float qx = fms(sy, e1z, sz * e1y), qy = fms(sz, e1x, sx * e1z), qz = fms(sx, e1y, sy * e1x);
                const float vn = fma_dot(r.dx, r.dy, r.dz, qx, qy, qz);
                const float tn = fma_dot(e2x, e2y, e2z, qx, qy, qz);
                const float xv = det_ok ? as_f(as_u(vn) ^ det_sign) : 1.0f, xt = det_ok ? as_f(as_u(tn) ^ det_sign) : 1.0f;
                // minNum drops NaN operands, so the minimum is <= the threshold iff one of the three ordered compares holds
                if (__ballot(!(fminf(fminf(xu, xv), xt) <= thr)) == 0) return;
                const float inv_det = 1.0f / det;
                const float u = inv_det * un, v = inv_det * vn, t = inv_det * tn;
                // mask & t>=0 & t<=max_t (:125), strict `<` vs the leaf best, then vs the global best (:129,:59):
                // equivalent to a running strict `<` against best.t (best.t never exceeds max_t); lim == best.t for live rays
                const bool acc = (u >= 0.0f) & (v >= 0.0f) & ((u + v) <= 1.0f) & (t >= 0.0f) & (t < lim);
                best_t = acc ? t : best_t;
                lim = acc ? t : lim;
                bu = acc ? u : bu;
                bv = acc ? v : bv;
                bprim = acc ? tri : bprim;
                changed |= __ballot(acc);
            };
            // two register sets (A, B) alternate: B is fetched while A is tested and vice versa (the array has tail padding)
            float a0 = tp[0], a1 = tp[1], a2 = tp[2], a3 = tp[3], a4 = tp[4], a5 = tp[5], a6 = tp[6], a7 = tp[7], a8 = tp[8];
            uint32_t tri = first * 8u;
            for (uint32_t p = n_real >> 1; p > 0; p--) {
                const float b0 = tp[9], b1 = tp[10], b2 = tp[11], b3 = tp[12], b4 = tp[13], b5 = tp[14], b6 = tp[15], b7 = tp[16], b8 = tp[17];
                test(a0, a1, a2, a3, a4, a5, a6, a7, a8, tri);
                a0 = tp[18]; a1 = tp[19]; a2 = tp[20]; a3 = tp[21]; a4 = tp[22]; a5 = tp[23]; a6 = tp[24]; a7 = tp[25]; a8 = tp[26];
                test(b0, b1, b2, b3, b4, b5, b6, b7, b8, tri + 1u);
                tri += 2u;
                tp += 2 * kTriDwords;
            }
            if (n_real & 1u) test(a0, a1, a2, a3, a4, a5, a6, a7, a8, tri);
            if (changed != 0) stale_top = sp;  // every entry still on the stack predates this change
        }
    }
    hit.t = best_t; hit.u = bu; hit.v = bv; hit.prim = bprim;
}

// Wave-uniform stack of the cached walk: three VGPRs used as 64-entry arrays.  An entry is a FRAME -- a visited node with the children
// that are still to be popped (node << MB | MB-bit mask, see trace_packet_cached) and the 64-bit mask of the rays that were live at the visit.  The frame on
// top lives in scalar registers: popping a child is three scalar instructions, and the arrays are touched once per node visit
// instead of once per child.
struct RegStack3 {
    int ent, mlo, mhi;
    __device__ __forceinline__ RegStack3() : ent(0), mlo(0), mhi(0) {}
    __device__ __forceinline__ void push(int sp, uint32_t e, uint64_t m) {
        asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\t"
                     "v_writelane_b32 %0, %4, m0\n\tv_writelane_b32 %1, %5, m0\n\tv_writelane_b32 %2, %6, m0"
                     : "+v"(ent), "+v"(mlo), "+v"(mhi)
                     : "s"(sp), "s"(e), "s"(static_cast<uint32_t>(m)), "s"(static_cast<uint32_t>(m >> 32))
                     : "m0");
    }
    __device__ __forceinline__ void pop(int sp, uint32_t& e, uint64_t& m) const {
        e = static_cast<uint32_t>(__builtin_amdgcn_readlane(ent, sp));
        m = static_cast<uint32_t>(__builtin_amdgcn_readlane(mlo, sp)) |
            (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(mhi, sp))) << 32);
    }
};

// The sign-specialised walk of a kernel with a per-unit mask cache (MaskCache, tri_may_hit; `mcache` = this wave's header and
// entries; every active ray has finite inverse directions of the sign pattern OCT and lies inside the cache's bounds).
// Same visits, same per-ray decisions as trace_packet_impl<1, OCT>, organised around the cache: a node visit is ONE lookup and
// opens a frame with the children some ray of the unit may pass, WITHOUT testing them; a child's per-ray slab test runs when it is
// popped from its frame (highest index first: the reference pushes ascending and pops descending, :161), against best.t as it is
// then.  That is the reference's decision: it pushes a child when t1 <= min(hi, best.t at the visit) (:158) and visits it when
// !(t1 > best.t at the pop) (:40); best.t only shrinks and t1 is never NaN here, so both hold exactly when t1 <= min(hi, best.t
// at the pop) -- one test with the later limit -- for a ray that was live at the parent's visit (the frame carries that mask: a
// child box may stick out of its parent's by an ulp).  No entry distance is stored or recomputed, no record is fetched at the
// visit, and the child's record -- box and link -- is one 32-byte scalar load at the pop.  The root is child 0 of a pseudo-node
// behind the last node: its record (device_tree.cpp) is an unbounded box, which every ray passes with t1 = 0 -- never culled (:28-32).
// The walk has a tree of its own, sc.nodes_pk: the PACKET tree (device_tree.cpp), 16 child slots per node, or, for a scene whose
// packet tree would not fit 16-bit node indices, the wide tree again with 8 (DevScene::pk_mask_bits = slots per node, a runtime
// value here: only the list builder needs it).
// A frame is a LIST (mask_cache.h, unit_list_build): the kept children of the node, with the kept children of absorbed inner
// children in their place.  Frame word = (dword index of the list's first entry in the wave's cache) << 16 | entries still to pop;
// popping takes the last entry -- the record index node * slots + slot -- from LDS.  An inner link is looked up by node index in
// the unit's table; a miss builds the list (unit_list_slow, a real call: once or twice per unit).  Returns false when a list did
// not fit the arena while frames of this walk still pointed into it: table and arena are reset, and the caller walks this pass
// without the cache (the same hits: every walk computes the reference's).  (Beginning the pass again as a cached walk on the
// emptied arena was built and measured: the restart state costs the flagship 0.6 ms, 15.3 against 14.7 ms, for a case that its
// frame never meets -- tools/cache_miss_count.py prints how often a frame does.)
template <int OCT>
__device__ __noinline__ uint32_t unit_list_slow(const float* __restrict__ nodes_pk, uint32_t* mcache, uint32_t node, uint32_t slots) {
    return unit_list_build(reinterpret_cast<const float4*>(nodes_pk), mcache, node, slots,
                           [](const float* b, const float bmn[3], const float bmx[3]) { return bounds_may_hit<OCT>(b, bmn, bmx); });
}
template <int OCT>
__device__ __forceinline__ bool trace_packet_cached(const DevScene& sc, const Ray& r, bool active, PacketHit& hit, uint32_t* mcache) {
    static_assert(kNullLink == MP_LINK_NULL, "mask_cache.h's copy of the null link");
    kfp nodes = (kfp)(uintptr_t)sc.nodes_pk;
    kfp tris = (kfp)(uintptr_t)sc.tris_aos;
    float best_t = FLT_MAX, bu = 0.0f, bv = 0.0f;  // best (:34-37)
    uint32_t bprim = kNoPrim;
    RegStack3 st;
    int sp = 0;                                   // frames below the current one
    // the first frame: a list of one entry, the root's record (child 0 of the pseudo-node behind the last node); every lane stores the same dword
    mcache[kRootListSlot] = sc.pk_count * sc.pk_mask_bits;
    wave_lds_sync();
    uint32_t cur = (static_cast<uint32_t>(kRootListSlot) << 16) | 1u;
    uint64_t pm = __ballot(active);               // the rays that were live at the current frame's visit
    // (fetching the record of the child that is popped next ahead of its pop was built and measured slower: 27.0 against 24.3 ms)
    for (;;) {
        if ((cur & 0xFFFFu) == 0u) {  // frame exhausted: back to the one below
            if (sp == 0) break;
            sp--;
            st.pop(sp, cur, pm);
        }
        cur -= 1u;  // last entry first
        const uint32_t src = __builtin_amdgcn_readfirstlane(mcache[(cur >> 16) + (cur & 0xFFFFu)]);
#ifndef MP_NO_EMPTY_SKIP
        // An entry with kEmptyLeafBit set is a leaf whose unit triangle mask is empty (marked below by the visit that found it so):
        // a visit would test no triangle and change no ray's state, so the record load and the slab test are skipped too.  The mask
        // depends on the leaf and the unit's bounds alone, and whatever changes the bounds or resets the arena rebuilds the lists,
        // unmarked, before they are walked again.  Record indices are below 2^28 (2^24 nodes x 16 slots, checked at upload).
        if (static_cast<int32_t>(src) < 0) {
            MP_PROF_COUNT(7);
            continue;
        }
#endif
        const bool pon = __builtin_amdgcn_inverse_ballot_w64(pm);
        // (base + a 32-bit byte offset: s_load's register-offset form; fewer than 2^24 nodes, checked at upload)
        const krec8 rec = *reinterpret_cast<const __attribute__((address_space(4))) krec8*>(reinterpret_cast<const __attribute__((address_space(4))) char*>(nodes) + scalar_u(src * 32u));
        float t1, t2;
        slab<false, OCT>(rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], r, pon ? best_t : -1.0f, t1, t2);  // aabb.rs:254-284
        const bool ok = t1 <= t2;
        if (__ballot(ok) == 0) continue;
        const uint32_t link = uniform_u(rec[6]);
        float lim = ok ? best_t : -1.0f;  // best.t for the rays this child is live for, -1 for the others: no slab interval and no hit distance passes
        if ((link & 63u) == 0u) {  // inner node (device link, mp_internal.h)
#ifndef MP_PROF_MASK_TRIS  // (that build counts surviving triangles in this slot: leaf_mask_slow)
            MP_PROF_COUNT(2);
#endif
            const uint32_t node = link >> 6;
            const uint32_t slot = node_slot(node);
            const uint32_t tag = __builtin_amdgcn_readfirstlane(mcache[static_cast<uint32_t>(kMaskCacheHeader) + slot]);
            uint32_t list = __builtin_amdgcn_readfirstlane(mcache[static_cast<uint32_t>(kNodeListBase) + slot]);
            if (__builtin_expect(tag != node, 0)) {  // first visit of this node under the current bounds, or its entry was evicted
                MP_PROF_COUNT(0);
                if (tag != 0xFFFFFFFFu) MP_PROF_COUNT(4);
                list = __builtin_amdgcn_readfirstlane(unit_list_slow<OCT>(sc.nodes_pk, mcache, node, sc.pk_mask_bits));
                if (list == kListOverflow) {
                    if (sp != 0 || (cur & 0xFFFFu) != 0u) {  // frames of this walk point into the arena that was reset
                        MP_PROF_COUNT(6);
                        return false;
                    }
                    list = __builtin_amdgcn_readfirstlane(unit_list_slow<OCT>(sc.nodes_pk, mcache, node, sc.pk_mask_bits));  // fits the empty arena
                }
            }
            if ((list & 0xFFFFu) != 0u) {  // a new frame; the one it replaces goes to the arrays if it still has entries
                if ((cur & 0xFFFFu) != 0u) {
                    st.push(sp, cur, pm);
                    sp++;
                }
                cur = list;
                pm = __ballot(lim >= 0.0f);
            }
        } else {
            // intersect_triangles :104-140 ; every lane walks the leaf's surviving triangles in (packet, lane) order with a strict `<`
            const uint32_t first = link >> 6, n_real = link & 63u;
            kfp tp = tris + static_cast<size_t>(first) * (8 * kTriDwords);
            static_assert(kExitTiny == kTiny && kExitHuge == kHuge, "mask_cache.h's copies of the early-out constants");
            const float thr = lim >= 0.0f ? -kTiny : INFINITY;  // early-out threshold: a disabled ray is always "surely rejected"
            auto test = [&](const float v0x, const float v0y, const float v0z, const float e1x, const float e1y, const float e1z,
                            const float e2x, const float e2y, const float e2z, const uint32_t tri) {
                // triangle.rs:183-217
                const float hx = fms(r.dy, e2z, r.dz * e2y), hy = fms(r.dz, e2x, r.dx * e2z), hz = fms(r.dx, e2y, r.dy * e2x);
                const float det = fma_dot(e1x, e1y, e1z, hx, hy, hz);
                const float sx = r.ox - v0x, sy = r.oy - v0y, sz = r.oz - v0z;
                const float un = fma_dot(sx, sy, sz, hx, hy, hz);
                // the two early-outs, near side and far side (mask_cache.h: tri_exit1_key, tri_exit2_key and their proof)
                const float xu = tri_flipped(det, un);
                if (__ballot(!(tri_exit1_key(det, xu) <= thr)) == 0) return;  // no live ray can have 0 <= u <= 1
                const float qx = fms(sy, e1z, sz * e1y), qy = fms(sz, e1x, sx * e1z), qz = fms(sx, e1y, sy * e1x);
                const float vn = fma_dot(r.dx, r.dy, r.dz, qx, qy, qz);
                const float tn = fma_dot(e2x, e2y, e2z, qx, qy, qz);
                const float xv = tri_flipped(det, vn), xt = tri_flipped(det, tn);
                if (__ballot(!(tri_exit2_key(det, xu, xv, xt) <= thr)) == 0) return;  // ... nor u, v, t >= 0 with u + v <= 1
                // inv_det = 1 / det (:201) through rm::rcp_short when every lane's |det| lies in its window [2^-94, 2^125] (ray_math.h:
                // there the short sequence is the IEEE division's own, minus range fix-ups that do nothing, so inv_det is the same
                // number); otherwise the whole wave divides.  Only live rays need the window (the others cannot accept: t < lim < 0
                // fails); testing every lane is stricter and keeps the guard at one compare and a branch on VCC.  The test is on the
                // magnitude bits: bits(det) << 1 drops the sign and keeps the order of |det| (NaN above +inf), and one unsigned compare
                // of the offset checks both ends: +-0, denormals, tiny, huge, inf and NaN all fall outside.
                constexpr uint32_t kRcpLo = 0x10800000u /* 2^-94 */, kRcpHi = 0x7E000000u /* 2^125 */;
                const uint32_t wkey = (as_u(det) << 1) - (kRcpLo << 1);
                const float inv_det = __ballot(wkey > ((kRcpHi - kRcpLo) << 1)) == 0 ? rm::rcp_short(det) : 1.0f / det;
                const float u = inv_det * un, v = inv_det * vn, t = inv_det * tn;
                // :125, :129, :59 -- (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t < lim) in fewer compares.  Without NaN operands
                // minNum is the minimum and `< 0` is false for -0, as `-0 >= 0` is true; a NaN in u or v makes u + v NaN and fails the
                // sum test, a NaN in t fails `t < lim`, so the cases where minNum drops a NaN operand are decided by the other tests.
                const bool acc = !(fminf(fminf(u, v), t) < 0.0f) & ((u + v) <= 1.0f) & (t < lim);
                best_t = acc ? t : best_t;
                lim = acc ? t : lim;
                bu = acc ? u : bu;
                bv = acc ? v : bv;
                bprim = acc ? tri : bprim;
            };
            // per-unit triangle masks (see tri_may_hit): which triangles of this leaf can ANY ray inside the unit's bounds hit?
            const uint32_t ls = first & static_cast<uint32_t>(kLeafCacheEntries - 1);
            const uint32_t tag = mcache[kLeafTagBase + ls];
            const uint2 tm = reinterpret_cast<const uint2*>(mcache + kLeafMaskBase)[ls];
            uint64_t todo;
            if (__builtin_expect(__builtin_amdgcn_readfirstlane(tag) == first, 1)) {
                todo = __builtin_amdgcn_readfirstlane(tm.x) | (static_cast<uint64_t>(__builtin_amdgcn_readfirstlane(tm.y)) << 32);
            } else {  // first visit of this leaf under the current bounds
                MP_PROF_COUNT(1);
                const uint64_t m = leaf_mask_slow(sc.tris_aos, mcache, first, n_real);  // (a call's result is not known to be uniform)
                todo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(m)) | (static_cast<uint64_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(m >> 32))) << 32);
            }
            // the next survivor's record is fetched while this one is tested (one register set rotated through moves: a two-set
            // form without the moves measured 3 % slower -- code size; no prefetch at all: the same time)
#ifndef MP_NO_EMPTY_SKIP
            if (todo == 0 && (cur >> 16) != static_cast<uint32_t>(kRootListSlot)) {
                // nothing to test here for any ray inside the unit's bounds: mark the list entry this leaf was popped from, so that
                // the unit's later pops of it stop at the entry (above).  The root's own slot is rewritten by every pass: not marked.
                if ((threadIdx.x & 63u) == 0u) mcache[(cur >> 16) + (cur & 0xFFFFu)] = src | kEmptyLeafBit;
                wave_lds_sync();
            }
#endif
            if (todo != 0) {
                uint32_t c = static_cast<uint32_t>(__builtin_ctzll(todo));
                todo &= ~(1ull << c);
                kfp ta = tri_record(tp, c);
                krec8 ra = *reinterpret_cast<const __attribute__((address_space(4))) krec8*>(ta);  // (one block of eight registers: rotated with 64-bit moves)
                float a8 = ta[8];
                while (todo != 0) {
                    const uint32_t cn = static_cast<uint32_t>(__builtin_ctzll(todo));
                    todo &= ~(1ull << cn);
                    kfp tb = tri_record(tp, cn);
                    const krec8 rb = *reinterpret_cast<const __attribute__((address_space(4))) krec8*>(tb);
                    const float b8 = tb[8];
                    test(ra[0], ra[1], ra[2], ra[3], ra[4], ra[5], ra[6], ra[7], a8, first * 8u + c);
                    ra = rb; a8 = b8;
                    c = cn;
                }
                test(ra[0], ra[1], ra[2], ra[3], ra[4], ra[5], ra[6], ra[7], a8, first * 8u + c);
            }
        }
    }
    hit.t = best_t; hit.u = bu; hit.v = bv; hit.prim = bprim;
    return true;
}

// OCTANTS: also instantiate the eight sign-specialised walks (the production kernels; the rest keep the generic slab).
template <bool OCTANTS, class Stack, bool MC = false>
__device__ __forceinline__ void trace_packet(const DevScene& sc, const Ray& r, bool active, Stack& st, PacketHit& hit,
                                             const MaskCache& mc = MaskCache{nullptr}) {
    if (OCTANTS && MC) {
        // Kernels with a mask cache: the sign-specialised walks use it, and a pass with a ray that fails mask_cache_ray_ok takes a
        // generic walk.  The same choices as below, in another order: a ray with an infinite inverse component fails
        // mask_cache_ray_ok, so a pass where every active ray passes is not `slow`; a pass where one fails takes the literal walk
        // if it is slow and the generic MODE 1 walk otherwise (whether its signs are uniform or not).
        auto cached = [&](const uint32_t oct) -> bool {  // false: a list did not fit the arena in mid-walk
            switch (oct) {
                case 0: return trace_packet_cached<0>(sc, r, active, hit, mc.lds);
                case 1: return trace_packet_cached<1>(sc, r, active, hit, mc.lds);
                case 2: return trace_packet_cached<2>(sc, r, active, hit, mc.lds);
                case 3: return trace_packet_cached<3>(sc, r, active, hit, mc.lds);
                case 4: return trace_packet_cached<4>(sc, r, active, hit, mc.lds);
                case 5: return trace_packet_cached<5>(sc, r, active, hit, mc.lds);
                case 6: return trace_packet_cached<6>(sc, r, active, hit, mc.lds);
                default: return trace_packet_cached<7>(sc, r, active, hit, mc.lds);
            }
        };
#ifndef MP_NO_ENTRY_FOLD
        // One bounds test first (mask_cache.h, mask_cache_pass_inside, with the argument): a pass whose every active ray lies inside
        // a valid B needs none of the guards in the block below -- mask_cache_ray_ok, the infinite-inverse test, the sign ballots,
        // mask_cache_begin_pass: all implied -- and enters the cached walk of B's pattern at once, B unchanged.  Any other pass (no
        // valid B, a ray outside B, a NaN or infinite component, mixed signs) goes through the block as before.
        // -DMP_NO_ENTRY_FOLD: the block for every pass (A/B builds, tools/build_variant.sh).
        uint32_t oct = sc.boxes_ordered ? mask_cache_pass_inside(mc, r, active) : kNoPattern;
        if (oct != kNoPattern) MP_PROF_COUNT(10);
        if (oct == kNoPattern) {
            if (__ballot(active & !mask_cache_ray_ok(r)) != 0) {
                const bool slow = active && (fabsf(r.ix) == INFINITY || fabsf(r.iy) == INFINITY || fabsf(r.iz) == INFINITY);
                if (__ballot(slow) != 0) trace_packet_impl<2, -1>(sc, r, active, st, hit);
                else trace_packet_impl<1, -1>(sc, r, active, st, hit);
                return;
            }
            if (sc.boxes_ordered) {
                const uint64_t am = __ballot(active);
                const uint64_t nx = __ballot(active && r.ix < 0.0f), ny = __ballot(active && r.iy < 0.0f), nz = __ballot(active && r.iz < 0.0f);
                if ((nx == 0 || nx == am) && (ny == 0 || ny == am) && (nz == 0 || nz == am)) {
                    oct = (nx ? 1u : 0u) | (ny ? 2u : 0u) | (nz ? 4u : 0u);
                    mask_cache_begin_pass(mc, r, active, oct);
                    MP_PROF_COUNT(11);
                }
            }
        }
        if (oct != kNoPattern && cached(oct)) return;
#else
        if (__ballot(active & !mask_cache_ray_ok(r)) != 0) {
            const bool slow = active && (fabsf(r.ix) == INFINITY || fabsf(r.iy) == INFINITY || fabsf(r.iz) == INFINITY);
            if (__ballot(slow) != 0) trace_packet_impl<2, -1>(sc, r, active, st, hit);
            else trace_packet_impl<1, -1>(sc, r, active, st, hit);
            return;
        }
        if (sc.boxes_ordered) {
            const uint64_t am = __ballot(active);
            const uint64_t nx = __ballot(active && r.ix < 0.0f), ny = __ballot(active && r.iy < 0.0f), nz = __ballot(active && r.iz < 0.0f);
            if ((nx == 0 || nx == am) && (ny == 0 || ny == am) && (nz == 0 || nz == am)) {
                const uint32_t oct = (nx ? 1u : 0u) | (ny ? 2u : 0u) | (nz ? 4u : 0u);
                mask_cache_begin_pass(mc, r, active, oct);
                MP_PROF_COUNT(11);
                if (cached(oct)) return;
            }
        }
#endif
        trace_packet_impl<1, -1>(sc, r, active, st, hit);  // (mixed signs, or a list did not fit: the generic walk, from the start)
        return;
    }
    const bool slow = active && (fabsf(r.ix) == INFINITY || fabsf(r.iy) == INFINITY || fabsf(r.iz) == INFINITY);
    if (__ballot(slow) != 0) {
        trace_packet_impl<2, -1>(sc, r, active, st, hit);
        return;
    }
    if (OCTANTS && sc.boxes_ordered) {
        const uint64_t am = __ballot(active);
        const uint64_t nx = __ballot(active && r.ix < 0.0f), ny = __ballot(active && r.iy < 0.0f), nz = __ballot(active && r.iz < 0.0f);
        if ((nx == 0 || nx == am) && (ny == 0 || ny == am) && (nz == 0 || nz == am)) {
            switch ((nx ? 1u : 0u) | (ny ? 2u : 0u) | (nz ? 4u : 0u)) {
                case 0: trace_packet_impl<1, 0>(sc, r, active, st, hit); return;
                case 1: trace_packet_impl<1, 1>(sc, r, active, st, hit); return;
                case 2: trace_packet_impl<1, 2>(sc, r, active, st, hit); return;
                case 3: trace_packet_impl<1, 3>(sc, r, active, st, hit); return;
                case 4: trace_packet_impl<1, 4>(sc, r, active, st, hit); return;
                case 5: trace_packet_impl<1, 5>(sc, r, active, st, hit); return;
                case 6: trace_packet_impl<1, 6>(sc, r, active, st, hit); return;
                default: trace_packet_impl<1, 7>(sc, r, active, st, hit); return;
            }
        }
    }
    trace_packet_impl<1, -1>(sc, r, active, st, hit);
}

// Object group (mp_scene_group / mp_scene_instances) on the packet walk: member by member, in order, the 64 rays are moved into
// the member's frame (object_ray) and walk the member's own tree as one packet; closest wins with a strict `<`, so the first
// member keeps ties -- the definition trace_objects (8-lane groups) and the oracle's bvh_intersect_impl implement.  A Sphere
// member is intersected lane-parallel.  k is wave-uniform: the member's descriptor comes through scalar loads.
template <class T>
__device__ __forceinline__ const T* uniform_ptr(const T* p) {  // a wave-uniform pointer that the compiler holds in VGPRs -> SGPRs
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v)), hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32));
    return reinterpret_cast<const T*>((static_cast<uint64_t>(hi) << 32) | lo);
}

template <bool OCTANTS, class Stack>
__device__ __forceinline__ void trace_packet_objects(const DevScene& sc, const Ray& r, bool act, Stack& st, PacketHit& h, uint32_t& inst) {
    h.t = FLT_MAX; h.u = h.v = 0.0f; h.prim = kNoPrim;
    inst = 0u;
    for (uint32_t k = 0; k < sc.inst_count; k++) {
        DevScene sk;
        Ray rk;
        object_scene(sc, k, sk);
        object_ray(sc, k, r, rk);
        // the packet walk feeds the scalar unit: what it reads through s_load / pushes with v_writelane must sit in SGPRs
        sk.kind = __builtin_amdgcn_readfirstlane(sk.kind);
        sk.root = __builtin_amdgcn_readfirstlane(sk.root);
        sk.root_lit = __builtin_amdgcn_readfirstlane(sk.root_lit);
        sk.nodes_aos = uniform_ptr(sk.nodes_aos);
        sk.nodes_lit = uniform_ptr(sk.nodes_lit);
        sk.tris_aos = uniform_ptr(sk.tris_aos);
        if (sk.kind == 1u) {  // scene/primitives.rs:16-48 ; prim 0
            float ts, nn[3];
            if (act && sphere_intersect(sk, rk, ts, nn) && ts < h.t) { h.t = ts; h.prim = 0u; h.u = h.v = 0.0f; inst = k; }
            continue;
        }
        const bool go = act && may_hit_scene(sk, rk);
        if (__ballot(go) == 0) continue;
        PacketHit hk;
        trace_packet<OCTANTS>(sk, rk, go, st, hk);
        if (hk.prim != kNoPrim && hk.t < h.t) { h = hk; inst = k; }
    }
}

static_assert(kPlanMaskCacheDwords == kMaskCacheDwords, "launch_plan.h sizes the launches with the device code's constants");

}  // namespace
}  // namespace mp
