// libmp_mask_probe.so: test probes of the packet walk's mask-cache predicates (mask_cache.h) on the GPU
// (tests/test_mask_cache_gpu.py), built with the library's flags.  Each entry point generates its cases on the device from a seed
// and a counter-based hash and checks the predicate that the walk inlines against the walk's own per-ray arithmetic:
//   * tri_may_hit against the per-ray Moeller-Trumbore sequence (triangle.rs:183-217, `1.0f / det`) of 192 rays inside B;
//   * tri_may_hit once more on boxes beyond a triangle's far edges and on exact-boundary rays (tests/test_mask_far_side_gpu.py);
//   * tri_exit1_key / tri_exit2_key (the walk's early-outs of a triangle test, as a wave decides them) against the same per-ray
//     sequence of 64 rays inside B (tests/test_tri_exits_gpu.py);
//   * bounds_may_hit<OCT> against slab<false, OCT> (aabb.rs:254-284, limit FLT_MAX) of 192 rays inside B, all eight patterns;
//   * mask_cache_ray_ok against its plain definition, every f32 bit pattern in each of the nine components;
//   * bounds_deviation against `v < lo || v > hi`;
//   * mask_cache_begin_pass against a serial restatement of its rule, over sequences of passes per wave;
//   * mask_cache_begin_unit's header for given cameras and pixel blocks, handed back for the host model of the test;
//   * mask_cache_pass_inside's decision on passes the test makes by hand, handed back likewise (tests/test_pass_entry_gpu.py).
// The 192 rays of a case are the 64 corners of its 6-D box (origin x direction or origin x inverse direction), those corners moved
// one ulp inward in every coordinate, and 64 interior points (one in four snapped onto a face); one wave per case, lane l owns rays
// l, 64 + l and 128 + l.  Counters (unsigned long long out[8]): [0] violations, [1] cases, [2] smallest violating case index (~0 if
// none), [3] cases some ray hits / passes, [4] cases the predicate rejects, [5] edge-only cases (hit by a corner or inward ray and
// by no interior ray), [6] begin_pass: calls that rewrote B.  Kernels write nothing but these counters and the dump buffer.  The
// return value is 0 or the HIP error code of the first call that failed.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "mask_cache.h"

namespace {

using namespace mp::mc;

constexpr int kCounters = 8;
constexpr float kOrgCap = 2.0f * kCoordCap;  // |B's origin bounds| <= 2^31 (mask_cache_begin_pass)

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
// draw k of case c
__device__ __forceinline__ uint64_t hsh(uint64_t seed, uint64_t c, uint32_t k) { return mix64(seed ^ mix64(c * 0x10000ull + k)); }
__device__ __forceinline__ float unit(uint64_t h) { return static_cast<float>(static_cast<uint32_t>(h >> 40)) * 0x1p-24f; }  // [0, 1)

// One wave's outcome, by lane 0 (every lane passes the same wave-uniform values)
__device__ __forceinline__ void record_case(unsigned long long* out, bool bad, uint64_t idx, bool hit, bool rejected, bool edge_only) {
    if ((threadIdx.x & 63) != 0) return;
    atomicAdd(out + 1, 1ull);
    if (bad) { atomicAdd(out + 0, 1ull); atomicMin(out + 2, static_cast<unsigned long long>(idx)); }
    if (hit) atomicAdd(out + 3, 1ull);
    if (rejected) atomicAdd(out + 4, 1ull);
    if (edge_only) atomicAdd(out + 5, 1ull);
}

// a float with a random mantissa and sign and a biased exponent in [elo, ehi]; one draw in four at an end of the range, one in eight
// with an extreme mantissa (probe.hip)
__device__ __forceinline__ float pick(uint64_t h, uint32_t elo, uint32_t ehi) {
    const uint32_t sel = static_cast<uint32_t>(h >> 56);
    uint32_t e = elo + static_cast<uint32_t>((h >> 32) & 0xFFFFu) % (ehi - elo + 1u);
    if ((sel & 3u) == 0u) e = (sel & 4u) ? ehi : elo;
    uint32_t m = static_cast<uint32_t>(h) & 0x7FFFFFu;
    if ((sel & 0x38u) == 0u) m = (sel & 0x40u) ? 0x7FFFFFu : 0u;
    return as_f(((sel & 0x80u) << 24) | (e << 23) | m);
}
__device__ __forceinline__ float pick_pos(uint64_t h, uint32_t elo, uint32_t ehi) { return fabsf(pick(h, elo, ehi)); }
// the neighbour of a finite x towards +inf (up) or -inf
__device__ __forceinline__ float step(float x, bool up) {
    if (x == 0.0f) return up ? 0x1p-149f : -0x1p-149f;
    return as_f(as_u(x) + (((x > 0.0f) == up) ? 1u : 0xFFFFFFFFu));
}
__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
__device__ __forceinline__ float lerp_in(float lo, float hi, float t) { return clampf(lo + (hi - lo) * t, lo, hi); }

// ray j (0..191) of a case whose 6-D box is lo[6], hi[6]: corner, corner one ulp inward, interior (one in four on a face)
__device__ __forceinline__ void case_ray(const float (&lo)[6], const float (&hi)[6], uint32_t j, uint64_t seed, uint64_t c, float (&x)[6]) {
    const uint64_t hs = hsh(seed, c, 1000u + j);
    const uint32_t face = static_cast<uint32_t>(hs >> 8) % 6u;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const bool up = ((j >> k) & 1u) != 0u;
        if (j < 128u) {
            x[k] = up ? hi[k] : lo[k];
            if (j >= 64u && lo[k] < hi[k]) x[k] = up ? step(hi[k], false) : step(lo[k], true);
        } else {
            x[k] = lerp_in(lo[k], hi[k], unit(hsh(seed, c, 2000u + j * 8u + k)));
            if ((hs & 3u) == 0u && face == static_cast<uint32_t>(k)) x[k] = (hs & 4u) ? hi[k] : lo[k];
        }
    }
}

// B's origin bounds: within +-2^31; one case in sixteen a point box, one axis in eight of zero or one-ulp width
__device__ __forceinline__ void gen_origin_bounds(uint64_t seed, uint64_t c, float (&lo)[3], float (&hi)[3]) {
    const bool point = (hsh(seed, c, 10) & 15u) == 0u;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint64_t h = hsh(seed, c, 11 + k), h2 = hsh(seed, c, 14 + k);
        const float ctr = (h & 0x700u) == 0u ? 0.0f : pick(h, 127 - 20, 127 + 30);
        const uint32_t wk = static_cast<uint32_t>(h2 >> 60);
        const float w = (point || wk == 0u) ? 0.0f : pick_pos(h2, 127 - 30, 127 + 30);
        lo[k] = clampf(ctr - w, -kOrgCap, kOrgCap);
        hi[k] = clampf(ctr + w, -kOrgCap, kOrgCap);
        if (!point && wk == 1u) hi[k] = step(lo[k], true);
    }
}

// ---- (a) tri_may_hit ------------------------------------------------------------------------------------------------------------
struct TriRay {
    float t, u, v;
    bool hit;
};
// triangle.rs:183-217 for one ray, with the walk's fms / fma_dot and a plain 1 / det; hit = u >= 0, v >= 0, u + v <= 1, t >= 0
__device__ __forceinline__ TriRay mt_ray(const float (&x)[6], const float (&v0)[3], const float (&e1)[3], const float (&e2)[3]) {
    const float dx = x[3], dy = x[4], dz = x[5];
    const float hx = fms(dy, e2[2], dz * e2[1]), hy = fms(dz, e2[0], dx * e2[2]), hz = fms(dx, e2[1], dy * e2[0]);
    const float det = fma_dot(e1[0], e1[1], e1[2], hx, hy, hz);
    const float inv_det = 1.0f / det;
    const float sx = x[0] - v0[0], sy = x[1] - v0[1], sz = x[2] - v0[2];
    const float u = inv_det * fma_dot(sx, sy, sz, hx, hy, hz);
    const float qx = fms(sy, e1[2], sz * e1[1]), qy = fms(sz, e1[0], sx * e1[2]), qz = fms(sx, e1[1], sy * e1[0]);
    const float v = inv_det * fma_dot(dx, dy, dz, qx, qy, qz);
    const float t = inv_det * fma_dot(e2[0], e2[1], e2[2], qx, qy, qz);
    return TriRay{t, u, v, u >= 0.0f && v >= 0.0f && (u + v) <= 1.0f && t >= 0.0f};
}

__device__ __forceinline__ void clamp_vertex(float (&p)[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = clampf(p[k], -kCoordCap, kCoordCap);
}

// One triangle case: B (header layout: origin bounds 0..5, direction bounds 13..18) and vertices within 2^30.
__device__ __forceinline__ void gen_tri_case(uint64_t seed, uint64_t c, float (&b)[20], float (&v0)[3], float (&v1)[3], float (&v2)[3]) {
    float olo[3], ohi[3];
    gen_origin_bounds(seed, c, olo, ohi);
    const bool tiny = (hsh(seed, c, 20) & 7u) == 0u;  // directions of 2^-60 .. 2^-20: determinants near the rcp_short window's low end
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint64_t h = hsh(seed, c, 21 + k), h2 = hsh(seed, c, 24 + k);
        const float ctr = tiny ? pick(h, 127 - 60, 127 - 20) : pick(h, 127 - 40, 127 + 1);
        const float w = (h2 & 7u) == 0u ? 0.0f : pick_pos(h2, tiny ? 127 - 70 : 127 - 40, tiny ? 127 - 20 : 127 + 1);
        b[k] = olo[k]; b[3 + k] = ohi[k];
        b[13 + k] = clampf(ctr - w, -2.0f, 2.0f);
        b[16 + k] = clampf(ctr + w, -2.0f, 2.0f);
    }
    for (int i = 6; i < 13; i++) b[i] = 0.0f;
    b[19] = 0.0f;
    float lo[6], hi[6];
#pragma unroll
    for (int k = 0; k < 3; k++) { lo[k] = b[k]; hi[k] = b[3 + k]; lo[3 + k] = b[13 + k]; hi[3 + k] = b[16 + k]; }

    const uint64_t hm = hsh(seed, c, 30);
    const uint32_t mode = static_cast<uint32_t>(hm & 7u);
    // an aimed point p = o + t d on a ray of B (a corner or inward ray three times in four)
    float x[6];
    const uint32_t j = (hm & 0x300u) ? static_cast<uint32_t>(hm >> 10) & 127u : 128u + (static_cast<uint32_t>(hm >> 10) & 63u);
    case_ray(lo, hi, j, seed, c, x);
    const uint64_t ht = hsh(seed, c, 31);
    const uint32_t tk = static_cast<uint32_t>(ht & 3u);
    const float t = tk == 0u ? 0.0f : tk == 1u ? as_f((127u - 1u - static_cast<uint32_t>(ht >> 8) % 40u) << 23)
                  : tk == 2u ? pick_pos(ht, 127 - 4, 127 + 10) : pick_pos(ht, 127 + 15, 127 + 31);
    float p[3] = {x[0] + t * x[3], x[1] + t * x[4], x[2] + t * x[5]};
    clamp_vertex(p);
    // edges of scale 2^-30 .. 2^31
    float E1[3], E2[3];
    const uint64_t he = hsh(seed, c, 32);
    const float s1 = as_f((127u - 30u + static_cast<uint32_t>(he & 63u) % 62u) << 23), s2 = as_f((127u - 30u + static_cast<uint32_t>((he >> 8) & 63u) % 62u) << 23);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        E1[k] = s1 * (2.0f * unit(hsh(seed, c, 33 + k)) - 1.0f);
        E2[k] = (he & 0x10000u) ? s1 * (2.0f * unit(hsh(seed, c, 36 + k)) - 1.0f) : s2 * (2.0f * unit(hsh(seed, c, 36 + k)) - 1.0f);
    }
    if (mode <= 2u || mode == 5u) {  // aimed (0, 1, 5) and near-miss (2): p on a vertex, on an edge or inside
        const uint32_t place = static_cast<uint32_t>(hm >> 20) % 3u;
        const float a = unit(hsh(seed, c, 40)), bb = unit(hsh(seed, c, 41)) * (1.0f - a);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            v0[k] = place == 0u ? p[k] : place == 1u ? p[k] - a * E1[k] : p[k] - a * E1[k] - bb * E2[k];
            v1[k] = v0[k] + E1[k];
            v2[k] = v0[k] + E2[k];
        }
        if (mode == 2u) {  // a few ulps off, one vertex or all three
            const uint64_t hn = hsh(seed, c, 42);
            const uint32_t n = 1u + static_cast<uint32_t>(hn & 3u), kk = static_cast<uint32_t>(hn >> 8) % 3u, which = static_cast<uint32_t>(hn >> 16) & 3u;
            const bool up = (hn >> 24) & 1u;
            for (uint32_t i = 0; i < n; i++) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    if (static_cast<uint32_t>(k) != kk) continue;
                    if (which == 0u || which == 3u) v0[k] = step(v0[k], up);
                    if (which == 1u || which == 3u) v1[k] = step(v1[k], up);
                    if (which == 2u || which == 3u) v2[k] = step(v2[k], up);
                }
            }
        }
    } else if (mode == 3u) {  // degenerate: axis-aligned collinear (det = 0 exactly), a zero edge, e1 = e2, or nearly collinear
        const uint32_t sub = static_cast<uint32_t>(hm >> 20) & 3u, ax = static_cast<uint32_t>(hm >> 24) % 3u;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            v0[k] = p[k];
            if (sub == 0u) { v1[k] = k == static_cast<int>(ax) ? p[k] + E1[k] : p[k]; v2[k] = k == static_cast<int>(ax) ? p[k] - E2[k] : p[k]; }
            else if (sub == 1u) { v1[k] = p[k]; v2[k] = p[k] + E2[k]; }
            else if (sub == 2u) { v1[k] = p[k] + E1[k]; v2[k] = v1[k]; }
            else { v1[k] = p[k] + E1[k]; v2[k] = p[k] + 2.0f * E1[k]; }
        }
    } else if (mode == 4u) {  // planar: in the plane of one of B's origin faces (s = 0 exactly for the corners on it)
        const uint32_t ax = static_cast<uint32_t>(hm >> 20) % 3u;
        const float f = clampf((hm >> 24) & 1u ? b[3 + ax] : b[ax], -kCoordCap, kCoordCap);
        const float a = unit(hsh(seed, c, 40)), bb = unit(hsh(seed, c, 41)) * (1.0f - a);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            v0[k] = p[k] - a * E1[k] - bb * E2[k];
            v1[k] = v0[k] + E1[k];
            v2[k] = v0[k] + E2[k];
            if (k == static_cast<int>(ax)) v0[k] = v1[k] = v2[k] = f;
        }
    } else {  // random vertices around B
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float ctr = 0.5f * b[k] + 0.5f * b[3 + k];
            v0[k] = ctr + pick(hsh(seed, c, 50 + k), 127 - 30, 127 + 30);
            v1[k] = ctr + pick(hsh(seed, c, 53 + k), 127 - 30, 127 + 30);
            v2[k] = ctr + pick(hsh(seed, c, 56 + k), 127 - 30, 127 + 30);
        }
    }
    clamp_vertex(v0); clamp_vertex(v1); clamp_vertex(v2);
}

// dump record of one case: kDumpHead dwords (inputs and verdict), then 192 rays of kDumpRay dwords
constexpr int kDumpHead = 40, kDumpRay = 10, kRays = 192;
constexpr int kDumpCase = kDumpHead + kRays * kDumpRay;

__global__ void tri_kernel(uint64_t seed, uint64_t base, uint64_t ncases, unsigned long long* out, uint32_t* dump) {
    const uint64_t c = base + (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / 64u;
    const uint32_t lane = threadIdx.x & 63u;
    if (c >= ncases) return;  // (whole waves)
    float b[20], v0[3], v1[3], v2[3];
    gen_tri_case(seed, c, b, v0, v1, v2);
    const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    float lo[6], hi[6];
#pragma unroll
    for (int k = 0; k < 3; k++) { lo[k] = b[k]; hi[k] = b[3 + k]; lo[3 + k] = b[13 + k]; hi[3 + k] = b[16 + k]; }
    const bool keep = tri_may_hit(b, v0, e1, e2);
    bool edge = false, inner = false;
    uint32_t* rec = dump ? dump + c * kDumpCase : nullptr;
    for (uint32_t s = 0; s < 3; s++) {
        const uint32_t j = s * 64u + lane;
        float x[6];
        case_ray(lo, hi, j, seed, c, x);
        const TriRay tr = mt_ray(x, v0, e1, e2);
        if (s < 2) edge |= tr.hit; else inner |= tr.hit;
        if (rec) {
            uint32_t* rr = rec + kDumpHead + j * kDumpRay;
            for (int k = 0; k < 6; k++) rr[k] = as_u(x[k]);
            rr[6] = as_u(tr.t); rr[7] = as_u(tr.u); rr[8] = as_u(tr.v); rr[9] = tr.hit ? 1u : 0u;
        }
    }
    const bool any_edge = __ballot(edge) != 0, any_inner = __ballot(inner) != 0, any = any_edge || any_inner;
    if (rec && lane < 20u) rec[lane] = as_u(b[lane]);
    if (rec && lane == 20u) {
        for (int k = 0; k < 3; k++) { rec[20 + k] = as_u(v0[k]); rec[23 + k] = as_u(v1[k]); rec[26 + k] = as_u(v2[k]); }
        for (int k = 0; k < 3; k++) { rec[29 + k] = as_u(e1[k]); rec[32 + k] = as_u(e2[k]); }
        rec[35] = keep ? 1u : 0u;
    }
    record_case(out, !keep && any, c, any, !keep, any_edge && !any_inner);
}

// ---- (a') the early-outs of a triangle test: tri_exit1_key / tri_exit2_key --------------------------------------------------------
// One wave per case of gen_tri_case: 64 rays inside its box (corners, inward corners or interior points, by the case index), a
// random set of them live (one case in eight: all).  The wave-level decision of the walk -- leave the triangle at stage 1 or 2 when
// every lane's key is <= its threshold (-2^-40 live, +inf disabled) -- against the plain per-ray sequence (mt_ray, `1.0f / det`) of
// the live rays.  Counters: [0] cases the wave leaves although a live ray hits, [3] cases some live ray hits, [4] cases left at
// stage 1, [5] cases left at stage 2 only, [6] cases left that the near side alone (a numerator surely negative) would not leave.
__global__ void exit_kernel(uint64_t seed, uint64_t base, uint64_t ncases, unsigned long long* out, uint32_t*) {
    const uint64_t c = base + (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / 64u;
    const uint32_t lane = threadIdx.x & 63u;
    if (c >= ncases) return;  // (whole waves)
    float b[20], v0[3], v1[3], v2[3];
    gen_tri_case(seed, c, b, v0, v1, v2);
    const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    float lo[6], hi[6];
#pragma unroll
    for (int k = 0; k < 3; k++) { lo[k] = b[k]; hi[k] = b[3 + k]; lo[3 + k] = b[13 + k]; hi[3 + k] = b[16 + k]; }
    float x[6];
    case_ray(lo, hi, static_cast<uint32_t>(c % 3u) * 64u + lane, seed, c, x);
    const uint64_t hl = hsh(seed, c, 90);
    const uint64_t live_mask = (hl & 7u) == 0u ? ~0ull : (hsh(seed, c, 91) | (1ull << (hl >> 58)));
    const bool live = ((live_mask >> lane) & 1u) != 0u;
    // the walk's sequence up to the division (packet_walk.h, trace_packet_cached)
    const float dx = x[3], dy = x[4], dz = x[5];
    const float hx = fms(dy, e2[2], dz * e2[1]), hy = fms(dz, e2[0], dx * e2[2]), hz = fms(dx, e2[1], dy * e2[0]);
    const float det = fma_dot(e1[0], e1[1], e1[2], hx, hy, hz);
    const float sx = x[0] - v0[0], sy = x[1] - v0[1], sz = x[2] - v0[2];
    const float un = fma_dot(sx, sy, sz, hx, hy, hz);
    const float thr = live ? -kExitTiny : INFINITY;
    const float xu = tri_flipped(det, un);
    const bool exit1 = __ballot(!(tri_exit1_key(det, xu) <= thr)) == 0;
    const float qx = fms(sy, e1[2], sz * e1[1]), qy = fms(sz, e1[0], sx * e1[2]), qz = fms(sx, e1[1], sy * e1[0]);
    const float vn = fma_dot(dx, dy, dz, qx, qy, qz);
    const float tn = fma_dot(e2[0], e2[1], e2[2], qx, qy, qz);
    const float xv = tri_flipped(det, vn), xt = tri_flipped(det, tn);
    const bool exit2 = __ballot(!(tri_exit2_key(det, xu, xv, xt) <= thr)) == 0;
    const bool near1 = __ballot(!(xu <= thr)) == 0, near2 = __ballot(!(fminf(fminf(xu, xv), xt) <= thr)) == 0;
    const TriRay tr = mt_ray(x, v0, e1, e2);
    const bool any = __ballot(live && tr.hit) != 0;
    const bool left = exit1 || exit2;
    record_case(out, left && any, c, any, exit1, exit2 && !exit1);
    if (lane == 0u && left && !(near1 || near2)) atomicAdd(out + 6, 1ull);
}

// ---- (a'') tri_may_hit beyond the far edges ----------------------------------------------------------------------------------------
// Cases the generator above rarely gives: boxes whose rays all pass the triangle's plane beyond the edge u = 1 (or v = 1) while the
// other coordinate's interval straddles zero, so that only the far-side terms of tri_may_hit (u.lo > 1, v.lo > 1) can reject; and
// exact-boundary cases, where one corner ray of the box computes u == 1 & v == 0, u == 0 & v == 1 or u + v == 1 exactly, is
// accepted, and the strict comparisons must keep the triangle.  Both are built in a local frame -- the triangle {p0, p0 + (sx, 0, 0),
// p0 + (0, sy, 0)} (plus a small tilt in the first family), rays going down -z from a height H -- and then moved to world axes by a
// permutation and sign flips of the axes (a mirror image has the same hits).
//   far family (5 cases in 8): the footprint [a0, a1] x [b0, b1] of the box in (u, v), a0 > 1, b1 >= 0 and b0 around 1 - a0, comes
//     from the origin bounds (directions nearly parallel) or from the direction bounds (origins nearly a point); u and v swapped
//     in half the cases.
//   exact family: every coordinate a small integer multiple of a power of two q, sx and sy powers of two, direction (+-0, +-0, -1):
//     un, vn, det and the quotients are exact.  The aimed point is v1, v2, a dyadic point of the edge v1 v2, or such a point moved one
//     ulp inside or outside; each coordinate of the box is that ray's value alone or extends from it to one side, upwards (away from
//     the triangle in x and y) more often than not, so the ray is a corner of the box; one case in eight lets the direction
//     bounds reach into the triangle's plane (the determinant interval touches zero), one in eight has a vertex at the cap 2^30.
// Counters: [0] violations, [1] cases, [2] first violating case, [3] cases some ray hits, [4] cases rejected, [5] cases that only the
// far-side terms reject, [6] cases kept in which a ray with u == 1, v == 1 or u + v == 1 exactly is accepted.
__device__ __forceinline__ void gen_far_case(uint64_t seed, uint64_t c, float (&b)[20], float (&v0)[3], float (&v1)[3], float (&v2)[3]) {
    float llo[6], lhi[6], p0[3], p1[3], p2[3];  // local frame: ray box (origin, direction) and vertices
    const uint64_t hm = hsh(seed, c, 100);
    if ((hm & 7u) < 5u) {
        const float S = as_f((127u - 8u + static_cast<uint32_t>(hm >> 8) % 29u) << 23);
        const float sx = S * (0.5f + unit(hsh(seed, c, 101))), sy = S * (0.5f + unit(hsh(seed, c, 102)));
        const float tilt = (hm & 0x300000u) == 0u ? 0.0f : 0.05f * S;
        for (int k = 0; k < 3; k++) p0[k] = 4.0f * S * (2.0f * unit(hsh(seed, c, 103 + k)) - 1.0f);
        const float E1[3] = {sx, tilt * (2.0f * unit(hsh(seed, c, 106)) - 1.0f), tilt * (2.0f * unit(hsh(seed, c, 107)) - 1.0f)};
        const float E2[3] = {tilt * (2.0f * unit(hsh(seed, c, 108)) - 1.0f), sy, tilt * (2.0f * unit(hsh(seed, c, 109)) - 1.0f)};
        for (int k = 0; k < 3; k++) { p1[k] = p0[k] + E1[k]; p2[k] = p0[k] + E2[k]; }
        // the footprint in (u, v)
        const uint64_t hf = hsh(seed, c, 110);
        float a0 = 1.0f + as_f((127u - static_cast<uint32_t>(hf & 15u)) << 23) * (0.25f + unit(hsh(seed, c, 111)));  // 1 + 2^-15 .. 1 + 1.25
        float a1 = a0 + 2.0f * unit(hsh(seed, c, 112)) * unit(hsh(seed, c, 113));
        float b0 = 1.0f - a0 - (2.0f * unit(hsh(seed, c, 114)) - 0.5f);  // around 1 - a0, mostly below
        float b1 = fmaxf(b0, (hf & 0x30u) == 0u ? -0.25f * unit(hsh(seed, c, 115)) : 0.5f * unit(hsh(seed, c, 115)));
        if (hf & 0x100u) { float x = a0; a0 = b0; b0 = x; x = a1; a1 = b1; b1 = x; }  // v beyond its far edge instead
        const float H = S * as_f((127u + 2u + static_cast<uint32_t>(hf >> 12) % 5u) << 23);
        const float am = 0.5f * (a0 + a1), bm = 0.5f * (b0 + b1);
        const float wz = (hf & 0x10000u) ? 0.0f : H * 0x1p-6f * unit(hsh(seed, c, 116));
        const float wd = (hf & 0x60000u) == 0u ? 0.0f : as_f((127u - 10u - static_cast<uint32_t>(hf >> 20) % 12u) << 23);
        if (hf & 0x200u) {  // by the origin bounds
            llo[0] = p0[0] + a0 * sx; lhi[0] = p0[0] + a1 * sx;
            llo[1] = p0[1] + b0 * sy; lhi[1] = p0[1] + b1 * sy;
            llo[3] = -wd; lhi[3] = wd; llo[4] = -wd; lhi[4] = wd;
        } else {  // by the direction bounds
            const float wo = (hf & 0x400u) ? 0.0f : S * 0x1p-8f * unit(hsh(seed, c, 117));
            llo[0] = p0[0] + am * sx - wo; lhi[0] = p0[0] + am * sx + wo;
            llo[1] = p0[1] + bm * sy - wo; lhi[1] = p0[1] + bm * sy + wo;
            llo[3] = (a0 - am) * sx / H; lhi[3] = (a1 - am) * sx / H;
            llo[4] = (b0 - bm) * sy / H; lhi[4] = (b1 - bm) * sy / H;
        }
        llo[2] = p0[2] + H; lhi[2] = p0[2] + H + wz;
        llo[5] = -1.0f; lhi[5] = -1.0f + wd;
    } else {
        const bool cap = ((hm >> 8) & 7u) == 0u, plane = ((hm >> 11) & 7u) == 0u;
        const float q = cap ? 0x1p20f : as_f((127u - 20u + static_cast<uint32_t>(hm >> 16) % 36u) << 23);
        const float sx = q * as_f((127u + 4u + static_cast<uint32_t>(hm >> 24) % 5u) << 23), sy = q * as_f((127u + 4u + static_cast<uint32_t>(hm >> 28) % 5u) << 23);
        for (int k = 0; k < 3; k++) p0[k] = q * (static_cast<float>(static_cast<uint32_t>(hsh(seed, c, 120 + k) >> 40) % 1025u) - 512.0f);
        if (cap) { p0[0] = 0x1p30f - sx; p0[1] = -0x1p30f; }  // v1.x at the cap, v0.y and v1.y at its negative
        for (int k = 0; k < 3; k++) { p1[k] = p0[k]; p2[k] = p0[k]; }
        p1[0] = p0[0] + sx; p2[1] = p0[1] + sy;
        // the aimed point (a, 1 - a) of the edge v1 v2: a = 1 (v1), 0 (v2) or k / 16
        const uint64_t hp = hsh(seed, c, 123);
        const uint32_t place = static_cast<uint32_t>(hp & 7u);  // 0, 1: v1; 2, 3: v2; 4: on the edge; 5: inside by an ulp; 6: outside by an ulp; 7: on the edge
        const float a = place < 2u ? 1.0f : place < 4u ? 0.0f : static_cast<float>(1u + static_cast<uint32_t>(hp >> 8) % 15u) * 0.0625f;
        float x[6] = {p0[0] + a * sx, p0[1] + (1.0f - a) * sy, p0[2] + q * static_cast<float>(1u + static_cast<uint32_t>(hp >> 16) % 4096u),
                      (hp & 0x10000000u) ? -0.0f : 0.0f, (hp & 0x20000000u) ? -0.0f : 0.0f, -1.0f};
        const bool along_x = (hp >> 30) & 1u;  // the coordinate the hair moves: towards the triangle is down in x and in y
        if (place == 5u) x[along_x ? 0 : 1] = step(x[along_x ? 0 : 1], false);
        if (place == 6u) x[along_x ? 0 : 1] = step(x[along_x ? 0 : 1], true);
        for (int k = 0; k < 6; k++) {
            const uint64_t hk = hsh(seed, c, 130 + k);
            const uint32_t side = static_cast<uint32_t>(hk & 7u);  // 0..2: the value alone; 3..5: upwards; 6, 7: downwards
            const float w = k < 3 ? q * as_f((127u - 2u + static_cast<uint32_t>(hk >> 8) % 12u) << 23) : as_f((127u - 20u + static_cast<uint32_t>(hk >> 8) % 18u) << 23);
            llo[k] = side >= 6u ? x[k] - w : x[k];
            lhi[k] = (side >= 3u && side < 6u) ? x[k] + w : x[k];
        }
        if (plane) { llo[5] = -1.0f; lhi[5] = 0.0f; }
    }
    // to world axes: world[k] = sg[k] * local[pm[k]]
    const uint64_t hw = hsh(seed, c, 140);
    const uint32_t rot = static_cast<uint32_t>(hw & 0xFFu) % 6u;
    const int pm[3] = {static_cast<int>(rot % 3u), static_cast<int>((rot % 3u + 1u + rot / 3u) % 3u), static_cast<int>((rot % 3u + 2u - rot / 3u) % 3u)};
    float lo[6], hi[6];
    for (int k = 0; k < 3; k++) {
        const float sg = ((hw >> (8 + k)) & 1u) ? -1.0f : 1.0f;
        v0[k] = sg * p0[pm[k]]; v1[k] = sg * p1[pm[k]]; v2[k] = sg * p2[pm[k]];
        for (int g = 0; g < 2; g++) {
            const float e0 = sg * llo[3 * g + pm[k]], e1 = sg * lhi[3 * g + pm[k]];
            lo[3 * g + k] = sg < 0.0f ? e1 : e0;
            hi[3 * g + k] = sg < 0.0f ? e0 : e1;
        }
    }
    clamp_vertex(v0); clamp_vertex(v1); clamp_vertex(v2);
    for (int k = 0; k < 3; k++) {
        b[k] = clampf(lo[k], -kOrgCap, kOrgCap); b[3 + k] = clampf(hi[k], -kOrgCap, kOrgCap);
        b[13 + k] = clampf(lo[3 + k], -2.0f, 2.0f); b[16 + k] = clampf(hi[3 + k], -2.0f, 2.0f);
    }
    for (int i = 6; i < 13; i++) b[i] = 0.0f;
    b[19] = 0.0f;
}

__global__ void far_kernel(uint64_t seed, uint64_t base, uint64_t ncases, unsigned long long* out, uint32_t*) {
    const uint64_t c = base + (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / 64u;
    const uint32_t lane = threadIdx.x & 63u;
    if (c >= ncases) return;  // (whole waves)
    float b[20], v0[3], v1[3], v2[3];
    gen_far_case(seed, c, b, v0, v1, v2);
    const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    float lo[6], hi[6];
#pragma unroll
    for (int k = 0; k < 3; k++) { lo[k] = b[k]; hi[k] = b[3 + k]; lo[3 + k] = b[13 + k]; hi[3 + k] = b[16 + k]; }
    bool far_only = false;
    const bool keep = tri_may_hit(b, v0, e1, e2, &far_only);
    bool hit = false, on_edge = false;
    for (uint32_t s = 0; s < 3; s++) {
        float x[6];
        case_ray(lo, hi, s * 64u + lane, seed, c, x);
        const TriRay tr = mt_ray(x, v0, e1, e2);
        hit |= tr.hit;
        on_edge |= tr.hit && (tr.u == 1.0f || tr.v == 1.0f || (tr.u + tr.v) == 1.0f);
    }
    const bool any = __ballot(hit) != 0, any_edge = __ballot(on_edge) != 0;
    record_case(out, !keep && any, c, any, !keep, far_only);
    if (lane == 0u && keep && any_edge) atomicAdd(out + 6, 1ull);
}

// ---- (b) bounds_may_hit<OCT> -------------------------------------------------------------------------------------------------------
// B's inverse-direction bounds: finite, non-zero, of the pattern's sign, magnitudes up to FLT_MAX
__device__ __forceinline__ void gen_box_case(uint64_t seed, uint64_t c, uint32_t oct, float (&b)[20], float (&bmn)[3], float (&bmx)[3]) {
    float olo[3], ohi[3];
    gen_origin_bounds(seed, c, olo, ohi);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint64_t h = hsh(seed, c, 60 + k), h2 = hsh(seed, c, 63 + k);
        const bool wide = (h & 0x300u) == 0u;
        float m1 = wide ? pick_pos(h, 1, 254) : pick_pos(h, 127 - 2, 127 + 12);
        float m2 = (h2 & 7u) == 0u ? m1 : wide ? pick_pos(h2, 1, 254) : pick_pos(h2, 127 - 2, 127 + 12);
        if ((h2 & 0x7F00u) == 0u) m2 = FLT_MAX;
        const float mlo = fminf(m1, m2), mhi = fmaxf(m1, m2);
        const bool neg = ((oct >> k) & 1u) != 0u;
        b[k] = olo[k]; b[3 + k] = ohi[k];
        b[6 + k] = neg ? -mhi : mlo;
        b[9 + k] = neg ? -mlo : mhi;
    }
    b[12] = as_f(oct | 0x100u);
    for (int i = 13; i < 20; i++) b[i] = 0.0f;
    float lo[6], hi[6];
#pragma unroll
    for (int k = 0; k < 3; k++) { lo[k] = b[k]; hi[k] = b[3 + k]; lo[3 + k] = b[6 + k]; hi[3 + k] = b[9 + k]; }
    const uint64_t hm = hsh(seed, c, 70);
    const uint32_t mode = static_cast<uint32_t>(hm & 7u);
    float x[6];
    const uint32_t j = (hm & 0x300u) ? static_cast<uint32_t>(hm >> 10) & 127u : 128u + (static_cast<uint32_t>(hm >> 10) & 63u);
    case_ray(lo, hi, j, seed, c, x);
    const float d[3] = {1.0f / x[3], 1.0f / x[4], 1.0f / x[5]};
    const uint64_t ht = hsh(seed, c, 71);
    const float t = mode == 2u ? -pick_pos(ht, 127 - 10, 127 + 30) : (ht & 3u) == 0u ? 0.0f : pick_pos(ht, 127 - 30, 127 + 30);
    float half[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float p = x[k] + t * d[k];
        half[k] = pick_pos(hsh(seed, c, 72 + k), 127 - 30, 127 + 31);
        bmn[k] = p - half[k];
        bmx[k] = p + half[k];
    }
    if (mode == 0u) {  // flat in 1-3 axes
        const uint32_t m = 1u + static_cast<uint32_t>(hm >> 20) % 7u;
#pragma unroll
        for (int k = 0; k < 3; k++) if ((m >> k) & 1u) bmx[k] = bmn[k] = (hm >> (24 + k)) & 1u ? x[k] + t * d[k] : bmn[k];
    } else if (mode == 1u) {  // faces on B's origin faces
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint32_t f = static_cast<uint32_t>(hm >> (20 + 3 * k)) & 7u;
            if (f == 1u) bmn[k] = b[k]; else if (f == 2u) bmn[k] = b[3 + k]; else if (f == 3u) bmx[k] = b[k]; else if (f == 4u) bmx[k] = b[3 + k];
            else if (f == 5u) { bmn[k] = b[k]; bmx[k] = b[3 + k]; }
            if (bmn[k] > bmx[k]) { const float s = bmn[k]; bmn[k] = bmx[k]; bmx[k] = s; }
        }
    } else if (mode == 3u) {  // entered at t = 0: the box holds the ray's origin, on a face one time in two
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint32_t f = static_cast<uint32_t>(hm >> (20 + 2 * k)) & 3u;
            bmn[k] = f == 1u ? x[k] : x[k] - half[k];
            bmx[k] = f == 2u ? x[k] : x[k] + half[k];
        }
    } else if (mode == 4u) {  // grazing: entry through axis a and exit through axis e at the same f32 distance for ray j
        const uint32_t a = static_cast<uint32_t>(hm >> 20) % 3u, e = (a + 1u + (static_cast<uint32_t>(hm >> 24) & 1u)) % 3u, o3 = 3u - a - e;
        const float T = pick_pos(ht, 127 - 20, 127 + 20), big = 0x1p40f;
        float xa = x[a] + T * d[a];
        const float Ta = (xa - x[a]) * x[3 + a];
        float ye = x[e] + Ta * d[e];
        for (int i = -4; i <= 4; i++) {  // the exit face that gives the same product, if one of the neighbours does
            float y = ye;
            for (int s = 0; s < (i < 0 ? -i : i); s++) y = step(y, i > 0);
            if ((y - x[e]) * x[3 + e] == Ta) { ye = y; break; }
        }
        const bool na = x[3 + a] < 0.0f, ne = x[3 + e] < 0.0f;
        bmn[a] = na ? xa - big : xa; bmx[a] = na ? xa : xa + big;
        bmn[e] = ne ? ye : ye - big; bmx[e] = ne ? ye + big : ye;
        bmn[o3] = x[o3] - big; bmx[o3] = x[o3] + big;
    } else if (mode == 5u) {  // faces at +-FLT_MAX: the products overflow to +-inf
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint32_t f = static_cast<uint32_t>(hm >> (20 + 2 * k)) & 3u;
            if (f == 1u) bmn[k] = -FLT_MAX; else if (f == 2u) bmx[k] = FLT_MAX; else if (f == 3u) { bmn[k] = -FLT_MAX; bmx[k] = FLT_MAX; }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {  // finite, min <= max
        bmn[k] = clampf(bmn[k], -FLT_MAX, FLT_MAX); bmx[k] = clampf(bmx[k], -FLT_MAX, FLT_MAX);
        if (!(bmn[k] <= bmx[k])) bmx[k] = bmn[k];
    }
}

template <int OCT>
__device__ __forceinline__ void box_case(uint64_t seed, uint64_t c, unsigned long long* out, uint32_t* dump) {
    const uint32_t lane = threadIdx.x & 63u;
    float b[20], bmn[3], bmx[3];
    gen_box_case(seed, c, OCT, b, bmn, bmx);
    float lo[6], hi[6];
#pragma unroll
    for (int k = 0; k < 3; k++) { lo[k] = b[k]; hi[k] = b[3 + k]; lo[3 + k] = b[6 + k]; hi[3 + k] = b[9 + k]; }
    const bool keep = bounds_may_hit<OCT>(b, bmn, bmx);
    bool edge = false, inner = false;
    uint32_t* rec = dump ? dump + c * kDumpCase : nullptr;
    for (uint32_t s = 0; s < 3; s++) {
        const uint32_t j = s * 64u + lane;
        float x[6];
        case_ray(lo, hi, j, seed, c, x);
        Ray r;
        r.ox = x[0]; r.oy = x[1]; r.oz = x[2]; r.ix = x[3]; r.iy = x[4]; r.iz = x[5];
        r.dx = 1.0f / x[3]; r.dy = 1.0f / x[4]; r.dz = 1.0f / x[5];
        float t1, t2;
        slab<false, OCT>(bmn[0], bmn[1], bmn[2], bmx[0], bmx[1], bmx[2], r, FLT_MAX, t1, t2);
        const bool pass = t1 <= t2;
        if (s < 2) edge |= pass; else inner |= pass;
        if (rec) {
            uint32_t* rr = rec + kDumpHead + j * kDumpRay;
            for (int k = 0; k < 6; k++) rr[k] = as_u(x[k]);
            rr[6] = as_u(t1); rr[7] = as_u(t2); rr[8] = 0u; rr[9] = pass ? 1u : 0u;
        }
    }
    const bool any_edge = __ballot(edge) != 0, any_inner = __ballot(inner) != 0, any = any_edge || any_inner;
    if (rec && lane < 20u) rec[lane] = as_u(b[lane]);
    if (rec && lane == 20u) {
        for (int k = 0; k < 3; k++) { rec[20 + k] = as_u(bmn[k]); rec[23 + k] = as_u(bmx[k]); }
        rec[26] = OCT;
        rec[35] = keep ? 1u : 0u;
    }
    record_case(out, !keep && any, c, any, !keep, any_edge && !any_inner);
}

// case c tests pattern c & 7
__global__ void box_kernel(uint64_t seed, uint64_t base, uint64_t ncases, unsigned long long* out, uint32_t* dump) {
    const uint64_t c = base + (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / 64u;
    if (c >= ncases) return;
    switch (static_cast<int>(c & 7u)) {
        case 0: box_case<0>(seed, c, out, dump); break;
        case 1: box_case<1>(seed, c, out, dump); break;
        case 2: box_case<2>(seed, c, out, dump); break;
        case 3: box_case<3>(seed, c, out, dump); break;
        case 4: box_case<4>(seed, c, out, dump); break;
        case 5: box_case<5>(seed, c, out, dump); break;
        case 6: box_case<6>(seed, c, out, dump); break;
        default: box_case<7>(seed, c, out, dump); break;
    }
}

// ---- (c) pass entry -----------------------------------------------------------------------------------------------------------------
// benign and boundary values for the components not under test (the first 8 pass every cap)
__constant__ uint32_t kOther[32] = {
    0x00000000u, 0x80000000u, 0x3F800000u, 0xBF000000u, 0x00000001u, 0x807FFFFFu, 0x00800000u, 0x3FFFFFFFu,  // +-0, 1, -0.5, denormals, FLT_MIN, 2^-
    0x40000000u, 0xC0000000u, 0x40000001u, 0xC0000001u, 0x4E800000u, 0xCE800000u, 0x4E7FFFFFu, 0x4E800001u,  // +-2, 2^+, +-2^30, 2^30 -+
    0xCE800001u, 0x7F7FFFFFu, 0xFF7FFFFFu, 0x7F800000u, 0xFF800000u, 0x7FC00000u, 0xFFC00000u, 0x7F800001u,  // FLT_MAX, inf, NaNs
    0xFFFFFFFFu, 0x4F000000u, 0x1F800000u, 0x40400000u, 0x3F7FFFFFu, 0xBE800000u, 0x00400000u, 0x7FFFFFFFu};
__device__ __forceinline__ bool ray_ok_plain(const float (&x)[9]) {
    bool ok = true;
    for (int k = 0; k < 3; k++) ok = ok && fabsf(x[k]) <= kCoordCap;      // origin
    for (int k = 3; k < 6; k++) ok = ok && fabsf(x[k]) <= FLT_MAX;        // inverse direction finite
    for (int k = 6; k < 9; k++) ok = ok && fabsf(x[k]) <= 2.0f;           // direction
    return ok;
}
constexpr uint32_t kOkPerThread = 16;
// component `comp` (0..2 origin, 3..5 inverse, 6..8 direction) takes bit patterns base + thread * 16 + i; the others come from kOther,
// a value that passes its own cap three times in four
__global__ void ray_ok_kernel(uint64_t seed, int comp, uint64_t base, unsigned long long* out) {
    const uint64_t tid = base + static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    bool bad = false;
    uint64_t first = ~0ull;
    for (uint32_t i = 0; i < kOkPerThread; i++) {
        const uint64_t idx = tid * kOkPerThread + i;
        const uint64_t h = mix64(seed ^ (idx * 0x9E3779B97F4A7C15ull) ^ static_cast<uint64_t>(comp));
        float x[9];
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const uint32_t sel = static_cast<uint32_t>(h >> (6 * k)) & 63u;
            x[k] = as_f(kOther[(sel & 0x30u) ? (sel & 7u) : (sel & 31u)]);
        }
#pragma unroll
        for (int k = 0; k < 9; k++) if (k == comp) x[k] = as_f(static_cast<uint32_t>(idx));
        Ray r;
        r.ox = x[0]; r.oy = x[1]; r.oz = x[2]; r.ix = x[3]; r.iy = x[4]; r.iz = x[5]; r.dx = x[6]; r.dy = x[7]; r.dz = x[8];
        if (mask_cache_ray_ok(r) != ray_ok_plain(x) && !bad) { bad = true; first = idx; }
    }
    const uint64_t m = __ballot(bad);
    if (bad) { atomicAdd(out + 0, 1ull); atomicMin(out + 2, static_cast<unsigned long long>(first)); }
    if ((threadIdx.x & 63u) == 0u) atomicAdd(out + 1, 64ull * kOkPerThread);
    (void)m;
}

// triples (v, lo, hi): mode 0 = every triple of the boundary set `set` (n values; thread = (v, lo, hi) index), mode 1 = random
// triples, v mostly near lo or hi.  Triples without finite lo <= hi and finite v are skipped.
__global__ void dev_kernel(uint64_t seed, int mode, uint64_t base, uint32_t n, const float* set, unsigned long long* out) {
    const uint64_t idx = base + static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    float v, lo, hi;
    if (mode == 0) {
        if (idx >= static_cast<uint64_t>(n) * n * n) return;
        v = set[idx % n]; lo = set[(idx / n) % n]; hi = set[idx / (static_cast<uint64_t>(n) * n)];
    } else {
        const uint64_t h = mix64(seed ^ mix64(idx)), h2 = mix64(h ^ 0x5555u), h3 = mix64(h2 ^ 0xAAAAu);
        const float a = pick(h, 0, 254), bb = (h & 0x30000u) == 0u ? pick(h2, 0, 254) : a + pick(h2, 0, 254);
        lo = fminf(a, bb); hi = fmaxf(a, bb);
        const uint32_t k = static_cast<uint32_t>(h3 & 7u);
        v = k == 0u ? lo : k == 1u ? hi : k == 2u ? step(lo, false) : k == 3u ? step(hi, true) : k == 4u ? step(lo, true)
          : k == 5u ? step(hi, false) : k == 6u ? lerp_in(lo, hi, unit(h3)) : pick(h3, 0, 254);
    }
    const bool valid = fabsf(v) <= FLT_MAX && fabsf(lo) <= FLT_MAX && fabsf(hi) <= FLT_MAX && lo <= hi;
    const bool bad = valid && ((bounds_deviation(v, lo, hi) != 0.0f) != (v < lo || v > hi));
    if (bad) { atomicAdd(out + 0, 1ull); atomicMin(out + 2, static_cast<unsigned long long>(idx)); }
    const uint64_t nv = __popcll(__ballot(valid));
    if ((threadIdx.x & 63u) == __ffsll(static_cast<unsigned long long>(__ballot(true))) - 1 && nv) atomicAdd(out + 1, nv);
}

// ---- (d) mask_cache_begin_pass ------------------------------------------------------------------------------------------------------
constexpr int kPasses = 64;
constexpr int kEntryDwords = kMaskCacheDwords - kMaskCacheHeader;
static_assert(kEntryDwords % 64 == 0 && (kLeafMaskBase - kMaskCacheHeader) % 64 == 0, "entries: whole dwords per lane");
__device__ __forceinline__ uint32_t entry_val(uint64_t seed, uint64_t c, int i, uint32_t lane) {
    return static_cast<uint32_t>(hsh(seed, c, 5000u + static_cast<uint32_t>(i) * 64u + lane));
}
__device__ __forceinline__ bool same_or_zero(float a, float b) { return as_u(a) == as_u(b) || (a == 0.0f && b == 0.0f); }

// One wave runs kPasses calls on its own 16-byte aligned region; every lane is in EXEC for each call.  Case index = wave * kPasses + pass.
__global__ void __launch_bounds__(256) pass_kernel(uint64_t seed, unsigned long long* out) {
    __shared__ __align__(16) uint32_t lds[4 * kMaskCacheDwords];
    __shared__ float rays[4][9][64];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * 4u + w;
    uint32_t* const base = lds + w * kMaskCacheDwords;
    const MaskCache mc{base};
    if (lane < static_cast<uint32_t>(kMaskCacheHeader)) base[lane] = static_cast<uint32_t>(hsh(seed, wave, 100u + lane));  // garbage
    if (lane == 0u) base[kHdrState] = 0xFFFFFFFFu;
    wave_lds_sync();
    uint32_t oct = static_cast<uint32_t>(hsh(seed, wave, 99)) & 7u;
    for (int pass = 0; pass < kPasses; pass++) {
        const uint64_t c = wave * kPasses + static_cast<uint64_t>(pass);
        const uint64_t hp = hsh(seed, c, 0);
        if ((hp & 7u) == 0u) oct = static_cast<uint32_t>(hp >> 8) & 7u;  // mostly the previous pattern
        for (int i = 0; i < kEntryDwords / 64; i++) base[kMaskCacheHeader + i * 64 + static_cast<int>(lane)] = entry_val(seed, c, i, lane);
        wave_lds_sync();
        float oh[32];
        for (int i = 0; i < 32; i++) oh[i] = as_f(base[i]);
        const bool valid = as_u(oh[kHdrState]) == (oct | 0x100u);
        // active lanes
        const uint32_t ak = static_cast<uint32_t>(hp >> 16) % 7u;
        const uint64_t rnd = hsh(seed, c, 1);
        const uint64_t am = ak == 0u ? ~0ull : ak == 1u ? 0ull : ak == 2u ? 1ull << ((hp >> 24) & 63u) : ak == 3u ? ~0ull >> 1
                          : ak == 4u ? ((hp >> 30) & 1u ? 0xAAAAAAAAAAAAAAAAull : 0x5555555555555555ull) : ak == 5u ? rnd : rnd | ~0ull << 60;
        const bool active = (am >> lane) & 1u;
        // this lane's ray: inside the current B, on a face, one ulp outside or far (outside only in passes that allow it)
        const bool may_leave = ((hp >> 40) & 1u) != 0u;
        float val[9];
        for (int g = 0; g < 3; g++) {
            for (int k = 0; k < 3; k++) {
                const uint64_t h = hsh(seed, c, 10u + lane * 9u + static_cast<uint32_t>(g * 3 + k));
                const uint32_t pos = static_cast<uint32_t>(h & 7u);
                const float lo = oh[hdr_lo(g) + k], hi = oh[hdr_lo(g) + 3 + k];
                float x;
                if (valid && lo <= hi && pos < 3u) x = lerp_in(lo, hi, unit(h));
                else if (valid && lo <= hi && pos < 5u) x = pos == 3u ? lo : hi;
                else if (valid && lo <= hi && pos == 5u && may_leave) x = (h >> 8) & 1u ? step(lo, false) : step(hi, true);
                else if (valid && lo <= hi && !may_leave) x = lo;
                else x = g == 2 ? pick(h, 127 - 20, 127 + 1) : pick(h, 127 - 20, g == 0 ? 127 + 30 : 127 + 20);
                if (g == 0) x = clampf(x, -kCoordCap, kCoordCap);
                if (g == 2) x = clampf(x, -2.0f, 2.0f);
                if (g == 1) {
                    x = clampf(fabsf(x), 0x1p-149f, FLT_MAX);
                    if ((oct >> k) & 1u) x = -x;
                }
                val[g * 3 + k] = active ? x : as_f(static_cast<uint32_t>(h >> 32) | ((h & 0x30u) ? 0x7F800000u : 0u));  // garbage: NaN, inf
            }
        }
        for (int i = 0; i < 9; i++) rays[w][i][lane] = val[i];
        Ray r;
        r.ox = val[0]; r.oy = val[1]; r.oz = val[2]; r.ix = val[3]; r.iy = val[4]; r.iz = val[5]; r.dx = val[6]; r.dy = val[7]; r.dz = val[8];
        wave_lds_sync();
        mask_cache_begin_pass(mc, r, active, oct);
        wave_lds_sync();
        // the rule, restated serially over the wave's rays
        bool outside = false;
        for (int g = 0; g < 3; g++)
            for (int k = 0; k < 3; k++) outside = outside || val[g * 3 + k] < oh[hdr_lo(g) + k] || val[g * 3 + k] > oh[hdr_lo(g) + 3 + k];
        const bool rewrite = __ballot(active && (!valid || outside)) != 0;
        float nh[32];
        for (int i = 0; i < 32; i++) nh[i] = as_f(base[i]);
        bool bad = false;
        if (rewrite) {
            for (int g = 0; g < 3; g++) {
                for (int k = 0; k < 3; k++) {
                    float lo = INFINITY, hi = -INFINITY;
                    for (int l = 0; l < 64; l++) {
                        if (!((am >> l) & 1u)) continue;
                        const float x = rays[w][g * 3 + k][l];
                        if (x < lo) lo = x;
                        if (x > hi) hi = x;
                    }
                    if (valid) { lo = oh[hdr_lo(g) + k] < lo ? oh[hdr_lo(g) + k] : lo; hi = oh[hdr_lo(g) + 3 + k] > hi ? oh[hdr_lo(g) + 3 + k] : hi; }
                    const float pad = (hi - lo) * MP_MCACHE_PAD;
                    float wlo = lo - pad, whi = hi + pad;
                    if (g == 1) {  // keep the pattern's sign, non-zero and finite, or do not widen
                        const bool neg = ((oct >> k) & 1u) != 0u;
                        if (!(neg ? (wlo < 0.0f && wlo > -INFINITY) : (wlo > 0.0f && wlo < INFINITY))) wlo = lo;
                        if (!(neg ? (whi < 0.0f && whi > -INFINITY) : (whi > 0.0f && whi < INFINITY))) whi = hi;
                    } else {
                        const float cap = g == 0 ? kOrgCap : 2.0f;
                        if (wlo < -cap) wlo = -cap;
                        if (whi > cap) whi = cap;
                    }
                    bad = bad || !same_or_zero(nh[hdr_lo(g) + k], wlo) || !same_or_zero(nh[hdr_lo(g) + 3 + k], whi);
                }
            }
            bad = bad || as_u(nh[kHdrState]) != (oct | 0x100u);
        } else {
            for (int i = 0; i < 19; i++) bad = bad || as_u(nh[i]) != as_u(oh[i]);
        }
        for (int i = 19; i < 32; i++) bad = bad || as_u(nh[i]) != as_u(oh[i]);  // slots the header does not use
        if (as_u(nh[kHdrState]) == (oct | 0x100u)) {  // the invariants of a valid B
            for (int k = 0; k < 3; k++) {
                const bool neg = ((oct >> k) & 1u) != 0u;
                const float ilo = nh[6 + k], ihi = nh[9 + k];
                bad = bad || !(ilo <= ihi) || !(fabsf(ilo) <= FLT_MAX) || !(fabsf(ihi) <= FLT_MAX);
                bad = bad || (neg ? !(ihi < 0.0f) : !(ilo > 0.0f));
                bad = bad || !(nh[k] >= -kOrgCap && nh[k] <= nh[3 + k] && nh[3 + k] <= kOrgCap);
                bad = bad || !(nh[13 + k] >= -2.0f && nh[13 + k] <= nh[16 + k] && nh[16 + k] <= 2.0f);
            }
        }
        // every active ray inside the new B
        bool lane_bad = false;
        for (int g = 0; g < 3; g++)
            for (int k = 0; k < 3; k++) lane_bad = lane_bad || (active && !(val[g * 3 + k] >= nh[hdr_lo(g) + k] && val[g * 3 + k] <= nh[hdr_lo(g) + 3 + k]));
        // node entries and leaf tags: all cleared after a rewrite, untouched otherwise; leaf masks: untouched (a cleared tag voids them)
        for (int i = 0; i < kEntryDwords / 64; i++) {
            const uint32_t e = base[kMaskCacheHeader + i * 64 + static_cast<int>(lane)];
            const bool cleared = rewrite && i < (kLeafMaskBase - kMaskCacheHeader) / 64;
            lane_bad = lane_bad || e != (cleared ? 0xFFFFFFFFu : entry_val(seed, c, i, lane));
        }
        bad = bad || __ballot(lane_bad) != 0;
        if (lane == 0u) {
            atomicAdd(out + 1, 1ull);
            if (rewrite) atomicAdd(out + 6, 1ull);
            if (bad) { atomicAdd(out + 0, 1ull); atomicMin(out + 2, static_cast<unsigned long long>(c)); }
        }
        wave_lds_sync();
    }
}

// ---- (e) mask_cache_begin_unit ------------------------------------------------------------------------------------------------------
// One wave per pixel block {x0, x1, y0, y1}: the header starts as garbage and every node / leaf tag as its own index (never
// 0xFFFFFFFF); out[20 * unit ..] = header dwords 0..18 after the call, then the number of tags that read 0xFFFFFFFF.
constexpr int kUnitOut = 20;
struct SamplerArg {
    mp_camera_sampler s;
};
__global__ void __launch_bounds__(256) unit_kernel(SamplerArg cam, float jitter_scale, const uint32_t* blocks, uint32_t n, uint32_t* out) {
    __shared__ __align__(16) uint32_t lds[4 * kMaskCacheDwords];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t unit = blockIdx.x * 4u + w;
    if (unit >= n) return;  // (whole waves)
    uint32_t* const base = lds + w * kMaskCacheDwords;
    if (lane < static_cast<uint32_t>(kMaskCacheHeader)) base[lane] = static_cast<uint32_t>(hsh(0x0E17ull, unit, lane));
    constexpr int kTags = kLeafMaskBase - kMaskCacheHeader;
    for (int i = 0; i < kTags / 64; i++) base[kMaskCacheHeader + i * 64 + static_cast<int>(lane)] = static_cast<uint32_t>(i * 64) + lane;
    wave_lds_sync();
    mask_cache_begin_unit(MaskCache{base}, cam.s, jitter_scale, blocks[4 * unit], blocks[4 * unit + 1], blocks[4 * unit + 2], blocks[4 * unit + 3]);
    wave_lds_sync();
    uint32_t cleared = 0u;
    for (int i = 0; i < kTags / 64; i++) cleared += static_cast<uint32_t>(__popcll(__ballot(base[kMaskCacheHeader + i * 64 + static_cast<int>(lane)] == 0xFFFFFFFFu)));
    if (lane < 19u) out[kUnitOut * unit + lane] = base[lane];
    if (lane == 19u) out[kUnitOut * unit + 19u] = cleared;
}

// ---- (f) unit_list_build -------------------------------------------------------------------------------------------------------------
// One wave per case (node, arena entries already in use): the cache starts with the case's header, every tag cleared and the
// arena's fill set, and the wave calls the builder the walk calls, behind a real call as in the walk.  out[kListOut * case ..] =
// returned value, arena entries in use afterwards, the tag and the value of the node's slot, then the whole arena.
constexpr int kListOut = 4 + kArenaRoom;
template <int OCT>
__device__ __noinline__ uint32_t list_slow(const float4* __restrict__ recs, uint32_t* mcache, uint32_t node, uint32_t slots) {
    return unit_list_build(recs, mcache, node, slots,
                           [](const float* b, const float bmn[3], const float bmx[3]) { return bounds_may_hit<OCT>(b, bmn, bmx); });
}
__global__ void __launch_bounds__(256) list_kernel(const float4* recs, uint32_t slots, const uint32_t* headers, const uint32_t* cases, uint32_t n,
                                                   uint32_t* out) {
    __shared__ __align__(16) uint32_t lds[4 * kMaskCacheDwords];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t c = blockIdx.x * 4u + w;
    if (c >= n) return;  // (whole waves)
    uint32_t* const base = lds + w * kMaskCacheDwords;
    for (uint32_t i = lane; i < static_cast<uint32_t>(kMaskCacheDwords); i += 64u)
        base[i] = i < static_cast<uint32_t>(kMaskCacheHeader) ? headers[32u * c + i] : i < static_cast<uint32_t>(kLeafMaskBase) ? 0xFFFFFFFFu : 0xDEAD0000u + i;
    wave_lds_sync();
    const uint32_t node = cases[2u * c], top0 = cases[2u * c + 1u];
    if (lane == 0u) base[kArenaTopSlot] = ~top0;
    wave_lds_sync();
    uint32_t val;
    switch (__builtin_amdgcn_readfirstlane(base[kHdrState]) & 7u) {
        case 0: val = list_slow<0>(recs, base, node, slots); break;
        case 1: val = list_slow<1>(recs, base, node, slots); break;
        case 2: val = list_slow<2>(recs, base, node, slots); break;
        case 3: val = list_slow<3>(recs, base, node, slots); break;
        case 4: val = list_slow<4>(recs, base, node, slots); break;
        case 5: val = list_slow<5>(recs, base, node, slots); break;
        case 6: val = list_slow<6>(recs, base, node, slots); break;
        default: val = list_slow<7>(recs, base, node, slots); break;
    }
    wave_lds_sync();
    uint32_t* const o = out + static_cast<size_t>(c) * kListOut;
    if (lane == 0u) {
        const uint32_t slot = node_slot(node);
        o[0] = val; o[1] = ~base[kArenaTopSlot]; o[2] = base[static_cast<uint32_t>(kMaskCacheHeader) + slot]; o[3] = base[static_cast<uint32_t>(kNodeListBase) + slot];
    }
    for (uint32_t i = lane; i < static_cast<uint32_t>(kArenaRoom); i += 64u) o[4u + i] = base[static_cast<uint32_t>(kArenaBase) + i];
}

// ---- (g) mask_cache_pass_inside: the pass-entry decision --------------------------------------------------------------------------
// One wave per hand-made pass: the header (32 dwords) goes to the wave's cache as given, lane l's ray is rays[(case * 9 + i) * 64 + l]
// (i = 0..2 origin, 3..5 inverse direction, 6..8 direction), bit l of active[case] says whether the lane is active.
// out[case] = the returned pattern (0..7) or kNoPattern.
__global__ void __launch_bounds__(256) entry_kernel(const uint32_t* headers, const float* rays, const uint64_t* active, uint32_t n, uint32_t* out) {
    __shared__ __align__(16) uint32_t lds[4 * kMaskCacheHeader];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t c = blockIdx.x * 4u + w;
    if (c >= n) return;  // (whole waves)
    uint32_t* const base = lds + w * kMaskCacheHeader;
    if (lane < static_cast<uint32_t>(kMaskCacheHeader)) base[lane] = headers[static_cast<size_t>(c) * kMaskCacheHeader + lane];
    wave_lds_sync();
    const float* x = rays + static_cast<size_t>(c) * 9u * 64u + lane;
    Ray r;
    r.ox = x[0]; r.oy = x[64]; r.oz = x[128]; r.ix = x[192]; r.iy = x[256]; r.iz = x[320]; r.dx = x[384]; r.dy = x[448]; r.dz = x[512];
    const uint32_t got = mask_cache_pass_inside(MaskCache{base}, r, ((active[c] >> lane) & 1ull) != 0ull);
    if (lane == 0u) out[c] = got;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// One launch on a fresh counter buffer.  HIP's last-error state is per thread and sticky: an error that earlier work of the process
// left there is not this probe's, so it is cleared before the launch, and every call's own status is checked (probe.hip).
template <class F>
int run(F launch, unsigned long long* host) {
    (void)hipGetLastError();
    unsigned long long* dev = nullptr;
    unsigned long long init[kCounters] = {0ull, 0ull, ~0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    hipError_t e = hipMalloc(&dev, sizeof(init));
    if (e != hipSuccess) return static_cast<int>(e);
    e = hipMemcpy(dev, init, sizeof(init), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch(dev);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(host, dev, sizeof(init), hipMemcpyDeviceToHost);
    }
    const hipError_t ef = hipFree(dev);
    return static_cast<int>(e != hipSuccess ? e : ef);
}
void merge(unsigned long long* acc, const unsigned long long* r) {
    for (int i = 0; i < kCounters; i++) if (i != 2) acc[i] += r[i];
    if (r[2] < acc[2]) acc[2] = r[2];
}
void reset(unsigned long long* acc) {
    for (int i = 0; i < kCounters; i++) acc[i] = 0ull;
    acc[2] = ~0ull;
}
constexpr uint64_t kCasesPerLaunch = 1ull << 20;  // 2^20 waves: 2^18 blocks of four

// ncases cases of kernel K (tri_kernel or box_kernel), in launches of kCasesPerLaunch
template <class K>
int run_cases(K kernel, uint64_t seed, uint64_t ncases, uint32_t* dump_dev, unsigned long long* out) {
    unsigned long long acc[kCounters];
    reset(acc);
    for (uint64_t c0 = 0; c0 < ncases; c0 += kCasesPerLaunch) {
        const uint64_t n = ncases - c0 < kCasesPerLaunch ? ncases - c0 : kCasesPerLaunch;
        unsigned long long r[kCounters];
        if (int rc = run([&](unsigned long long* d) {
                hipLaunchKernelGGL(kernel, dim3(static_cast<uint32_t>((n + 3) / 4)), dim3(256), 0, 0, seed, c0, c0 + n, d, dump_dev);
            }, r))
            return rc;
        merge(acc, r);
    }
    for (int i = 0; i < kCounters; i++) out[i] = acc[i];
    return 0;
}

}  // namespace

extern "C" {
// (a) tri_may_hit: ncases cases
int mp_mask_probe_tri(uint64_t seed, uint64_t ncases, unsigned long long* out) { return run_cases(tri_kernel, seed, ncases, nullptr, out); }
// (a') tri_exit1_key / tri_exit2_key, the wave's decision: ncases cases
int mp_mask_probe_exits(uint64_t seed, uint64_t ncases, unsigned long long* out) { return run_cases(exit_kernel, seed, ncases, nullptr, out); }
// (a'') tri_may_hit on boxes beyond the far edges and on exact-boundary cases: ncases cases
int mp_mask_probe_far(uint64_t seed, uint64_t ncases, unsigned long long* out) { return run_cases(far_kernel, seed, ncases, nullptr, out); }
// (b) bounds_may_hit<OCT>: ncases cases, case c of pattern c & 7
int mp_mask_probe_box(uint64_t seed, uint64_t ncases, unsigned long long* out) { return run_cases(box_kernel, seed, ncases, nullptr, out); }
// (a) / (b) with a dump of every case to `host` (ncases * mp_mask_probe_dump_dwords() dwords): kind 0 triangles, 1 boxes
int mp_mask_probe_dump_dwords() { return kDumpCase; }
int mp_mask_probe_dump(int kind, uint64_t seed, uint64_t ncases, uint32_t* host, unsigned long long* out) {
    (void)hipGetLastError();
    uint32_t* dev = nullptr;
    const size_t bytes = static_cast<size_t>(ncases) * kDumpCase * sizeof(uint32_t);
    hipError_t e = hipMalloc(&dev, bytes);
    if (e != hipSuccess) return static_cast<int>(e);
    e = hipMemset(dev, 0, bytes);
    int rc = static_cast<int>(e);
    if (e == hipSuccess) rc = kind == 0 ? run_cases(tri_kernel, seed, ncases, dev, out) : run_cases(box_kernel, seed, ncases, dev, out);
    if (rc == 0) rc = static_cast<int>(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    const hipError_t ef = hipFree(dev);
    return rc != 0 ? rc : static_cast<int>(ef);
}
// (c) mask_cache_ray_ok: every bit pattern in each of the nine components (9 x 2^32 rays)
int mp_mask_probe_ray_ok(uint64_t seed, unsigned long long* out) {
    unsigned long long acc[kCounters];
    reset(acc);
    constexpr uint64_t kThreads = (1ull << 32) / kOkPerThread, kBlocks = kThreads / 256;
    for (int comp = 0; comp < 9; comp++) {
        unsigned long long r[kCounters];
        if (int rc = run([&](unsigned long long* d) {
                hipLaunchKernelGGL(ray_ok_kernel, dim3(static_cast<uint32_t>(kBlocks)), dim3(256), 0, 0, seed, comp, 0ull, d);
            }, r))
            return rc;
        if (r[2] != ~0ull) r[2] += static_cast<unsigned long long>(comp) << 32;  // index = component << 32 | bit pattern
        merge(acc, r);
    }
    for (int i = 0; i < kCounters; i++) out[i] = acc[i];
    return 0;
}
// (c) bounds_deviation: every triple of the n values `set` (host array), then nrandom random triples
int mp_mask_probe_dev(uint64_t seed, const float* set, uint32_t n, uint64_t nrandom, unsigned long long* out) {
    (void)hipGetLastError();
    float* dset = nullptr;
    hipError_t e = hipMalloc(&dset, sizeof(float) * (n ? n : 1u));
    if (e != hipSuccess) return static_cast<int>(e);
    e = hipMemcpy(dset, set, sizeof(float) * n, hipMemcpyHostToDevice);
    int rc = static_cast<int>(e);
    unsigned long long acc[kCounters];
    reset(acc);
    const uint64_t ntrip = static_cast<uint64_t>(n) * n * n;
    if (rc == 0 && ntrip) {
        unsigned long long r[kCounters];
        rc = run([&](unsigned long long* d) {
            hipLaunchKernelGGL(dev_kernel, dim3(static_cast<uint32_t>((ntrip + 255) / 256)), dim3(256), 0, 0, seed, 0, 0ull, n, dset, d);
        }, r);
        if (rc == 0) merge(acc, r);
    }
    if (rc == 0 && nrandom) {
        unsigned long long r[kCounters];
        rc = run([&](unsigned long long* d) {
            hipLaunchKernelGGL(dev_kernel, dim3(static_cast<uint32_t>((nrandom + 255) / 256)), dim3(256), 0, 0, seed, 1, 0ull, n, dset, d);
        }, r);
        if (rc == 0) { if (r[2] != ~0ull) r[2] += 1ull << 40; merge(acc, r); }  // random triples: index 2^40 + i
    }
    const hipError_t ef = hipFree(dset);
    if (rc != 0) return rc;
    for (int i = 0; i < kCounters; i++) out[i] = acc[i];
    return static_cast<int>(ef);
}
// (e) mask_cache_begin_unit: n pixel blocks {x0, x1, y0, y1} (host) under the sampler's 15 floats -> 20 dwords per block (host):
// the header and the number of cleared tags; *ntags = tags per wave, *margin = the MP_MCACHE_MARGIN the probe was built with
int mp_mask_probe_unit(const float* sampler, float jitter_scale, const uint32_t* blocks, uint32_t n, uint32_t* out, uint32_t* ntags,
                       float* margin) {
    (void)hipGetLastError();
    *ntags = static_cast<uint32_t>(kLeafMaskBase - kMaskCacheHeader);
    *margin = MP_MCACHE_MARGIN;
    if (n == 0u) return 0;
    SamplerArg cam;
    const float* p = sampler;
    for (int k = 0; k < 3; k++) { cam.s.center[k] = p[k]; cam.s.up[k] = p[3 + k]; cam.s.right[k] = p[6 + k]; cam.s.film_origin_offset[k] = p[9 + k]; }
    cam.s.pixel_scale = p[12]; cam.s.lens_radius = p[13]; cam.s.lens_weight = p[14];
    uint32_t *dblocks = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc(&dblocks, sizeof(uint32_t) * 4u * n);
    if (e == hipSuccess) e = hipMalloc(&dout, sizeof(uint32_t) * kUnitOut * n);
    if (e == hipSuccess) e = hipMemcpy(dblocks, blocks, sizeof(uint32_t) * 4u * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(unit_kernel, dim3((n + 3u) / 4u), dim3(256), 0, 0, cam, jitter_scale, dblocks, n, dout);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(out, dout, sizeof(uint32_t) * kUnitOut * n, hipMemcpyDeviceToHost);
    }
    (void)hipFree(dblocks);
    (void)hipFree(dout);
    return static_cast<int>(e);
}
// (d) mask_cache_begin_pass: nwaves waves (a multiple of 4) of 64 passes each
int mp_mask_probe_pass(uint64_t seed, uint64_t nwaves, unsigned long long* out) {
    return run([&](unsigned long long* d) {
        hipLaunchKernelGGL(pass_kernel, dim3(static_cast<uint32_t>(nwaves / 4)), dim3(256), 0, 0, seed, d);
    }, out);
}
// (g) mask_cache_pass_inside: ncases passes (host arrays: 32 header dwords, 9 x 64 ray components and one active mask per case) ->
// one dword per case, the pattern or *no_pattern
int mp_mask_probe_entry(const uint32_t* headers, const float* rays, const uint64_t* active, uint32_t ncases, uint32_t* out, uint32_t* no_pattern) {
    (void)hipGetLastError();
    *no_pattern = kNoPattern;
    if (ncases == 0u) return 0;
    uint32_t *dhdr = nullptr, *dout = nullptr;
    float* drays = nullptr;
    uint64_t* dact = nullptr;
    const size_t hdr_bytes = sizeof(uint32_t) * kMaskCacheHeader * ncases, ray_bytes = sizeof(float) * 9u * 64u * ncases;
    hipError_t e = hipMalloc(&dhdr, hdr_bytes);
    if (e == hipSuccess) e = hipMalloc(&drays, ray_bytes);
    if (e == hipSuccess) e = hipMalloc(&dact, sizeof(uint64_t) * ncases);
    if (e == hipSuccess) e = hipMalloc(&dout, sizeof(uint32_t) * ncases);
    if (e == hipSuccess) e = hipMemcpy(dhdr, headers, hdr_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(drays, rays, ray_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dact, active, sizeof(uint64_t) * ncases, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(entry_kernel, dim3((ncases + 3u) / 4u), dim3(256), 0, 0, dhdr, drays, dact, ncases, dout);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(out, dout, sizeof(uint32_t) * ncases, hipMemcpyDeviceToHost);
    }
    (void)hipFree(dhdr); (void)hipFree(drays); (void)hipFree(dact); (void)hipFree(dout);
    return static_cast<int>(e);
}
// (f) unit_list_build: the tree `recs` (n_nodes nodes of `slots` records of 8 dwords, as mp_scene_device_tree exports it; every inner
// link must name a node of it), ncases headers of 32 dwords and cases {node, arena entries in use} -> mp_mask_probe_list_dwords()
// dwords per case.  info (may be null): {arena entries, node table entries, dword index of the arena's first entry}.  Returns -1 for
// a case outside the tree or the arena.
int mp_mask_probe_list_dwords() { return kListOut; }
int mp_mask_probe_list(const uint32_t* recs, uint32_t n_nodes, uint32_t slots, const uint32_t* headers, const uint32_t* cases, uint32_t ncases,
                       uint32_t* out, uint32_t* info) {
    (void)hipGetLastError();
    if (info) { info[0] = static_cast<uint32_t>(kArenaEntries); info[1] = static_cast<uint32_t>(kMaskCacheEntries); info[2] = static_cast<uint32_t>(kArenaBase); }
    if (slots != 8u && slots != 16u) return -1;
    for (uint32_t c = 0; c < ncases; c++)
        if (cases[2u * c] >= n_nodes || cases[2u * c + 1u] > static_cast<uint32_t>(kArenaEntries)) return -1;
    for (size_t i = 0; i < static_cast<size_t>(n_nodes) * slots; i++) {
        const uint32_t link = recs[i * 8u + 6u];
        if (link != kNullLink && (link & 63u) == 0u && (link >> 6) >= n_nodes) return -1;
    }
    if (ncases == 0u) return 0;
    uint32_t *drecs = nullptr, *dhdr = nullptr, *dcases = nullptr, *dout = nullptr;
    const size_t rec_bytes = sizeof(uint32_t) * 8u * slots * n_nodes, out_bytes = sizeof(uint32_t) * kListOut * static_cast<size_t>(ncases);
    hipError_t e = hipMalloc(&drecs, rec_bytes);
    if (e == hipSuccess) e = hipMalloc(&dhdr, sizeof(uint32_t) * 32u * ncases);
    if (e == hipSuccess) e = hipMalloc(&dcases, sizeof(uint32_t) * 2u * ncases);
    if (e == hipSuccess) e = hipMalloc(&dout, out_bytes);
    if (e == hipSuccess) e = hipMemcpy(drecs, recs, rec_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dhdr, headers, sizeof(uint32_t) * 32u * ncases, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dcases, cases, sizeof(uint32_t) * 2u * ncases, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(list_kernel, dim3((ncases + 3u) / 4u), dim3(256), 0, 0, reinterpret_cast<const float4*>(drecs), slots, dhdr, dcases, ncases, dout);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost);
    }
    (void)hipFree(drecs); (void)hipFree(dhdr); (void)hipFree(dcases); (void)hipFree(dout);
    return static_cast<int>(e);
}
}
