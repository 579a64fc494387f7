// gfx950 (CDNA4) kernels for minipath's per-pixel sampling hot path.
//
// Lane mapping (DESIGN.md "Kernels"):
//   * ray generation, shading and accumulation are LANE-PARALLEL: one (pixel, sample) per lane;
//   * BVH traversal is GROUP-PARALLEL: a 64-wide wavefront is 8 groups of 8 lanes, one ray per group, lane i of a
//     group owns child i of an inner node / triangle i of a leaf packet -- the reference's 8-wide AVX2 lane i
//     (ray_bvh_intersection.rs:104-162).  The wavefront keeps a ray queue and eight traversal stacks in LDS;
//     active rays are compacted into the queue with __ballot + mbcnt and groups pull the next ray when they finish.
//
// Arithmetic contract: f32, compiled with -ffp-contract=off; fused multiply-adds only where the reference writes
// mul_add / mul_sub (util/simba.rs:57-67); IEEE division and sqrt; no fast-math.  The results are bit-identical to
// the CPU oracle's.
//
// Translation units.  The kernel families are being moved into units of their own, one family at a time, each over the device
// headers it needs and each with its own sub-table of kernel_table.h: so far the ray queries (kernels_queries.hip over group_walk.h
// and wave_common.h).  This file holds the families that have not moved yet, the utility kernels, and what stays here for good: the
// launch_* entry points of mp_internal.h and the launch record (family_launch.h is what the other units share with it).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "launch_plan.h"
#include "mp_internal.h"
#include "family_launch.h"
#include "ray_math.h"

#ifdef MP_PROF_MISSES  // profiling builds only (tools/build_variant.sh): slow-path calls of the mask cache, read by mp_prof_read
namespace mp {
namespace {
__device__ unsigned long long g_prof[10];  // [0] list builds [1] leaf-mask builds [2] inner links followed [3] bound sets [4] table evictions [5] arena resets [6] passes left to the uncached walk [7] pops skipped on an empty-mask leaf [8] units that skip the per-ray scene pre-test [9] units that keep it
}  // namespace
}  // namespace mp
#define MP_PROF_COUNT(i) do { if ((threadIdx.x & 63u) == 0u) atomicAdd(&g_prof[i], 1ull); } while (0)
#endif
#include "mask_cache.h"
#include "group_walk.h"

namespace mp {
namespace {

// Work the cached packet kernels (MCACHE = true) do once per unit instead of once per pass, each with a switch for A/B builds
// (tools/build_variant.sh) that gives the per-pass code back: the sample key's part that is fixed per unit (-DMP_NO_KEY_HOIST), the scene
// pre-test decided per unit (-DMP_NO_UNIT_PRETEST), and the shading normal's short normalisation (-DMP_NO_SHORT_NORMAL).
#ifdef MP_NO_KEY_HOIST
constexpr bool kKeyHoist = false;
#else
constexpr bool kKeyHoist = true;
#endif
#ifdef MP_NO_UNIT_PRETEST
constexpr bool kUnitPretest = false;
#else
constexpr bool kUnitPretest = true;
#endif
#ifdef MP_NO_SHORT_NORMAL
constexpr bool kShortNormal = false;
#else
constexpr bool kShortNormal = true;
#endif

// ---- fused tile render: Worker::render_tile (worker.rs:32-49) for a list of tiles -----------------------------
struct RenderParams {
    DevScene scene;
    RayGen gen;
    const mp_block* tiles;
    uint32_t n_tiles, tile_size;
    float* out;           // tile-major RGBA f32
    uint32_t* counter;    // work-queue head
    float inv_spp;        // 1.0 / spp as f32 (worker.rs:44)
    uint32_t s_begin, s_end;  // samples of this launch (progressive accumulation: a sub-range of [0, spp))
    uint32_t carry_in;    // out holds the running sums / hit counts of samples [0, s_begin)
    uint32_t finalize;    // write the means (worker.rs:44); otherwise the running sums
    uint32_t chunked;     // MP_FLAG_CHUNKED_SUM: f32 sums over 256-sample chunks, f64 total kept in the tile buffer
    const uint32_t* tile_order;      // optional hand-out order: work slot k renders tile tile_order[k] (into that tile's own slot)
    unsigned long long* tile_cost;   // optional: += shader-clock cycles the waves spent on each tile
    uint32_t lds_per_wave;
    uint32_t max_depth;   // path extension only
    unsigned long long* segments;  // path extension: ray segments traced (Object::intersect calls), may be null
    float* pool;           // pooled path kernel: per-wave workspace (ray queue + parked path state), pool_stride floats per wave
    uint32_t pool_stride;
};

// worker.rs:40-44 with the running state of a pixel carried across launches (MP_FLAG_ACCUMULATE): rgb = sequential sample sum,
// a = hit count; the launch that draws the last sample writes the means.  Every lane of the pixel loads the same state.
//
// MP_FLAG_CHUNKED_SUM (build-defined, include/minipath_hip.h): the pixel's slot holds {x: f32 sum of the current 256-sample
// chunk, y: hit count, (z,w): f64 total of the finished chunks}.  The total stays in memory (one read-modify-write per pixel and
// chunk by the pixel's first lane), so the rule costs the render kernels no registers.
constexpr uint32_t kSumChunk = 256;
__device__ __forceinline__ void pixel_state_load(const RenderParams& P, size_t off, bool inpix, bool writer, float& acc, float& cnt) {
    acc = 0.0f;
    cnt = 0.0f;
    if (P.carry_in && inpix) {
        const float4 prev = *reinterpret_cast<const float4*>(P.out + off);
        acc = prev.x;
        cnt = P.chunked ? prev.y : prev.w;
    } else if (P.chunked && inpix && writer) {
        *reinterpret_cast<double*>(P.out + off + 2) = 0.0;
    }
}
// end of a chunk: total += (f64)chunk sum; the next chunk starts from +0
__device__ __forceinline__ void chunk_flush(const RenderParams& P, size_t off, bool writer, float& acc) {
    if (writer) {
        double* t = reinterpret_cast<double*>(P.out + off + 2);
        *t = *t + static_cast<double>(acc);
    }
    acc = 0.0f;
}
// `s_next` = index of the first sample NOT yet added (the launch's s_end)
__device__ __forceinline__ void pixel_state_store(const RenderParams& P, size_t off, float acc, float cnt) {
    if (P.chunked) {
        if (!P.finalize) {
            *reinterpret_cast<float2*>(P.out + off) = make_float2(acc, cnt);
            return;
        }
        double t = *reinterpret_cast<const double*>(P.out + off + 2);
        if ((P.s_end & (kSumChunk - 1u)) != 0u) t = t + static_cast<double>(acc);  // the last, partial chunk
        const double inv = 1.0 / static_cast<double>(P.gen.spp);
        const float m = static_cast<float>(t * inv), a = static_cast<float>(static_cast<double>(cnt) * inv);
        *reinterpret_cast<float4*>(P.out + off) = make_float4(m, m, m, a);
        return;
    }
    const float m = P.finalize ? acc * P.inv_spp : acc;  // worker.rs:44
    const float a = P.finalize ? cnt * P.inv_spp : cnt;
    *reinterpret_cast<float4*>(P.out + off) = make_float4(m, m, m, a);
}

// The render kernels take RenderParams by value (328 bytes of kernel arguments) but read it through the kernarg segment pointer,
// one short-lived VIEW per phase (unit setup, ray generation, walk, shading, accumulation): a compiler barrier on the pointer
// ends the life of everything loaded through the previous view, so a field costs an s_load from the constant cache where it is
// used instead of an SGPR for the whole kernel -- the walks need the scalar registers for their record double-buffers, and what
// did not fit was spilled to VGPR lanes and scratch (round 2: 78 SGPR + 4 VGPR spills in the packet kernel, 67 + 29 and 104 B of
// scratch in the path kernel).
typedef const __attribute__((address_space(4))) RenderParams* kparams_t;
__device__ __forceinline__ const RenderParams& params_view(kparams_t kp) { return kernarg_view<RenderParams>(kp); }
#define MP_KERNEL_PARAMS kparams_t KP = (kparams_t)__builtin_amdgcn_kernarg_segment_ptr()

// get_next_tile (machinery.rs:206-208) for wavefronts: kWorkQueues interleaved queues (mp_internal.h), home queue = this
// workgroup's XCD, the others once it is empty.  Wave-uniform; `state` = queue | consecutive dry queues << 8 (one SGPR: the
// packet kernel has none to spare).  Used as:  for (;;) { MP_NEXT_UNIT(unit); ... }
#define MP_NEXT_UNIT(unit)                                                                              \
    uint32_t unit;                                                                                      \
    {                                                                                                   \
        const uint32_t q_ = qstate & 0xFFu;                                                             \
        uint32_t idx_ = 0;                                                                              \
        if (lane == 0) idx_ = atomicAdd(P.counter + q_ * kWorkQueueStride, 1u);                         \
        idx_ = __builtin_amdgcn_readfirstlane(idx_);                                                    \
        unit = idx_ * kWorkQueues + q_;                                                                 \
        if (unit >= total || idx_ >= 0x10000000u) {                                                     \
            if ((qstate >> 8) + 1u == kWorkQueues) break;                                               \
            qstate = ((q_ + 1u) % kWorkQueues) | (((qstate >> 8) + 1u) << 8);                           \
            continue;                                                                                   \
        }                                                                                               \
        qstate = q_;                                                                                    \
    }

// S = samples of one pixel in flight in a wavefront (64/S pixels x S consecutive samples per pass).
template <int S, bool OBJ>
__global__ __launch_bounds__(256) void render_tiles_kernel(RenderParams) {
    extern __shared__ __align__(16) unsigned char smem[];
    MP_KERNEL_PARAMS;
    const RenderParams& P0 = params_view(KP);
    constexpr int BW = (S == 1) ? 8 : (S == 2) ? 8 : (S == 4) ? 4 : 4;
    constexpr int BH = 64 / S / BW;
    const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
    float* q = reinterpret_cast<float*>(smem + static_cast<size_t>(wave) * P0.lds_per_wave);
    uint2* stack = reinterpret_cast<uint2*>(q + kQueueFloats);
    const uint32_t ts = P0.tile_size;
    const uint32_t bx = (ts + BW - 1) / BW, by = (ts + BH - 1) / BH, upt = bx * by;
    const uint32_t total = P0.n_tiles * upt;
    const int pix = lane / S, sub = lane % S;

    uint32_t qstate = blockIdx.x % kWorkQueues;
    for (;;) {
        const RenderParams& P = params_view(KP);  // one view per work unit
        MP_NEXT_UNIT(unit)
        const uint32_t b = unit % upt;
        const uint32_t tile_i = P.tile_order ? P.tile_order[unit / upt] : unit / upt;
        const uint64_t t_unit = P.tile_cost ? __builtin_readcyclecounter() : 0;
        const mp_block T = P.tiles[tile_i];
        const uint32_t px = T.min_x + (b % bx) * BW + static_cast<uint32_t>(pix % BW);
        const uint32_t py = T.min_y + (b / bx) * BH + static_cast<uint32_t>(pix / BW);
        const bool inpix = px < T.max_x && py < T.max_y;
        if (__ballot(inpix) == 0) continue;
        const size_t off = (static_cast<size_t>(tile_i) * ts * ts + static_cast<size_t>(py - T.min_y) * ts + (px - T.min_x)) * 4;
        float acc, cnt;  // pixel_sum (r=g=b) and alpha (worker.rs:40)
        pixel_state_load(P, off, inpix, sub == 0, acc, cnt);
        // passes are aligned to multiples of S in the absolute sample index, so that a chunk boundary (MP_FLAG_CHUNKED_SUM) never
        // falls inside a pass; lanes outside [s_begin, s_end) add +0.0, which is exact
        for (uint32_t s0 = P.s_begin & ~static_cast<uint32_t>(S - 1); s0 < P.s_end; s0 += S) {
            const uint32_t s = s0 + static_cast<uint32_t>(sub);
            const bool act = inpix && s >= P.s_begin && s < P.s_end;
            Ray r;
            r.dx = r.dy = r.dz = 0.0f;
            if (act) sample_ray(P.gen, px, py, s, r);
            if (P.scene.kind == 1u) {  // Scene<Sphere>: no traversal, everything is lane-parallel
                float c = 0.0f, h = 0.0f, ts_, nn[3];
                if (act && sphere_intersect(P.scene, r, ts_, nn)) { c = fabsf(r.dx * nn[0] + r.dy * nn[1] + r.dz * nn[2]); h = 1.0f; }
#pragma unroll
                for (int j = 0; j < S; j++) {
                    acc += __shfl(c, (lane & ~(S - 1)) + j);
                    cnt += __shfl(h, (lane & ~(S - 1)) + j);
                }
                if (P.chunked && ((s0 + S) & (kSumChunk - 1u)) == 0u && s0 + S <= P.s_end) chunk_flush(P, off, inpix && sub == 0, acc);
                continue;
            }
            // group walk (once per member of an object group): closest hit, then the shading of worker.rs:59-65
            GroupHit gh;
            trace_objects<OBJ>(P.scene, r, act, q, stack, gh);
            float c = 0.0f, h = 0.0f;
            if (gh.prim != kNoPrim) {
                float nn[3];
                if (OBJ) object_normal(P.scene, gh.inst, r, gh.prim, gh.u, gh.v, nn);
                else resolve_normal(P.scene, gh.prim, gh.u, gh.v, nn);
                c = fabsf(r.dx * nn[0] + r.dy * nn[1] + r.dz * nn[2]);  // worker.rs:60
                h = 1.0f;
            }
            // pixel_sum += sample, strictly in sample order (worker.rs:41-43); inactive samples add +0.0 (exact)
#pragma unroll
            for (int j = 0; j < S; j++) {
                acc += __shfl(c, (lane & ~(S - 1)) + j);
                cnt += __shfl(h, (lane & ~(S - 1)) + j);
            }
            if (P.chunked && ((s0 + S) & (kSumChunk - 1u)) == 0u && s0 + S <= P.s_end) chunk_flush(P, off, inpix && sub == 0, acc);
        }
        if (inpix && sub == 0) pixel_state_store(P, off, acc, cnt);
        if (P.tile_cost && lane == 0) atomicAdd(P.tile_cost + tile_i, static_cast<unsigned long long>(__builtin_readcyclecounter() - t_unit));
    }
}


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
            MP_PROF_COUNT(2);
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
        // if it is slow and the generic MODE 1 walk otherwise (below, whether its signs are uniform or not).
        if (__ballot(active & !mask_cache_ray_ok(r)) != 0) {
            const bool slow = active && (fabsf(r.ix) == INFINITY || fabsf(r.iy) == INFINITY || fabsf(r.iz) == INFINITY);
            if (__ballot(slow) != 0) trace_packet_impl<2, -1>(sc, r, active, st, hit);
            else trace_packet_impl<1, -1>(sc, r, active, st, hit);
            return;
        }
    } else {
        const bool slow = active && (fabsf(r.ix) == INFINITY || fabsf(r.iy) == INFINITY || fabsf(r.iz) == INFINITY);
        if (__ballot(slow) != 0) {
            trace_packet_impl<2, -1>(sc, r, active, st, hit);
            return;
        }
    }
    if (OCTANTS && sc.boxes_ordered) {
        const uint64_t am = __ballot(active);
        const uint64_t nx = __ballot(active && r.ix < 0.0f), ny = __ballot(active && r.iy < 0.0f), nz = __ballot(active && r.iz < 0.0f);
        if ((nx == 0 || nx == am) && (ny == 0 || ny == am) && (nz == 0 || nz == am)) {
            const uint32_t oct = (nx ? 1u : 0u) | (ny ? 2u : 0u) | (nz ? 4u : 0u);
            if (MC) {  // kernels with a mask cache: the sign-specialised walks use it
                mask_cache_begin_pass(mc, r, active, oct);
                bool done;
                switch (oct) {
                    case 0: done = trace_packet_cached<0>(sc, r, active, hit, mc.lds); break;
                    case 1: done = trace_packet_cached<1>(sc, r, active, hit, mc.lds); break;
                    case 2: done = trace_packet_cached<2>(sc, r, active, hit, mc.lds); break;
                    case 3: done = trace_packet_cached<3>(sc, r, active, hit, mc.lds); break;
                    case 4: done = trace_packet_cached<4>(sc, r, active, hit, mc.lds); break;
                    case 5: done = trace_packet_cached<5>(sc, r, active, hit, mc.lds); break;
                    case 6: done = trace_packet_cached<6>(sc, r, active, hit, mc.lds); break;
                    default: done = trace_packet_cached<7>(sc, r, active, hit, mc.lds); break;
                }
                if (done) return;  // (else: a list did not fit the arena in mid-walk -- the generic walk below, from the start)
            } else {
                switch (oct) {
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

// ---- two rays per lane: 128 rays share one walk (opt-in: mp_ctx_set_option "packet_rays_per_lane" = 2) --------------------
// The walk's scalar work (record fetches, loop control, pops and pushes) does not depend on how many rays ride on it, and the
// scalar ALU is the unit the 64-ray walk saturates first (profiles/r02_notes.md).  Here every lane carries TWO rays (A and B: the
// same sample index in two pixels two columns apart), so the scalar work per ray halves and each fetched record feeds two
// independent vector dependency chains.  Per-ray decisions are exactly those of trace_packet_impl (same operations on the same
// operands: the frame is bit-identical, tested); an entry is visited while any ray of either set needs it.
// MEASURED SLOWER than the 64-ray walk on MI355X (metric's frame: 52.9 ms at 6 waves / 80 VGPRs, 54.2 at 5, 56.5 at 4, against
// 48.6 ms; teapot 13.5 against 12.4): the union of two 2x2-pixel packets is visited by twice the vector work, the wave-level
// early-outs fire less often, and the 80-VGPR budget spills in the pop loop.  Kept as the measured alternative, not the default.
struct RegStack2 {
    int link, src, alo, ahi, blo, bhi;
    __device__ __forceinline__ RegStack2() : link(0), src(0), alo(0), ahi(0), blo(0), bhi(0) {}
    __device__ __forceinline__ void push(int sp, uint32_t l, uint32_t s, uint64_t ma, uint64_t mb) {
        asm volatile(
            "s_mov_b32 m0, %6\n\ts_nop 0\n\t"
            "v_writelane_b32 %0, %7, m0\n\tv_writelane_b32 %1, %8, m0\n\tv_writelane_b32 %2, %9, m0\n\tv_writelane_b32 %3, %10, m0\n\t"
            "v_writelane_b32 %4, %11, m0\n\tv_writelane_b32 %5, %12, m0"
            : "+v"(link), "+v"(src), "+v"(alo), "+v"(ahi), "+v"(blo), "+v"(bhi)
            : "s"(sp), "s"(l), "s"(s), "s"(static_cast<uint32_t>(ma)), "s"(static_cast<uint32_t>(ma >> 32)),
              "s"(static_cast<uint32_t>(mb)), "s"(static_cast<uint32_t>(mb >> 32))
            : "m0");
    }
    __device__ __forceinline__ void pop(int sp, uint32_t& l, uint32_t& s, uint64_t& ma, uint64_t& mb) const {
        l = static_cast<uint32_t>(__builtin_amdgcn_readlane(link, sp));
        s = static_cast<uint32_t>(__builtin_amdgcn_readlane(src, sp));
        ma = static_cast<uint32_t>(__builtin_amdgcn_readlane(alo, sp)) |
             (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(ahi, sp))) << 32);
        mb = static_cast<uint32_t>(__builtin_amdgcn_readlane(blo, sp)) |
             (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(bhi, sp))) << 32);
    }
};

template <int MODE, int OCT>
__device__ __forceinline__ void trace_packet2_impl(const DevScene& sc, const Ray& ra, const Ray& rb, bool active_a, bool active_b,
                                                   PacketHit& hit_a, PacketHit& hit_b) {
    constexpr bool PATCH_NAN = MODE == 2;
    kfp nodes = (kfp)(uintptr_t)(PATCH_NAN ? sc.nodes_lit : sc.nodes_aos);  // literal / wide tree, as in trace_packet_impl
    kfp tris = (kfp)(uintptr_t)sc.tris_aos;
    RegStack2 st;
    float best_a = FLT_MAX, ua = 0.0f, va = 0.0f, best_b = FLT_MAX, ub = 0.0f, vb = 0.0f;  // best (:34-37), per ray
    uint32_t prim_a = kNoPrim, prim_b = kNoPrim;
    st.push(0, PATCH_NAN ? sc.root_lit : sc.root, kSrcRoot, __ballot(active_a), __ballot(active_b));  // entry 0 = root (:28-32), never culled
    int sp = 1;
    int stale_top = 0;  // entries [0, stale_top) were pushed before some ray's best.t last changed
    while (sp > 0) {
        sp--;
        uint32_t link, src;
        uint64_t onm_a, onm_b;  // rays of each set this entry is still live for
        st.pop(sp, link, src, onm_a, onm_b);
        if (sp < stale_top) {  // :40-44, per ray
            stale_top = sp;
            kfp bx = nodes + static_cast<size_t>(src) * 8;
            const float b0 = bx[0], b1 = bx[1], b2 = bx[2], b3 = bx[3], b4 = bx[4], b5 = bx[5];
            onm_a &= ~mask_gt(slab_entry<PATCH_NAN, OCT>(b0, b1, b2, b3, b4, b5, ra), best_a);
            onm_b &= ~mask_gt(slab_entry<PATCH_NAN, OCT>(b0, b1, b2, b3, b4, b5, rb), best_b);
        }
        if ((onm_a | onm_b) == 0) continue;
        const bool on_a = __builtin_amdgcn_inverse_ballot_w64(onm_a), on_b = __builtin_amdgcn_inverse_ballot_w64(onm_b);
        float lim_a = on_a ? best_a : -1.0f, lim_b = on_b ? best_b : -1.0f;  // nothing passes for a disabled ray
        if ((link & 63u) == 0u) {
            // InnerNode::intersect :149-162, children ascending; record = {min.xyz, max.xyz, dlink, n}
            const uint32_t node = link >> 6;
            kfp nd = nodes + static_cast<size_t>(node) * 64;
            float a0 = nd[0], a1 = nd[1], a2 = nd[2], a3 = nd[3], a4 = nd[4], a5 = nd[5], a6 = nd[6];
            const uint32_t nchild = uniform_u(nd[7]);
            uint32_t slot = node * 8u;
            auto child = [&](const float b0, const float b1, const float b2, const float b3, const float b4, const float b5,
                             const float blink, const uint32_t cslot) {
                const uint32_t cl = uniform_u(blink);
                if (cl == MP_LINK_NULL) return;  // Null links are skipped at pop in the reference (:49)
                float t1a, t2a, t1b, t2b;
                slab<PATCH_NAN, OCT>(b0, b1, b2, b3, b4, b5, ra, lim_a, t1a, t2a);
                slab<PATCH_NAN, OCT>(b0, b1, b2, b3, b4, b5, rb, lim_b, t1b, t2b);
                const uint64_t ok_a = __ballot(t1a <= t2a), ok_b = __ballot(t1b <= t2b);
                if ((ok_a | ok_b) != 0) {
                    st.push(sp, cl, cslot, ok_a, ok_b);
                    sp++;
                }
            };
            for (uint32_t p = nchild >> 1; p > 0; p--) {
                const float b0 = nd[8], b1 = nd[9], b2 = nd[10], b3 = nd[11], b4 = nd[12], b5 = nd[13], b6 = nd[14];
                child(a0, a1, a2, a3, a4, a5, a6, slot);
                a0 = nd[16]; a1 = nd[17]; a2 = nd[18]; a3 = nd[19]; a4 = nd[20]; a5 = nd[21]; a6 = nd[22];
                child(b0, b1, b2, b3, b4, b5, b6, slot + 1u);
                slot += 2u;
                nd += 16;
            }
            if (nchild & 1u) child(a0, a1, a2, a3, a4, a5, a6, slot);
        } else {
            // intersect_triangles :104-140 for both rays of every lane
            const uint32_t first = link >> 6, n_real = link & 63u;
            kfp tp = tris + static_cast<size_t>(first) * (8 * kTriDwords);
            const float thr_a = on_a ? -kTiny : INFINITY, thr_b = on_b ? -kTiny : INFINITY;
            uint64_t changed = 0;
            auto test = [&](const float v0x, const float v0y, const float v0z, const float e1x, const float e1y, const float e1z,
                            const float e2x, const float e2y, const float e2z, const uint32_t tri) {
                // triangle.rs:183-217, ray A and ray B side by side (see trace_packet_impl for the early-out argument)
                const float hxa = fms(ra.dy, e2z, ra.dz * e2y), hya = fms(ra.dz, e2x, ra.dx * e2z), hza = fms(ra.dx, e2y, ra.dy * e2x);
                const float hxb = fms(rb.dy, e2z, rb.dz * e2y), hyb = fms(rb.dz, e2x, rb.dx * e2z), hzb = fms(rb.dx, e2y, rb.dy * e2x);
                const float det_a = fma_dot(e1x, e1y, e1z, hxa, hya, hza), det_b = fma_dot(e1x, e1y, e1z, hxb, hyb, hzb);
                const float sxa = ra.ox - v0x, sya = ra.oy - v0y, sza = ra.oz - v0z;
                const float sxb = rb.ox - v0x, syb = rb.oy - v0y, szb = rb.oz - v0z;
                const float un_a = fma_dot(sxa, sya, sza, hxa, hya, hza), un_b = fma_dot(sxb, syb, szb, hxb, hyb, hzb);
                const uint32_t sg_a = as_u(det_a) & 0x80000000u, sg_b = as_u(det_b) & 0x80000000u;
                const bool ok_a = fabsf(det_a) <= kHuge, ok_b = fabsf(det_b) <= kHuge;
                const float xua = ok_a ? as_f(as_u(un_a) ^ sg_a) : 1.0f, xub = ok_b ? as_f(as_u(un_b) ^ sg_b) : 1.0f;
                if ((__ballot(!(xua <= thr_a)) | __ballot(!(xub <= thr_b))) == 0) return;  // no live ray of either set can have u >= 0
                const float qxa = fms(sya, e1z, sza * e1y), qya = fms(sza, e1x, sxa * e1z), qza = fms(sxa, e1y, sya * e1x);
                const float qxb = fms(syb, e1z, szb * e1y), qyb = fms(szb, e1x, sxb * e1z), qzb = fms(sxb, e1y, syb * e1x);
                const float vn_a = fma_dot(ra.dx, ra.dy, ra.dz, qxa, qya, qza), vn_b = fma_dot(rb.dx, rb.dy, rb.dz, qxb, qyb, qzb);
                const float tn_a = fma_dot(e2x, e2y, e2z, qxa, qya, qza), tn_b = fma_dot(e2x, e2y, e2z, qxb, qyb, qzb);
                const float xva = ok_a ? as_f(as_u(vn_a) ^ sg_a) : 1.0f, xta = ok_a ? as_f(as_u(tn_a) ^ sg_a) : 1.0f;
                const float xvb = ok_b ? as_f(as_u(vn_b) ^ sg_b) : 1.0f, xtb = ok_b ? as_f(as_u(tn_b) ^ sg_b) : 1.0f;
                if ((__ballot(!(fminf(fminf(xua, xva), xta) <= thr_a)) | __ballot(!(fminf(fminf(xub, xvb), xtb) <= thr_b))) == 0) return;
                const float inv_a = 1.0f / det_a, inv_b = 1.0f / det_b;
                const float u_a = inv_a * un_a, v_a = inv_a * vn_a, t_a = inv_a * tn_a;
                const float u_b = inv_b * un_b, v_b = inv_b * vn_b, t_b = inv_b * tn_b;
                const bool acc_a = (u_a >= 0.0f) & (v_a >= 0.0f) & ((u_a + v_a) <= 1.0f) & (t_a >= 0.0f) & (t_a < lim_a);
                const bool acc_b = (u_b >= 0.0f) & (v_b >= 0.0f) & ((u_b + v_b) <= 1.0f) & (t_b >= 0.0f) & (t_b < lim_b);
                best_a = acc_a ? t_a : best_a; lim_a = acc_a ? t_a : lim_a; ua = acc_a ? u_a : ua; va = acc_a ? v_a : va; prim_a = acc_a ? tri : prim_a;
                best_b = acc_b ? t_b : best_b; lim_b = acc_b ? t_b : lim_b; ub = acc_b ? u_b : ub; vb = acc_b ? v_b : vb; prim_b = acc_b ? tri : prim_b;
                changed |= __ballot(acc_a) | __ballot(acc_b);
            };
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
            if (changed != 0) stale_top = sp;
        }
    }
    hit_a.t = best_a; hit_a.u = ua; hit_a.v = va; hit_a.prim = prim_a;
    hit_b.t = best_b; hit_b.u = ub; hit_b.v = vb; hit_b.prim = prim_b;
}

__device__ __forceinline__ void trace_packet2(const DevScene& sc, const Ray& ra, const Ray& rb, bool act_a, bool act_b, PacketHit& ha,
                                              PacketHit& hb) {
    const bool slow = (act_a && (fabsf(ra.ix) == INFINITY || fabsf(ra.iy) == INFINITY || fabsf(ra.iz) == INFINITY)) ||
                      (act_b && (fabsf(rb.ix) == INFINITY || fabsf(rb.iy) == INFINITY || fabsf(rb.iz) == INFINITY));
    if (__ballot(slow) != 0) {
        trace_packet2_impl<2, -1>(sc, ra, rb, act_a, act_b, ha, hb);
        return;
    }
    if (sc.boxes_ordered) {
        // wave-uniform octant over BOTH ray sets
        const uint64_t am = __ballot(act_a), bm = __ballot(act_b);
        const uint64_t nxa = __ballot(act_a && ra.ix < 0.0f), nya = __ballot(act_a && ra.iy < 0.0f), nza = __ballot(act_a && ra.iz < 0.0f);
        const uint64_t nxb = __ballot(act_b && rb.ix < 0.0f), nyb = __ballot(act_b && rb.iy < 0.0f), nzb = __ballot(act_b && rb.iz < 0.0f);
        const bool xn = (nxa | nxb) != 0, yn = (nya | nyb) != 0, zn = (nza | nzb) != 0;
        const bool xu = !xn || (nxa == am && nxb == bm), yu = !yn || (nya == am && nyb == bm), zu = !zn || (nza == am && nzb == bm);
        if (xu && yu && zu) {
            switch ((xn ? 1 : 0) | (yn ? 2 : 0) | (zn ? 4 : 0)) {
                case 0: trace_packet2_impl<1, 0>(sc, ra, rb, act_a, act_b, ha, hb); return;
                case 1: trace_packet2_impl<1, 1>(sc, ra, rb, act_a, act_b, ha, hb); return;
                case 2: trace_packet2_impl<1, 2>(sc, ra, rb, act_a, act_b, ha, hb); return;
                case 3: trace_packet2_impl<1, 3>(sc, ra, rb, act_a, act_b, ha, hb); return;
                case 4: trace_packet2_impl<1, 4>(sc, ra, rb, act_a, act_b, ha, hb); return;
                case 5: trace_packet2_impl<1, 5>(sc, ra, rb, act_a, act_b, ha, hb); return;
                case 6: trace_packet2_impl<1, 6>(sc, ra, rb, act_a, act_b, ha, hb); return;
                default: trace_packet2_impl<1, 7>(sc, ra, rb, act_a, act_b, ha, hb); return;
            }
        }
    }
    trace_packet2_impl<1, -1>(sc, ra, rb, act_a, act_b, ha, hb);
}

// pixel_sum += sample, strictly in sample order (worker.rs:41-43), for the S samples of a pixel held by S consecutive lanes.
// S = 16 is one DPP row: v_add_f32_dpp with row_newbcast:j adds lane j of the row in ONE instruction (no LDS permute); every
// lane of the row ends with the same sum.  Inactive samples contribute +0.0 (exact).
template <int J, int N>
struct RowSum {
    static __device__ __forceinline__ void run(float& acc, float c) {
        acc += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(c), 0x150 + J, 0xF, 0xF, false));
        RowSum<J + 1, N>::run(acc, c);
    }
};
template <int N>
struct RowSum<N, N> {
    static __device__ __forceinline__ void run(float&, float) {}
};
template <int S>
__device__ __forceinline__ void add_samples_in_order(float& acc, float c, int lane) {
    if (S == 1) {
        acc += c;
    } else if (S == 16) {
        RowSum<0, 16>::run(acc, c);
    } else if (S == 32) {
        // a pixel = two rows: every row adds its own 16 samples to the incoming sum (right for the even rows), row_bcast15 hands
        // the even rows' result to the odd rows, which add their 16 samples (the even rows redo theirs: discarded), and the
        // pixel's last lane holds the sum that all 32 lanes take over
        RowSum<0, 16>::run(acc, c);
        acc = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(acc), __float_as_int(acc), 0x142, 0xA, 0xF, false));
        RowSum<0, 16>::run(acc, c);
        const float lo = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 31));
        const float hi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 63));
        acc = lane < 32 ? lo : hi;
    } else {
#pragma unroll
        for (int j = 0; j < S; j++) acc += __shfl(c, (lane & ~(S - 1)) + j);
    }
}

// Fused tile render on ray packets.  A wave owns a block of 64/S pixels and shoots S consecutive samples of each
// pixel per pass (lane = pixel*S + sub-sample): all 64 rays of a pass are neighbours on the film, so the packet stays
// coherent, while the work unit (block x all samples) shrinks with S, which evens out the load.  pixel_sum is
// accumulated strictly in sample order (worker.rs:41-43), redundantly by every lane of the pixel (add_samples_in_order).
// WPE = waves per SIMD the register allocation is held to: 8 (64 VGPRs) hides the scalar-cache misses of scenes that
// outgrow it, 7 (72 VGPRs) schedules slightly better when the scene stays cache resident (profiles/r01_notes.md).
template <int S, bool LDS_STACK, int WPE, bool OBJ = false, bool MCACHE = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, 8))) void render_tiles_packet_kernel(RenderParams) {
    extern __shared__ __align__(16) unsigned char smem[];
    MP_KERNEL_PARAMS;
    constexpr int BW = (S <= 2) ? 8 : (S <= 8) ? 4 : (S <= 32) ? 2 : 1;  // pixel block = BW x BH, BW*BH*S == 64
    constexpr int BH = 64 / S / BW;
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int pix = lane / S, sub = lane % S;
    uint32_t qstate = blockIdx.x % kWorkQueues;
    // per-unit mask cache of the packet-level child rejection (MaskCache): this wave's header + entries in LDS
    MaskCache mc{nullptr};
    if (MCACHE) mc.lds = reinterpret_cast<uint32_t*>(smem) + static_cast<size_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6)) * kMaskCacheDwords;
    for (;;) {
        const RenderParams& P = params_view(KP);  // unit setup
        const uint32_t ts = P.tile_size;
        const uint32_t bx = (ts + BW - 1) / BW, by = (ts + BH - 1) / BH, upt = bx * by, total = P.n_tiles * upt;
        MP_NEXT_UNIT(unit)
        const uint32_t b = unit % upt;
        const uint32_t tile_i = P.tile_order ? P.tile_order[unit / upt] : unit / upt;
        const uint64_t t_unit = P.tile_cost ? __builtin_readcyclecounter() : 0;
        const mp_block T = P.tiles[tile_i];
        const uint32_t px = T.min_x + (b % bx) * BW + static_cast<uint32_t>(pix % BW);
        const uint32_t py = T.min_y + (b / bx) * BH + static_cast<uint32_t>(pix / BW);
        const bool inpix = px < T.max_x && py < T.max_y;
        if (__ballot(inpix) == 0) continue;
        const size_t off = (static_cast<size_t>(tile_i) * ts * ts + static_cast<size_t>(py - T.min_y) * ts + (px - T.min_x)) * 4;
        float acc, cnt;  // pixel_sum (r=g=b) and alpha (worker.rs:40)
        pixel_state_load(P, off, inpix, sub == 0, acc, cnt);
        // what the unit's passes share (kernels with a mask cache): whether they enter the walk without the per-ray scene pre-test
        // (mask_cache_unit_reaches), and the lane's sample key at sample 0, to which a pass adds its sample index (ray_math.h,
        // key_add_sample)
        bool pre_skip = false;
        uint64_t key0 = 0;
        if (MCACHE) {  // a new unit: other pixels, other bounds, set from the camera
            const RenderParams& C = params_view(KP);  // corner rays
            const uint32_t ux = T.min_x + (b % bx) * BW, uy = T.min_y + (b / bx) * BH;
            if (kKeyHoist) key0 = sample_key(C.gen, px, py, 0u);
            mask_cache_begin_unit(mc, C.gen.s, C.gen.jitter_scale, ux, min(ux + BW, T.max_x) - 1u, uy, min(uy + BH, T.max_y) - 1u);
            if (kUnitPretest && C.scene.has_pre) {
                pre_skip = mask_cache_unit_reaches(mc, C.scene.pre_min, C.scene.pre_max);
                if (pre_skip) MP_PROF_COUNT(8);
                else MP_PROF_COUNT(9);
            }
        }
        // passes are aligned to multiples of S in the absolute sample index, so that a chunk boundary (MP_FLAG_CHUNKED_SUM) never
        // falls inside a pass; lanes outside [s_begin, s_end) add +0.0, which is exact
        const uint32_t s_begin = P.s_begin, s_end = P.s_end;
        for (uint32_t s0 = s_begin & ~static_cast<uint32_t>(S - 1); s0 < s_end; s0 += S) {
            const uint32_t s = s0 + static_cast<uint32_t>(sub);
            const bool act = inpix && s >= s_begin && s < s_end;
            Ray r;
            r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
            {
                const RenderParams& G = params_view(KP);  // ray generation
                if (act) {
                    if (MCACHE && kKeyHoist) sample_ray_keyed(G.gen, px, py, rm::key_add_sample(key0, s), r);
                    else sample_ray(G.gen, px, py, s, r);
                }
            }
            PacketHit h;
            h.t = FLT_MAX; h.u = h.v = 0.0f; h.prim = kNoPrim;
            uint32_t hinst = 0u;
            {
                const RenderParams& W = params_view(KP);  // walk
                float* lds = reinterpret_cast<float*>(smem + static_cast<size_t>(static_cast<int>(threadIdx.x) >> 6) * W.lds_per_wave);
                if (OBJ) {  // object group: the packet walks every member's tree in turn
                    if (LDS_STACK) {
                        HybridStack st(lds, lane, W.scene.stack_cap, W.scene.packet_stack_regs);
                        trace_packet_objects<false>(W.scene, r, act, st, h, hinst);
                    } else {
                        RegStack st(lds, lane);
                        trace_packet_objects<(S >= 8 && S <= 32)>(W.scene, r, act, st, h, hinst);
                    }
                } else {
#ifdef MP_PROF_NOWALK  // profiling builds only (tools/build_variant.sh): what a pass costs without its walk
                    const bool go = false;
#else
                    const bool go = act && W.scene.kind == 0u && ((MCACHE && kUnitPretest && pre_skip) || may_hit_scene(W.scene, r));
#endif
                    if (__ballot(go) != 0) {
                        if (LDS_STACK) {
                            HybridStack st(lds, lane, W.scene.stack_cap, W.scene.packet_stack_regs);
                            trace_packet<false>(W.scene, r, go, st, h);
                        } else {
                            RegStack st(lds, lane);
                            trace_packet<((S >= 8 && S <= 32) || MCACHE), RegStack, MCACHE>(W.scene, r, go, st, h, mc);
                        }
                    }
                }
            }
            float c = 0.0f;
            bool hit = h.prim != kNoPrim;
            const RenderParams& H = params_view(KP);  // shading + accumulation
            if (hit) {
#ifdef MP_PROF_NOSHADE  // profiling builds only
                c = h.u;
#else
                float nn[3];
                if (OBJ) object_normal(H.scene, hinst, r, h.prim, h.u, h.v, nn);
                else if (MCACHE && kShortNormal) resolve_normal_short(H.scene, h.prim, h.u, h.v, nn);
                else resolve_normal(H.scene, h.prim, h.u, h.v, nn);
                c = fabsf(r.dx * nn[0] + r.dy * nn[1] + r.dz * nn[2]);  // worker.rs:60
#endif
            } else if (H.scene.kind == 1u) {  // Scene<Sphere>
                float ts_, nn[3];
                hit = act && sphere_intersect(H.scene, r, ts_, nn);
                if (hit) c = fabsf(r.dx * nn[0] + r.dy * nn[1] + r.dz * nn[2]);
            }
            // alpha sums 1.0 per hit: an exact integer in f32, so the order is irrelevant
            {   // (the mask of this pixel's lanes is rebuilt from the lane id here: two registers less across the walk)
                int l_ = lane;
                asm volatile("" : "+v"(l_));
                const uint64_t pixel_lanes = (S == 64 ? ~0ull : ((1ull << (S & 63)) - 1ull)) << (l_ & ~(S - 1));
                cnt += static_cast<float>(__popcll(__ballot(hit) & pixel_lanes));
            }
            add_samples_in_order<S>(acc, c, lane);  // misses add +0.0 (exact)
            if (H.chunked && ((s0 + S) & (kSumChunk - 1u)) == 0u && s0 + S <= s_end) chunk_flush(H, off, inpix && sub == 0, acc);
        }
        const RenderParams& E = params_view(KP);  // unit end
        if (inpix && sub == 0) pixel_state_store(E, off, acc, cnt);
        if (E.tile_cost && lane == 0) atomicAdd(E.tile_cost + tile_i, static_cast<unsigned long long>(__builtin_readcyclecounter() - t_unit));
    }
}

// Fused tile render on 128-ray packets (two rays per lane, trace_packet2).  A wave owns a 4x2 block of pixels and shoots 16
// consecutive samples of each pixel per pass: lane = (pixel of the left 2x2 half) * 16 + sub-sample carries that sample of its
// pixel (ray A) and of the pixel two columns to the right (ray B).  Reference semantics only (the path kernel has its own loop);
// TriangleBvh scenes whose stack bound fits the register stack.
template <int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, 8))) void render_tiles_packet2_kernel(RenderParams P) {
    constexpr int S = 16;
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int pix = lane / S, sub = lane % S;
    const uint64_t pixel_lanes = ((1ull << S) - 1ull) << (lane & ~(S - 1));
    const uint32_t ts = P.tile_size;
    const uint32_t bx = (ts + 3) / 4, by = (ts + 1) / 2, upt = bx * by, total = P.n_tiles * upt;
    uint32_t qstate = blockIdx.x % kWorkQueues;
    for (;;) {
        MP_NEXT_UNIT(unit)
        const uint32_t b = unit % upt;
        const uint32_t tile_i = P.tile_order ? P.tile_order[unit / upt] : unit / upt;
        const uint64_t t_unit = P.tile_cost ? __builtin_readcyclecounter() : 0;
        const mp_block T = P.tiles[tile_i];
        const uint32_t px_a = T.min_x + (b % bx) * 4 + static_cast<uint32_t>(pix % 2), px_b = px_a + 2u;
        const uint32_t py = T.min_y + (b / bx) * 2 + static_cast<uint32_t>(pix / 2);
        const bool in_a = px_a < T.max_x && py < T.max_y, in_b = px_b < T.max_x && py < T.max_y;
        if (__ballot(in_a) == 0) continue;  // B lies to the right of A: no A pixel, no B pixel
        const size_t off_a = (static_cast<size_t>(tile_i) * ts * ts + static_cast<size_t>(py - T.min_y) * ts + (px_a - T.min_x)) * 4;
        const size_t off_b = off_a + 8;
        float acc_a, cnt_a, acc_b, cnt_b;  // pixel_sum (r=g=b) and alpha (worker.rs:40)
        pixel_state_load(P, off_a, in_a, sub == 0, acc_a, cnt_a);
        pixel_state_load(P, off_b, in_b, sub == 0, acc_b, cnt_b);
        for (uint32_t s0 = P.s_begin & ~static_cast<uint32_t>(S - 1); s0 < P.s_end; s0 += S) {
            const uint32_t s = s0 + static_cast<uint32_t>(sub);
            const bool in_pass = s >= P.s_begin && s < P.s_end;
            const bool act_a = in_a && in_pass, act_b = in_b && in_pass;
            Ray ra, rb;
            ra.ox = ra.oy = ra.oz = ra.dx = ra.dy = ra.dz = ra.ix = ra.iy = ra.iz = 0.0f;
            rb = ra;
            if (act_a) sample_ray(P.gen, px_a, py, s, ra);
            if (act_b) sample_ray(P.gen, px_b, py, s, rb);
            const bool go_a = act_a && may_hit_scene(P.scene, ra), go_b = act_b && may_hit_scene(P.scene, rb);
            PacketHit ha, hb;
            ha.t = FLT_MAX; ha.u = ha.v = 0.0f; ha.prim = kNoPrim;
            hb = ha;
            if ((__ballot(go_a) | __ballot(go_b)) != 0) trace_packet2(P.scene, ra, rb, go_a, go_b, ha, hb);
            float c_a = 0.0f, c_b = 0.0f;
            const bool hit_a = ha.prim != kNoPrim, hit_b = hb.prim != kNoPrim;
            if (hit_a) {
                float nn[3];
                resolve_normal(P.scene, ha.prim, ha.u, ha.v, nn);
                c_a = fabsf(ra.dx * nn[0] + ra.dy * nn[1] + ra.dz * nn[2]);  // worker.rs:60
            }
            if (hit_b) {
                float nn[3];
                resolve_normal(P.scene, hb.prim, hb.u, hb.v, nn);
                c_b = fabsf(rb.dx * nn[0] + rb.dy * nn[1] + rb.dz * nn[2]);
            }
            cnt_a += static_cast<float>(__popcll(__ballot(hit_a) & pixel_lanes));
            cnt_b += static_cast<float>(__popcll(__ballot(hit_b) & pixel_lanes));
            add_samples_in_order<S>(acc_a, c_a, lane);  // misses add +0.0 (exact)
            add_samples_in_order<S>(acc_b, c_b, lane);
            if (P.chunked && ((s0 + S) & (kSumChunk - 1u)) == 0u && s0 + S <= P.s_end) {
                chunk_flush(P, off_a, in_a && sub == 0, acc_a);
                chunk_flush(P, off_b, in_b && sub == 0, acc_b);
            }
        }
        if (sub == 0) {
            if (in_a) pixel_state_store(P, off_a, acc_a, cnt_a);
            if (in_b) pixel_state_store(P, off_b, acc_b, cnt_b);
        }
        if (P.tile_cost && lane == 0) atomicAdd(P.tile_cost + tile_i, static_cast<unsigned long long>(__builtin_readcyclecounter() - t_unit));
    }
}

// ---- build-defined path extension (MP_FLAG_PATHS; the reference has no bounce loop) -----------------
// Diffuse grey surfaces {albedo, emission} indexed by TriangleShadingData.material under a uniform sky (defaults: one material
// {0.75, 0}, sky 1), at most max_depth segments per path; the operations and their order are those of the oracle's
// render_sample_paths_impl (only + - * / sqrt and compares => bit-identical).
// Camera rays are coherent and go through the packet walk; bounce rays are incoherent: the lanes whose path is still
// alive are compacted (ballot + mbcnt) into the wave's LDS ray queue and traced by the 8-lane-group traversal.
constexpr float kPathEps = 1e-4f;

// HitRecord.texture_coords (geometry/mod.rs:78-79; BarycentricCoordinates::interpolate at ray_bvh_intersection.rs:80-83), x and y
__device__ __forceinline__ void hit_tex(const DevScene& so, uint32_t prim, float u, float v, float& tx, float& ty) {
    const uint32_t* vi = so.vidx + static_cast<size_t>(prim) * 3;
    const float *t0 = so.vtex + 3 * static_cast<size_t>(vi[0]), *t1 = so.vtex + 3 * static_cast<size_t>(vi[1]),
                *t2 = so.vtex + 3 * static_cast<size_t>(vi[2]);
    const float w = 1.0f - u - v;
    tx = t0[0] * w + t1[0] * u + t2[0] * v;
    ty = t0[1] * w + t1[1] * u + t2[1] * v;
}

// One path vertex of the build-defined extension (oracle: render_sample_paths_impl), shared by the fused and the staged kernels so
// that both evaluate the very same operations: `h` is the closest hit of segment `depth` along `r`.  Updates L / thr, and either
// ends the path (returns false) or replaces `r` by the bounce ray drawn from `rng` (returns true).
// N = colour channels carried: 3 when some material of the table is coloured or textured (DevScene::materials_rgb), else 1 -- a grey
// table makes the three channels the same number, so one is computed (same bits).  Material record = mp_material: albedo rgb,
// emission rgb, albedo2 rgb, texture, texture_scale.
template <bool OBJ, int N>
__device__ __forceinline__ bool path_vertex(const DevScene& sc, const PacketHit& h, uint32_t depth, uint32_t max_depth, Rng& rng,
                                            Ray& r, float (&L)[N], float (&thr)[N], bool& primary_hit, uint32_t inst = 0u) {
    if (h.prim == kNoPrim) {
#pragma unroll
        for (int c = 0; c < N; c++) L[c] = L[c] + thr[c] * sc.sky;
        return false;
    }
    if (depth == 1) primary_hit = true;
    float n[3];
    const uint32_t mat = OBJ ? object_normal(sc, inst, r, h.prim, h.u, h.v, n) : resolve_normal(sc, h.prim, h.u, h.v, n);
    const float* m = sc.materials + static_cast<size_t>(mat) * 12;
#pragma unroll
    for (int c = 0; c < N; c++) L[c] = L[c] + thr[c] * m[3 + c];
    const float dn = r.dx * n[0] + r.dy * n[1] + r.dz * n[2];
    if (dn > 0.0f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
    const float* alb = m;
    if (N == 3 && as_u(m[9]) == MP_TEXTURE_CHECKER) {  // reads HitRecord.texture_coords; a Sphere member's are the origin (primitives.rs:45)
        float tx = 0.0f, ty = 0.0f;
        if (OBJ) {
            DevScene so;
            object_scene(sc, inst, so);
            if (so.kind == 0u) hit_tex(so, h.prim, h.u, h.v, tx, ty);
        } else {
            hit_tex(sc, h.prim, h.u, h.v, tx, ty);
        }
        const float cell = floorf(tx * m[10]) + floorf(ty * m[10]);
        const float half = cell * 0.5f;
        if (half - floorf(half) != 0.0f) alb = m + 6;  // odd cell (NaN counts as odd): albedo2
    }
#pragma unroll
    for (int c = 0; c < N; c++) thr[c] = thr[c] * alb[c];
    if (depth == max_depth) return false;
    const float hx = r.ox + r.dx * h.t, hy = r.oy + r.dy * h.t, hz = r.oz + r.dz * h.t;  // geometry/mod.rs:56-58
    float x1, x2;
    unit_disc(rng, x1, x2);
    const float z = sqrtf(1.0f - (x1 * x1 + x2 * x2));
    const float sign = copysignf(1.0f, n[2]);
    const float a = -1.0f / (sign + n[2]);
    const float bb = n[0] * n[1] * a;
    const float t0 = 1.0f + sign * n[0] * n[0] * a, t1 = sign * bb, t2 = -sign * n[0];
    const float b0 = bb, b1 = sign + n[1] * n[1] * a, b2 = -n[1];
    ray_new(hx + n[0] * kPathEps, hy + n[1] * kPathEps, hz + n[2] * kPathEps, t0 * x1 + b0 * x2 + n[0] * z,
            t1 * x1 + b1 * x2 + n[1] * z, t2 * x1 + b2 * x2 + n[2] * z, r);
    return true;
}

// worker.rs:40-44 for three colour channels (coloured / textured material tables; never with MP_FLAG_CHUNKED_SUM): the slot holds
// {sum r, sum g, sum b, hit count} between MP_FLAG_ACCUMULATE launches
__device__ __forceinline__ void pixel_state_load3(const RenderParams& P, size_t off, bool inpix, float (&acc)[3], float& cnt) {
    acc[0] = acc[1] = acc[2] = 0.0f;
    cnt = 0.0f;
    if (P.carry_in && inpix) {
        const float4 prev = *reinterpret_cast<const float4*>(P.out + off);
        acc[0] = prev.x; acc[1] = prev.y; acc[2] = prev.z;
        cnt = prev.w;
    }
}
__device__ __forceinline__ void pixel_state_store3(const RenderParams& P, size_t off, const float (&acc)[3], float cnt) {
    const float s = P.finalize ? P.inv_spp : 1.0f;  // worker.rs:44 ; x * 1.0f is x
    *reinterpret_cast<float4*>(P.out + off) = make_float4(acc[0] * s, acc[1] * s, acc[2] * s, cnt * s);
}

// ---- build-defined first-hit feature planes (mp_render_aov_device / mp_render_aov_pass_device, include/minipath_hip.h) --------
struct AovParams {
    RenderParams r;   // r.out is not used; r.s_begin / s_end / carry_in / finalize as in the render kernels
    float* shade;     // {c, c, c, alpha}
    float* normal;    // {n.x, n.y, n.z, t}
    float* albedo;    // {r, g, b, alpha}
    uint32_t* ids;    // {prim, instance, material, hit} of sample 0
    float* position;  // {p.x, p.y, p.z, alpha}
    float* shade_sq;  // {c * c, c * c, c * c, alpha}
    uint32_t park_pixel;  // bytes of parked sums per pixel: 32, or 48 when position or shade_sq is asked for (LaunchPlan::park_pixel)
};

// Reflectance of a hit: the factor path_vertex multiplies the throughput by (mp_material.albedo, or albedo2 on the odd cells of a
// MP_TEXTURE_CHECKER material; NaN cells count as odd; a Sphere's texture coordinates are the origin).  RESTATED from path_vertex,
// not shared with it: path_vertex's instantiations stay exactly as measured, and tests/test_gpu_aov.py holds the two rules together
// (its checker case compares this kernel with a model of path_vertex's rule).  A scene without a material table (Scene<Sphere>)
// has the default material.
template <bool OBJ>
__device__ __forceinline__ void hit_albedo(const DevScene& sc, uint32_t inst, uint32_t mat, uint32_t prim, float u, float v, float (&a)[3]) {
    if (sc.materials == nullptr) { a[0] = a[1] = a[2] = 0.75f; return; }
    const float* m = sc.materials + static_cast<size_t>(mat) * 12;
    const float* alb = m;
    if (as_u(m[9]) == MP_TEXTURE_CHECKER) {
        float tx = 0.0f, ty = 0.0f;
        if (OBJ) {
            DevScene so;
            object_scene(sc, inst, so);
            if (so.kind == 0u) hit_tex(so, prim, u, v, tx, ty);
        } else {
            hit_tex(sc, prim, u, v, tx, ty);
        }
        const float cell = floorf(tx * m[10]) + floorf(ty * m[10]);
        const float half = cell * 0.5f;
        if (half - floorf(half) != 0.0f) alb = m + 6;
    }
    a[0] = alb[0]; a[1] = alb[1]; a[2] = alb[2];
}

// The packet render with up to six planes per pixel.  Work units, queues, ray generation, pre-test and walk are those of
// render_tiles_packet_kernel (called, not copied); new is what follows the walk: normal, material and texture cell per lane, then
// up to twelve channels through add_samples_in_order and the id record of the lane that holds sample 0.
// Registers: the running sums of a pixel do NOT live across the walk.  Every lane of a pixel ends a pass with the same sums,
// so the pixel's first lane parks them in LDS (8 or 12 dwords per pixel, 64/S pixels per wave: 32 B .. 3 KB per wave, in front of
// the mask cache / the LDS stack) and every lane of the pixel reads them back (a broadcast read) for the adds of the next pass; only
// the hit count stays in a register, as in the render kernel.  Planes the caller did not ask for are skipped by wave-uniform
// branches on the plane pointers (scalar loads from the kernel arguments): a compile-time plane mask would multiply the
// instantiations by up to 15 for the price of a few s_cbranch per pass.  The point and the squared shade (d_position, d_shade_sq)
// are four more channels in a third float4 of the park, which then takes 48 bytes per pixel instead of 32: the park's stride is a
// wave-uniform kernel argument (park_pixel), so a launch without the two planes keeps the LDS size and the park traffic it had.
// Passes (MP_FLAG_ACCUMULATE through mp_render_aov_pass_device): the launch adds samples [s_begin, s_end).  With carry_in the
// pixel's first lane starts the park from the sums the planes hold ({sum, sum, sum, hits}; d_normal {sum n, sum t}) instead of
// zeros; without finalize the unit's end stores the sums unscaled (x * 1.0f is x).  Any split of [0, spp) into passes gives the bits
// of the single launch -- the render kernels' argument (render_tiles_packet_kernel): passes are aligned to multiples of S in the
// absolute sample index, so sample s sits in the same lane of its pixel whatever the split, and the lanes of a boundary pass that
// lie outside [s_begin, s_end) are inactive and add +0.0.  A running sum that starts at +0.0 is never -0.0 (x + y is -0.0 only
// when both are), so x + (+0.0) is x bit for bit, and the adds of the samples themselves happen in the same order on the same
// values as in one launch.  The hit count is an exact integer in f32.  The id record is stored by the lane that holds sample 0
// only when that lane is active: a pass that begins at sample 1 .. S-1 starts at the aligned index 0 too.
template <int S, bool LDS_STACK, int WPE, bool OBJ = false, bool MCACHE = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, 8))) void render_aov_packet_kernel(AovParams) {
    extern __shared__ __align__(16) unsigned char smem[];
    typedef const __attribute__((address_space(4))) AovParams* kaov_t;
    kaov_t KP = (kaov_t)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr int BW = (S <= 2) ? 8 : (S <= 8) ? 4 : (S <= 32) ? 2 : 1;  // pixel block = BW x BH, BW*BH*S == 64
    constexpr int BH = 64 / S / BW;
    constexpr uint32_t kParkPixels = 64 / S;  // parked pixels per wave, park_pixel bytes each
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int pix = lane / S, sub = lane % S;
    uint32_t qstate = blockIdx.x % kWorkQueues;
    MaskCache mc{nullptr};
    if (MCACHE) mc.lds = reinterpret_cast<uint32_t*>(smem + 4 * kParkPixels * kernarg_view<AovParams>(KP).park_pixel) + static_cast<size_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6)) * kMaskCacheDwords;
    for (;;) {
        const RenderParams& P = kernarg_view<AovParams>(KP).r;  // unit setup
        const uint32_t ts = P.tile_size;
        const uint32_t bx = (ts + BW - 1) / BW, by = (ts + BH - 1) / BH, upt = bx * by, total = P.n_tiles * upt;
        MP_NEXT_UNIT(unit)
        const uint32_t b = unit % upt;
        const uint32_t tile_i = P.tile_order ? P.tile_order[unit / upt] : unit / upt;
        const uint64_t t_unit = P.tile_cost ? __builtin_readcyclecounter() : 0;
        const mp_block T = P.tiles[tile_i];
        const uint32_t px = T.min_x + (b % bx) * BW + static_cast<uint32_t>(pix % BW);
        const uint32_t py = T.min_y + (b / bx) * BH + static_cast<uint32_t>(pix / BW);
        const bool inpix = px < T.max_x && py < T.max_y;
        if (__ballot(inpix) == 0) continue;
        const size_t off = (static_cast<size_t>(tile_i) * ts * ts + static_cast<size_t>(py - T.min_y) * ts + (px - T.min_x)) * 4;
        float cnt = 0.0f;  // alpha (worker.rs:40); the pixel's first lane is the one that stores it
        uint64_t key0 = 0;  // (kernels with a mask cache) the lane's sample key at sample 0, as in render_tiles_packet_kernel
        {
            const AovParams& U = kernarg_view<AovParams>(KP);  // unit start: zeros, or the sums of the earlier passes
            float4* park = reinterpret_cast<float4*>(smem + (static_cast<size_t>(static_cast<int>(threadIdx.x) >> 6) * kParkPixels + pix) * U.park_pixel);
            if (sub == 0) {
                float4 a0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), a1 = a0, a2 = a0;
                if (U.r.carry_in && inpix) {  // the count: from the first of shade, albedo, position, shade_sq that is there
                    if (U.shade_sq) { const float4 v = *reinterpret_cast<const float4*>(U.shade_sq + off); a2.w = v.x; cnt = v.w; }
                    if (U.position) { const float4 v = *reinterpret_cast<const float4*>(U.position + off); a2.x = v.x; a2.y = v.y; a2.z = v.z; cnt = v.w; }
                    if (U.albedo) { const float4 v = *reinterpret_cast<const float4*>(U.albedo + off); a1.y = v.x; a1.z = v.y; a1.w = v.z; cnt = v.w; }
                    if (U.normal) { const float4 v = *reinterpret_cast<const float4*>(U.normal + off); a0.y = v.x; a0.z = v.y; a0.w = v.z; a1.x = v.w; }
                    if (U.shade) { const float4 v = *reinterpret_cast<const float4*>(U.shade + off); a0.x = v.x; cnt = v.w; }
                }
                park[0] = a0; park[1] = a1;
                if (U.park_pixel > 32u) park[2] = a2;
            }
            if (MCACHE && lane == 0) mc.lds[kHdrState] = 0xFFFFFFFFu;  // a new unit: other pixels, other bounds
            if (MCACHE && kKeyHoist) key0 = sample_key(U.r.gen, px, py, 0u);
            wave_lds_sync();
        }
        const uint32_t s_end = P.s_end;
        // passes are aligned to multiples of S in the absolute sample index; lanes outside [s_begin, s_end) add +0.0, which is exact
        for (uint32_t s0 = P.s_begin & ~static_cast<uint32_t>(S - 1); s0 < s_end; s0 += S) {
            const uint32_t s = s0 + static_cast<uint32_t>(sub);
            bool act;
            Ray r;
            r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
            {
                const RenderParams& G = kernarg_view<AovParams>(KP).r;  // ray generation
                act = inpix && s >= G.s_begin && s < s_end;
                if (act) {
                    if (MCACHE && kKeyHoist) sample_ray_keyed(G.gen, px, py, rm::key_add_sample(key0, s), r);
                    else sample_ray(G.gen, px, py, s, r);
                }
            }
            PacketHit h;
            h.t = FLT_MAX; h.u = h.v = 0.0f; h.prim = kNoPrim;
            uint32_t hinst = 0u;
            {
                const AovParams& WA = kernarg_view<AovParams>(KP);  // walk
                const RenderParams& W = WA.r;
                float* lds = reinterpret_cast<float*>(smem + 4 * kParkPixels * WA.park_pixel + static_cast<size_t>(static_cast<int>(threadIdx.x) >> 6) * W.lds_per_wave);
                if (OBJ) {
                    if (LDS_STACK) {
                        HybridStack st(lds, lane, W.scene.stack_cap, W.scene.packet_stack_regs);
                        trace_packet_objects<false>(W.scene, r, act, st, h, hinst);
                    } else {
                        RegStack st(lds, lane);
                        trace_packet_objects<(S == 16)>(W.scene, r, act, st, h, hinst);
                    }
                } else {
                    const bool go = act && W.scene.kind == 0u && may_hit_scene(W.scene, r);
                    if (__ballot(go) != 0) {
                        if (LDS_STACK) {
                            HybridStack st(lds, lane, W.scene.stack_cap, W.scene.packet_stack_regs);
                            trace_packet<false>(W.scene, r, go, st, h);
                        } else {
                            RegStack st(lds, lane);
                            trace_packet<(S == 16 || MCACHE), RegStack, MCACHE>(W.scene, r, go, st, h, mc);
                        }
                    }
                }
            }
            const AovParams& H = kernarg_view<AovParams>(KP);  // hit record + accumulation
            bool hit = h.prim != kNoPrim;
            float nn[3] = {0.0f, 0.0f, 0.0f};
            uint32_t mat = 0u;
            if (hit) {
                mat = OBJ ? object_normal(H.r.scene, hinst, r, h.prim, h.u, h.v, nn)
                    : (MCACHE && kShortNormal) ? resolve_normal_short(H.r.scene, h.prim, h.u, h.v, nn)
                                               : resolve_normal(H.r.scene, h.prim, h.u, h.v, nn);
            } else if (H.r.scene.kind == 1u) {  // Scene<Sphere>: prim 0, material 0 (primitives.rs:40-46)
                hit = act && sphere_intersect(H.r.scene, r, h.t, nn);
                if (hit) h.prim = 0u;
            }
            if (H.ids && act && s == 0u)  // not averaged: the record of sample 0, written by the pass that holds it
                *reinterpret_cast<uint4*>(H.ids + off) = hit ? make_uint4(h.prim, hinst, mat, 1u) : make_uint4(kNoPrim, 0u, 0u, 0u);
            int l_ = lane;  // (pixel mask and park address rebuilt from the lane id here: nothing of them lives across the walk)
            asm volatile("" : "+v"(l_));
            const uint64_t pixel_lanes = (S == 64 ? ~0ull : ((1ull << (S & 63)) - 1ull)) << (l_ & ~(S - 1));
            cnt += static_cast<float>(__popcll(__ballot(hit) & pixel_lanes));  // exact integers: the order is irrelevant
            float4* park = reinterpret_cast<float4*>(smem + (static_cast<size_t>(static_cast<int>(threadIdx.x) >> 6) * kParkPixels + (l_ / S)) * H.park_pixel);
            float4 a0 = park[0], a1 = park[1];  // {shade, n.x, n.y, n.z}, {t, r, g, b}
            // misses add +0.0 (exact)
            float c = 0.0f;  // worker.rs:60, once for d_shade and d_shade_sq
            if (H.shade || H.shade_sq) c = hit ? fabsf(r.dx * nn[0] + r.dy * nn[1] + r.dz * nn[2]) : 0.0f;
            if (H.shade) add_samples_in_order<S>(a0.x, c, lane);
            if (H.normal) {
                add_samples_in_order<S>(a0.y, hit ? nn[0] : 0.0f, lane);
                add_samples_in_order<S>(a0.z, hit ? nn[1] : 0.0f, lane);
                add_samples_in_order<S>(a0.w, hit ? nn[2] : 0.0f, lane);
                add_samples_in_order<S>(a1.x, hit ? h.t : 0.0f, lane);
            }
            if (H.albedo) {
                float al[3] = {0.0f, 0.0f, 0.0f};
                if (hit) hit_albedo<OBJ>(H.r.scene, hinst, mat, h.prim, h.u, h.v, al);
                add_samples_in_order<S>(a1.y, al[0], lane);
                add_samples_in_order<S>(a1.z, al[1], lane);
                add_samples_in_order<S>(a1.w, al[2], lane);
            }
            float4 a2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // {p.x, p.y, p.z, c * c}
            if (H.park_pixel > 32u) {
                a2 = park[2];
                if (H.position) {  // HitRecord.point = point_at(t) of the world ray (geometry/mod.rs:56-58), as mp_trace_rays stores it
                    add_samples_in_order<S>(a2.x, hit ? r.ox + r.dx * h.t : 0.0f, lane);
                    add_samples_in_order<S>(a2.y, hit ? r.oy + r.dy * h.t : 0.0f, lane);
                    add_samples_in_order<S>(a2.z, hit ? r.oz + r.dz * h.t : 0.0f, lane);
                }
                if (H.shade_sq) add_samples_in_order<S>(a2.w, c * c, lane);  // one rounded product (no contraction); a miss: +0.0 * +0.0
            }
            wave_lds_sync();  // every lane of the pixel has read the old sums
            if ((l_ & (S - 1)) == 0) {
                park[0] = a0; park[1] = a1;
                if (H.park_pixel > 32u) park[2] = a2;
            }
            wave_lds_sync();
        }
        const AovParams& E = kernarg_view<AovParams>(KP);  // unit end: pixel = sum * inv_spp (worker.rs:44), or the sums as they are
        if (inpix && sub == 0) {
            const float4* park = reinterpret_cast<const float4*>(smem + (static_cast<size_t>(static_cast<int>(threadIdx.x) >> 6) * kParkPixels + pix) * E.park_pixel);
            const float4 a0 = park[0], a1 = park[1];
            const float inv = E.r.finalize ? E.r.inv_spp : 1.0f, a = cnt * inv;  // x * 1.0f is x
            if (E.shade) { const float m = a0.x * inv; *reinterpret_cast<float4*>(E.shade + off) = make_float4(m, m, m, a); }
            if (E.normal) *reinterpret_cast<float4*>(E.normal + off) = make_float4(a0.y * inv, a0.z * inv, a0.w * inv, a1.x * inv);
            if (E.albedo) *reinterpret_cast<float4*>(E.albedo + off) = make_float4(a1.y * inv, a1.z * inv, a1.w * inv, a);
            if (E.park_pixel > 32u) {
                const float4 a2 = park[2];
                if (E.position) *reinterpret_cast<float4*>(E.position + off) = make_float4(a2.x * inv, a2.y * inv, a2.z * inv, a);
                if (E.shade_sq) { const float m = a2.w * inv; *reinterpret_cast<float4*>(E.shade_sq + off) = make_float4(m, m, m, a); }
            }
        }
        if (E.r.tile_cost && lane == 0) atomicAdd(E.r.tile_cost + tile_i, static_cast<unsigned long long>(__builtin_readcyclecounter() - t_unit));
    }
}

#ifndef MP_PATHS_WPE
#define MP_PATHS_WPE 6  // waves per SIMD the path kernel's registers are held to (A/B-measured, profiles/r03_notes.md)
#endif
// MCACHE: the camera pass runs the cached packet walk (MaskCache; the wave's header + tables are the last kMaskCacheDwords dwords of
// its LDS region)
template <int S, bool OBJ, bool RGB, bool MCACHE = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MP_PATHS_WPE, 8))) void render_paths_kernel(RenderParams) {
    constexpr int N = RGB ? 3 : 1;
    extern __shared__ __align__(16) unsigned char smem[];
    MP_KERNEL_PARAMS;  // RenderParams through short-lived views (params_view)
    MaskCache mc{nullptr};
    if (MCACHE) {
        const RenderParams& P0 = params_view(KP);
        mc.lds = reinterpret_cast<uint32_t*>(smem + static_cast<size_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6) + 1) * P0.lds_per_wave) - kMaskCacheDwords;
    }
    constexpr int BW = (S <= 2) ? 8 : (S <= 8) ? 4 : 2;
    constexpr int BH = 64 / S / BW;
    const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
    const int pix = lane / S, sub = lane % S;
    unsigned long long segs = 0;  // wave-uniform
    uint32_t qstate = blockIdx.x % kWorkQueues;
    for (;;) {
        const RenderParams& P = params_view(KP);  // unit setup
        const uint32_t ts = P.tile_size;
        const uint32_t bx = (ts + BW - 1) / BW, by = (ts + BH - 1) / BH, upt = bx * by, total = P.n_tiles * upt;
        MP_NEXT_UNIT(unit)
        const uint32_t b = unit % upt;
        const uint32_t tile_i = P.tile_order ? P.tile_order[unit / upt] : unit / upt;
        const uint64_t t_unit = P.tile_cost ? __builtin_readcyclecounter() : 0;
        const mp_block T = P.tiles[tile_i];
        const uint32_t px = T.min_x + (b % bx) * BW + static_cast<uint32_t>(pix % BW);
        const uint32_t py = T.min_y + (b / bx) * BH + static_cast<uint32_t>(pix / BW);
        const bool inpix = px < T.max_x && py < T.max_y;
        if (__ballot(inpix) == 0) continue;
        const size_t off = (static_cast<size_t>(tile_i) * ts * ts + static_cast<size_t>(py - T.min_y) * ts + (px - T.min_x)) * 4;
        float acc[N], cnt;  // pixel_sum (r=g=b for a grey table: one channel) and alpha (worker.rs:40)
        if (RGB) pixel_state_load3(P, off, inpix, reinterpret_cast<float (&)[3]>(acc[0]), cnt);
        else pixel_state_load(P, off, inpix, sub == 0, acc[0], cnt);
        if (MCACHE) {  // a new unit: other pixels, other bounds
            if (lane == 0) mc.lds[kHdrState] = 0xFFFFFFFFu;
            wave_lds_sync();
        }
        // passes are aligned to multiples of S in the absolute sample index, so that a chunk boundary (MP_FLAG_CHUNKED_SUM) never
        // falls inside a pass; lanes outside [s_begin, s_end) add +0.0, which is exact
        const uint32_t s_begin = P.s_begin, s_end = P.s_end, max_depth = P.max_depth;
        for (uint32_t s0 = s_begin & ~static_cast<uint32_t>(S - 1); s0 < s_end; s0 += S) {
            const uint32_t s = s0 + static_cast<uint32_t>(sub);
            const bool act = inpix && s >= s_begin && s < s_end;
            Rng rng;
            rng_zero(rng);
            Ray r;
            r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
            {
                const RenderParams& G = params_view(KP);  // ray generation
                if (act) {
                    rng_seed(rng, sample_key(G.gen, px, py, s));
                    sample_ray_rng(G.gen, px, py, rng, r);
                }
            }
            float L[N], thr[N];
#pragma unroll
            for (int c = 0; c < N; c++) { L[c] = 0.0f; thr[c] = 1.0f; }
            bool alive = act, primary_hit = false;
            PacketHit h;
            for (uint32_t depth = 1; depth <= max_depth; depth++) {
                const uint64_t alive_m = __ballot(alive);
                if (alive_m == 0) break;
                segs += static_cast<unsigned long long>(__popcll(alive_m));
                h.t = FLT_MAX; h.u = h.v = 0.0f; h.prim = kNoPrim;
                uint32_t hinst = 0u;
                {
                    const RenderParams& W = params_view(KP);  // walk
                    float* q = reinterpret_cast<float*>(smem + static_cast<size_t>(wave) * W.lds_per_wave);
                    uint2* stack = reinterpret_cast<uint2*>(q + kQueueFloats);
                    if (depth == 1 && OBJ) {  // camera rays of an object group: one packet walk per member
                        RegStack rst(nullptr, lane);
                        HybridStack hst(reinterpret_cast<float*>(stack), lane, W.scene.stack_cap, W.scene.packet_stack_regs);
                        if (W.scene.stack_cap > W.scene.packet_stack_regs) trace_packet_objects<false>(W.scene, r, alive, hst, h, hinst);
                        else trace_packet_objects<(S >= 8)>(W.scene, r, alive, rst, h, hinst);
                    } else if (depth == 1) {
                        const bool go = alive && may_hit_scene(W.scene, r);
                        if (__ballot(go) != 0) {
                            RegStack rst(nullptr, lane);
                            HybridStack hst(reinterpret_cast<float*>(stack), lane, W.scene.stack_cap, W.scene.packet_stack_regs);
                            if (W.scene.stack_cap > W.scene.packet_stack_regs) trace_packet<false>(W.scene, r, go, hst, h);
                            else trace_packet<(S >= 8), RegStack, MCACHE>(W.scene, r, go, rst, h, mc);
                        }
                    } else {
                        // bounce rays: group walk (once per member of an object group)
                        GroupHit gh;
                        trace_objects<OBJ>(W.scene, r, alive, q, stack, gh);
                        h.t = gh.t; h.u = gh.u; h.v = gh.v; h.prim = gh.prim;
                        hinst = gh.inst;
                    }
                }
                const RenderParams& V = params_view(KP);  // shade + bounce
                if (alive) alive = path_vertex<OBJ, N>(V.scene, h, depth, max_depth, rng, r, L, thr, primary_hit, hinst);
            }
            {   // (the mask of this pixel's lanes is rebuilt from the lane id here: two registers less across the walks)
                int l_ = lane;
                asm volatile("" : "+v"(l_));
                const uint64_t pixel_lanes = (S == 64 ? ~0ull : ((1ull << (S & 63)) - 1ull)) << (l_ & ~(S - 1));
                cnt += static_cast<float>(__popcll(__ballot(primary_hit) & pixel_lanes));
            }
#pragma unroll
            for (int c = 0; c < N; c++) add_samples_in_order<S>(acc[c], L[c], lane);
            const RenderParams& A = params_view(KP);  // accumulation
            if (!RGB && A.chunked && ((s0 + S) & (kSumChunk - 1u)) == 0u && s0 + S <= s_end) chunk_flush(A, off, inpix && sub == 0, acc[0]);
        }
        const RenderParams& E = params_view(KP);  // unit end
        if (inpix && sub == 0) {
            if (RGB) pixel_state_store3(E, off, reinterpret_cast<const float (&)[3]>(acc[0]), cnt);
            else pixel_state_store(E, off, acc[0], cnt);
        }
        if (E.tile_cost && lane == 0) atomicAdd(E.tile_cost + tile_i, static_cast<unsigned long long>(__builtin_readcyclecounter() - t_unit));
    }
    const RenderParams& Z = params_view(KP);
    if (lane == 0 && Z.segments && segs) atomicAdd(Z.segments, segs);
}

// ---- pooled form of render_paths_kernel (round 3) ----------------------------------------------------------------------------
// The fused kernel above traces the bounce rays of ONE pass (8 pixels x 8 samples = at most 64 rays) per call of the 8-lane-group
// walk, and a ray's walk takes 10 to 80 steps: when the queue runs dry the groups idle until the slowest ray of the call finishes
// -- 13 % of the group-iterations of a 64-ray call on the stand-in, 6.5 % of a 256-ray call (tools/sim_collapse.py's traces;
// profiles/r03_notes.md).  Here a wave keeps NSUB passes in flight: per bounce, the passes are shaded one after the other, lane =
// path, and their rays are compacted into ONE queue of up to 64 * NSUB rays that the walk drains in a single call.  The state of
// the passes that are not being shaded -- RNG, radiance, throughput, flags: 11 dwords per path -- and the queue itself (origin,
// direction, inverse direction, hit: 13 dwords per ray) live in a per-wave slab of global memory (RenderParams::pool, 24 dwords
// x 64 * NSUB per wave, L2-resident): the "rays laid out SoA + stream compaction" of the north star, inside one persistent wave.
// Nothing of a path is live in registers across the walk, so the kernel fits 64 VGPRs = 8 waves per SIMD.
// Per path the operations, their order and the RNG stream are those of render_paths_kernel (same path_vertex, same walks, samples
// added in index order): the frame is bit-identical (tests run both kernels on the same cases).
#ifndef MP_POOL_WPE
#define MP_POOL_WPE 8
#endif
constexpr int kPoolQueueRows = 13, kPoolStateRows = 11;
__host__ __device__ constexpr uint32_t pool_floats_per_wave(int nsub) { return static_cast<uint32_t>((kPoolQueueRows + kPoolStateRows) * 64 * nsub); }
constexpr uint32_t kPoolAlive = 1u, kPoolPrimary = 2u, kPoolQueued = 4u;  // flags word: bits 0..2, queue slot << 8

template <int NSUB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MP_POOL_WPE, 8))) void render_paths_pooled_kernel(RenderParams) {
    extern __shared__ __align__(16) unsigned char smem[];
    MP_KERNEL_PARAMS;
    constexpr int S = 8, BW = 4, BH = 2, QN = 64 * NSUB;
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);  // uniform: the pool / stack pointers stay in SGPRs
    const int pix = lane / S, sub = lane % S;
    unsigned long long segs = 0;  // wave-uniform
    uint32_t qstate = blockIdx.x % kWorkQueues;
    float* q;        // ray queue: kPoolQueueRows rows x QN slots
    uint32_t* park;  // parked path state: kPoolStateRows rows x QN (slot = pass * 64 + lane): rng 8, L, thr, flags
    uint2* stack;
    {
        const RenderParams& P0 = params_view(KP);
        q = P0.pool + static_cast<size_t>(blockIdx.x * 4u + static_cast<uint32_t>(wave)) * P0.pool_stride;
        park = reinterpret_cast<uint32_t*>(q + kPoolQueueRows * QN);
        stack = reinterpret_cast<uint2*>(smem + static_cast<size_t>(wave) * P0.lds_per_wave);
    }
    auto park_store = [&](int j, const Rng& rng, float L, float thr, uint32_t flags) {
        // streamed (non-temporal): 200 MB of parked state per launch must not push the scene out of the L2
        uint32_t* p = park + j * 64 + lane;
        __builtin_nontemporal_store(rng.s0.lo, p + 0 * QN); __builtin_nontemporal_store(rng.s0.hi, p + 1 * QN);
        __builtin_nontemporal_store(rng.s1.lo, p + 2 * QN); __builtin_nontemporal_store(rng.s1.hi, p + 3 * QN);
        __builtin_nontemporal_store(rng.s2.lo, p + 4 * QN); __builtin_nontemporal_store(rng.s2.hi, p + 5 * QN);
        __builtin_nontemporal_store(rng.s3.lo, p + 6 * QN); __builtin_nontemporal_store(rng.s3.hi, p + 7 * QN);
        __builtin_nontemporal_store(as_u(L), p + 8 * QN); __builtin_nontemporal_store(as_u(thr), p + 9 * QN); __builtin_nontemporal_store(flags, p + 10 * QN);
    };
    // bounce ray of a path that is still alive: into the queue (compacted over the lanes whose ray can reach the scene at all)
    auto push_ray = [&](const DevScene& sc, const Ray& r, bool alive, uint32_t& nq, uint32_t& flags) {
        const bool queued = alive && may_hit_scene(sc, r);
        const uint64_t am = __ballot(queued);
        const uint32_t slot = nq + static_cast<uint32_t>(rank_below(am));
        if (queued) {
            q[0 * QN + slot] = r.ox; q[1 * QN + slot] = r.oy; q[2 * QN + slot] = r.oz;
            q[3 * QN + slot] = r.dx; q[4 * QN + slot] = r.dy; q[5 * QN + slot] = r.dz;
            q[6 * QN + slot] = r.ix; q[7 * QN + slot] = r.iy; q[8 * QN + slot] = r.iz;
            flags |= kPoolQueued | (slot << 8);
        }
        nq += static_cast<uint32_t>(__popcll(am));
    };
    for (;;) {
        const RenderParams& P = params_view(KP);  // unit setup
        const uint32_t ts = P.tile_size;
        const uint32_t bx = (ts + BW - 1) / BW, by = (ts + BH - 1) / BH, upt = bx * by, total = P.n_tiles * upt;
        MP_NEXT_UNIT(unit)
        const uint32_t b = unit % upt;
        const uint32_t tile_i = P.tile_order ? P.tile_order[unit / upt] : unit / upt;
        const uint64_t t_unit = P.tile_cost ? __builtin_readcyclecounter() : 0;
        const mp_block T = P.tiles[tile_i];
        const uint32_t px = T.min_x + (b % bx) * BW + static_cast<uint32_t>(pix % BW);
        const uint32_t py = T.min_y + (b / bx) * BH + static_cast<uint32_t>(pix / BW);
        const bool inpix = px < T.max_x && py < T.max_y;
        if (__ballot(inpix) == 0) continue;
        const size_t off = (static_cast<size_t>(tile_i) * ts * ts + static_cast<size_t>(py - T.min_y) * ts + (px - T.min_x)) * 4;
        float acc, cnt;  // pixel_sum (grey table: one channel) and alpha (worker.rs:40)
        pixel_state_load(P, off, inpix, sub == 0, acc, cnt);
        const uint32_t s_begin = P.s_begin, s_end = P.s_end, max_depth = P.max_depth;
        // a batch = NSUB consecutive passes of S samples, aligned in the absolute sample index (so that a 256-sample chunk boundary
        // of MP_FLAG_CHUNKED_SUM never falls inside a batch); samples outside [s_begin, s_end) add +0.0, which is exact
        for (uint32_t s0 = s_begin & ~static_cast<uint32_t>(S * NSUB - 1); s0 < s_end; s0 += S * NSUB) {
            uint32_t nq = 0, na = 0;  // rays in the queue / paths alive, over all passes of the batch (wave-uniform)
            // ---- segment 1: camera rays of every pass as one packet each, then the first vertex
#pragma nounroll
            for (int j = 0; j < NSUB; j++) {
                const uint32_t s = s0 + static_cast<uint32_t>(j * S + sub);
                const bool act = inpix && s >= s_begin && s < s_end;
                Rng rng;
                rng_zero(rng);
                Ray r;
                r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
                {
                    const RenderParams& G = params_view(KP);  // ray generation
                    if (act) {
                        rng_seed(rng, sample_key(G.gen, px, py, s));
                        sample_ray_rng(G.gen, px, py, rng, r);
                    }
                }
                segs += static_cast<unsigned long long>(__popcll(__ballot(act)));
                PacketHit h;
                h.t = FLT_MAX; h.u = h.v = 0.0f; h.prim = kNoPrim;
                {
                    const RenderParams& W = params_view(KP);  // walk
                    const bool go = act && may_hit_scene(W.scene, r);
                    if (__ballot(go) != 0) {
                        RegStack rst(nullptr, lane);
                        HybridStack hst(reinterpret_cast<float*>(stack), lane, W.scene.stack_cap, W.scene.packet_stack_regs);
                        if (W.scene.stack_cap > W.scene.packet_stack_regs) trace_packet<false>(W.scene, r, go, hst, h);
                        else trace_packet<true>(W.scene, r, go, rst, h);
                    }
                }
                const RenderParams& V = params_view(KP);  // shade + bounce
                float L[1] = {0.0f}, thr[1] = {1.0f};
                bool alive = act, primary_hit = false;
                if (alive) alive = path_vertex<false, 1>(V.scene, h, 1u, max_depth, rng, r, L, thr, primary_hit);
                uint32_t flags = (alive ? kPoolAlive : 0u) | (primary_hit ? kPoolPrimary : 0u);
                push_ray(V.scene, r, alive, nq, flags);
                na += static_cast<uint32_t>(__popcll(__ballot(alive)));
                park_store(j, rng, L[0], thr[0], flags);
            }
            // ---- segments 2 .. max_depth: one walk over the rays of all passes, then the passes' vertices one after the other
            for (uint32_t depth = 2; depth <= max_depth && na != 0u; depth++) {
                segs += na;
                wave_mem_sync();  // the queue written above is read by other lanes of this wave
                if (nq != 0u) {
                    const RenderParams& W = params_view(KP);
                    trace_wave_pool<QN>(W.scene, q, stack, static_cast<int>(nq));
                }
                wave_mem_sync();
                nq = 0;
                na = 0;
    #pragma nounroll
            for (int j = 0; j < NSUB; j++) {
                    const uint32_t* p = park + j * 64 + lane;
                    uint32_t flags = __builtin_nontemporal_load(p + 10 * QN);
                    bool alive = (flags & kPoolAlive) != 0u;
                    if (__ballot(alive) == 0) continue;  // the whole pass is finished: its parked L / flags stay as they are
                    Rng rng;
                    auto ld = [&](int row) { return static_cast<uint64_t>(__builtin_nontemporal_load(p + row * QN)); };
                    auto ld2 = [&](int row) { return rm::U64{__builtin_nontemporal_load(p + row * QN), __builtin_nontemporal_load(p + (row + 1) * QN)}; };
                    rng.s0 = ld2(0); rng.s1 = ld2(2);
                    rng.s2 = ld2(4); rng.s3 = ld2(6);
                    float L[1] = {as_f(static_cast<uint32_t>(ld(8)))}, thr[1] = {as_f(static_cast<uint32_t>(ld(9)))};
                    bool primary_hit = (flags & kPoolPrimary) != 0u;
                    Ray r;
                    r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
                    PacketHit h;
                    h.t = FLT_MAX; h.u = h.v = 0.0f; h.prim = kNoPrim;
                    if (alive && (flags & kPoolQueued)) {  // the ray this path shot and what it hit (a ray that was not queued missed)
                        const uint32_t slot = flags >> 8;
                        r.ox = q[0 * QN + slot]; r.oy = q[1 * QN + slot]; r.oz = q[2 * QN + slot];
                        r.dx = q[3 * QN + slot]; r.dy = q[4 * QN + slot]; r.dz = q[5 * QN + slot];
                        h.t = q[9 * QN + slot]; h.prim = as_u(q[10 * QN + slot]); h.u = q[11 * QN + slot]; h.v = q[12 * QN + slot];
                    }
                    const RenderParams& V = params_view(KP);
                    if (alive) alive = path_vertex<false, 1>(V.scene, h, depth, max_depth, rng, r, L, thr, primary_hit);
                    flags = (alive ? kPoolAlive : 0u) | (primary_hit ? kPoolPrimary : 0u);
                    // every lane of this pass has read its old slot (the loads above feed the stores below); the new slots are no
                    // higher than the old ones of this pass, so later passes' rays and hits are untouched
                    push_ray(V.scene, r, alive, nq, flags);
                    na += static_cast<uint32_t>(__popcll(__ballot(alive)));
                    park_store(j, rng, L[0], thr[0], flags);
                }
            }
            // ---- pixel_sum += sample, strictly in sample order (worker.rs:41-43): the passes in index order
#pragma nounroll
            for (int j = 0; j < NSUB; j++) {
                const uint32_t* p = park + j * 64 + lane;
                const float L = as_f(p[8 * QN]);
                const bool primary_hit = (p[10 * QN] & kPoolPrimary) != 0u;
                {
                    int l_ = lane;
                    asm volatile("" : "+v"(l_));
                    const uint64_t pixel_lanes = ((1ull << S) - 1ull) << (l_ & ~(S - 1));
                    cnt += static_cast<float>(__popcll(__ballot(primary_hit) & pixel_lanes));
                }
                add_samples_in_order<S>(acc, L, lane);
            }
            const RenderParams& A = params_view(KP);  // accumulation
            if (A.chunked && ((s0 + S * NSUB) & (kSumChunk - 1u)) == 0u && s0 + S * NSUB <= s_end) chunk_flush(A, off, inpix && sub == 0, acc);
        }
        const RenderParams& E = params_view(KP);  // unit end
        if (inpix && sub == 0) pixel_state_store(E, off, acc, cnt);
        if (E.tile_cost && lane == 0) atomicAdd(E.tile_cost + tile_i, static_cast<unsigned long long>(__builtin_readcyclecounter() - t_unit));
    }
    const RenderParams& Z = params_view(KP);
    if (lane == 0 && Z.segments && segs) atomicAdd(Z.segments, segs);
}

// ---- staged ("wavefront") evaluation of the path extension: MP_FLAG_WAVEFRONT --------------------------------------
// The north star's formulation, kept beside the fused render_paths_kernel: the paths of a batch (a few tiles x a chunk of
// samples, ~2 M paths) live in HBM as SoA streams (RNG state, ray, throughput, radiance, hit); per segment: a vertex kernel
// (shade + bounce, one thread per path), a counting sort of the live paths by (tile, direction bin) = stream compaction, and a
// trace kernel over the sorted stream.  Per-path RNG stream and operations are those of the fused kernel (path_vertex), every
// ray's result is independent of its neighbours, and the per-pixel sum is taken in sample order at the end: the frame is
// bit-identical to the fused kernel's and the oracle's (the two pipelines cross-check each other in the tests).  Measured slower
// than the fused kernel, which therefore stays the default.
constexpr uint32_t kDirBins = 512;  // 8 octants x 8 x 8 cells of the octahedral map of |d|

struct WfState {
    uint64_t* rng;       // 4 rows x n
    float* ray;          // 6 rows x n : origin, unit direction
    float* thr;          // nchan rows x n (nchan = 3 for a coloured / textured material table, else 1)
    float* L;            // nchan rows x n
    float* hit_t;        // n
    uint32_t* hit_prim;  // n
    float* hit_u;        // n
    float* hit_v;        // n
    uint32_t* hit_inst;  // n : member of the object group that was hit (groups only; otherwise unused)
    uint32_t* flags;     // n : kWfAlive | kWfPrimaryHit | kWfValid
    uint32_t* key;       // n : sort key of a live path
    uint32_t* idx;       // n : live paths in key order
    uint32_t* hist;      // nbins + 1 : per-key counts of the segment being generated ; [nbins] unused
    uint32_t* offs;      // nbins + 1 : exclusive scan of hist ; [nbins] = number of live paths
    uint32_t* cursor;    // nbins
    uint32_t n, nbins, nchan;
};
constexpr uint32_t kWfAlive = 1u, kWfPrimaryHit = 2u, kWfValid = 4u;

struct WfParams {
    DevScene scene;
    RayGen gen;
    const mp_block* tiles;  // this batch's tiles (device)
    uint32_t n_tiles, tile_size;
    uint32_t tile_base;     // index of the batch's first tile in the caller's tile list (output slot)
    uint32_t s0, sc, s_end; // the chunk covers samples [s0, min(s0 + sc, s_end))
    uint32_t depth, max_depth;
    float* out;
    float inv_spp;
    uint32_t carry_in, finalize, chunked;
    uint32_t lds_per_wave;
    unsigned long long* segments;
    WfState st;
};

__device__ __forceinline__ uint32_t direction_bin(float dx, float dy, float dz) {
    const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
    const float inv = __builtin_amdgcn_rcpf(ax + ay + az);  // approximate: the bin only steers the sort
    const uint32_t qx = min(7u, static_cast<uint32_t>(ax * inv * 8.0f)), qy = min(7u, static_cast<uint32_t>(ay * inv * 8.0f));
    const uint32_t oct = (dx < 0.0f ? 1u : 0u) | (dy < 0.0f ? 2u : 0u) | (dz < 0.0f ? 4u : 0u);
    return oct * 64u + qx * 8u + qy;
}

// path p = (tile_local * ts*ts + (y - min_y) * ts + (x - min_x)) * sc + (s - s0)
// Stage 1: camera rays, generated and walked as packets of 2x2 pixels x 16 samples like render_tiles_packet_kernel.
template <bool LDS_STACK, bool OBJ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 8))) void wf_camera_kernel(WfParams) {
    extern __shared__ __align__(16) unsigned char smem[];
    typedef const __attribute__((address_space(4))) WfParams* kwf_t;
    kwf_t KP = (kwf_t)__builtin_amdgcn_kernarg_segment_ptr();  // WfParams through short-lived views (see params_view)
    const WfParams& P0 = kernarg_view<WfParams>(KP);
    constexpr int S = 16, BW = 2, BH = 2;
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int pix = lane / S, sub = lane % S;
    const uint32_t ts = P0.tile_size, bx = (ts + BW - 1) / BW, by = (ts + BH - 1) / BH, upt = bx * by, total = P0.n_tiles * upt;
    const uint32_t n = P0.st.n;
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    unsigned long long segs = 0;  // camera segments of this wave (wave-uniform)
    for (uint32_t unit = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); unit < total; unit += n_waves) {
        const WfParams& Pu = kernarg_view<WfParams>(KP);
        const uint32_t tile_l = unit / upt, b = unit % upt;
        const mp_block T = Pu.tiles[tile_l];
        const uint32_t px = T.min_x + (b % bx) * BW + static_cast<uint32_t>(pix % BW);
        const uint32_t py = T.min_y + (b / bx) * BH + static_cast<uint32_t>(pix / BW);
        const bool inpix = px < T.max_x && py < T.max_y;
        const uint32_t pbase = ((tile_l * ts + (py - T.min_y)) * ts + (px - T.min_x)) * Pu.sc;
        const uint32_t sc_ = Pu.sc;
        for (uint32_t sl0 = 0; sl0 < sc_; sl0 += S) {
            const WfParams& P = kernarg_view<WfParams>(KP);  // one view per pass
            const uint32_t sl = sl0 + static_cast<uint32_t>(sub), s = P.s0 + sl;
            const bool slot = inpix && sl < P.sc;       // a path slot of the batch exists for this lane
            const bool act = slot && s < P.s_end;       // ... and holds a sample of this launch
            Rng rng;
            rng_zero(rng);
            Ray r;
            r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
            if (act) {
                rng_seed(rng, sample_key(P.gen, px, py, s));
                sample_ray_rng(P.gen, px, py, rng, r);
            }
            segs += static_cast<unsigned long long>(__popcll(__ballot(act)));
            PacketHit h;
            h.t = FLT_MAX; h.u = h.v = 0.0f; h.prim = kNoPrim;
            uint32_t hinst = 0u;
            float* lds = reinterpret_cast<float*>(smem + static_cast<size_t>(static_cast<int>(threadIdx.x) >> 6) * P.lds_per_wave);
            if (OBJ) {  // object group: one packet walk per member
                if (LDS_STACK) {
                    HybridStack st(lds, lane, P.scene.stack_cap, P.scene.packet_stack_regs);
                    trace_packet_objects<false>(P.scene, r, act, st, h, hinst);
                } else {
                    RegStack st(lds, lane);
                    trace_packet_objects<true>(P.scene, r, act, st, h, hinst);
                }
            } else {
                const bool go = act && may_hit_scene(P.scene, r);
                if (__ballot(go) != 0) {
                    if (LDS_STACK) {
                        HybridStack st(lds, lane, P.scene.stack_cap, P.scene.packet_stack_regs);
                        trace_packet<false>(P.scene, r, go, st, h);
                    } else {
                        RegStack st(lds, lane);
                        trace_packet<true>(P.scene, r, go, st, h);
                    }
                }
            }
            if (slot) {
                const uint32_t p = pbase + sl;
                P.st.flags[p] = act ? (kWfAlive | kWfValid) : 0u;
                if (act) {
                    P.st.rng[0 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s0); P.st.rng[1 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s1);
                    P.st.rng[2 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s2); P.st.rng[3 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s3);
                    P.st.ray[0 * static_cast<size_t>(n) + p] = r.ox; P.st.ray[1 * static_cast<size_t>(n) + p] = r.oy;
                    P.st.ray[2 * static_cast<size_t>(n) + p] = r.oz; P.st.ray[3 * static_cast<size_t>(n) + p] = r.dx;
                    P.st.ray[4 * static_cast<size_t>(n) + p] = r.dy; P.st.ray[5 * static_cast<size_t>(n) + p] = r.dz;
                    for (uint32_t c = 0; c < P.st.nchan; c++) {
                        P.st.thr[c * static_cast<size_t>(n) + p] = 1.0f;
                        P.st.L[c * static_cast<size_t>(n) + p] = 0.0f;
                    }
                    P.st.hit_t[p] = h.t; P.st.hit_prim[p] = h.prim; P.st.hit_u[p] = h.u; P.st.hit_v[p] = h.v;
                    if (OBJ) P.st.hit_inst[p] = hinst;
                }
            }
        }
    }
    if (lane == 0 && P0.segments && segs) atomicAdd(P0.segments, segs);
}

// Stage 2: one thread per path: shade the hit of segment P.depth, draw the bounce ray, count it under its sort key.
template <int N, bool OBJ>
__global__ __launch_bounds__(256) void wf_vertex_kernel(WfParams P) {
    const uint32_t n = P.st.n;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        uint32_t fl = P.st.flags[p];
        if (!(fl & kWfAlive)) continue;
        Rng rng;
        rng.s0 = rm::u64_split(P.st.rng[0 * static_cast<size_t>(n) + p]); rng.s1 = rm::u64_split(P.st.rng[1 * static_cast<size_t>(n) + p]);
        rng.s2 = rm::u64_split(P.st.rng[2 * static_cast<size_t>(n) + p]); rng.s3 = rm::u64_split(P.st.rng[3 * static_cast<size_t>(n) + p]);
        Ray r;
        r.ox = P.st.ray[0 * static_cast<size_t>(n) + p]; r.oy = P.st.ray[1 * static_cast<size_t>(n) + p];
        r.oz = P.st.ray[2 * static_cast<size_t>(n) + p]; r.dx = P.st.ray[3 * static_cast<size_t>(n) + p];
        r.dy = P.st.ray[4 * static_cast<size_t>(n) + p]; r.dz = P.st.ray[5 * static_cast<size_t>(n) + p];
        r.ix = r.iy = r.iz = 0.0f;  // not used by path_vertex
        PacketHit h;
        h.t = P.st.hit_t[p]; h.prim = P.st.hit_prim[p]; h.u = P.st.hit_u[p]; h.v = P.st.hit_v[p];
        float L[N], thr[N];
#pragma unroll
        for (int c = 0; c < N; c++) { L[c] = P.st.L[c * static_cast<size_t>(n) + p]; thr[c] = P.st.thr[c * static_cast<size_t>(n) + p]; }
        bool primary = (fl & kWfPrimaryHit) != 0u;
        const bool alive = path_vertex<OBJ, N>(P.scene, h, P.depth, P.max_depth, rng, r, L, thr, primary, OBJ ? P.st.hit_inst[p] : 0u);
        fl = (fl & ~(kWfAlive | kWfPrimaryHit)) | (alive ? kWfAlive : 0u) | (primary ? kWfPrimaryHit : 0u);
        P.st.flags[p] = fl;
#pragma unroll
        for (int c = 0; c < N; c++) { P.st.L[c * static_cast<size_t>(n) + p] = L[c]; P.st.thr[c * static_cast<size_t>(n) + p] = thr[c]; }
        if (alive) {
            P.st.rng[0 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s0); P.st.rng[1 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s1);
            P.st.rng[2 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s2); P.st.rng[3 * static_cast<size_t>(n) + p] = rm::u64_join(rng.s3);
            P.st.ray[0 * static_cast<size_t>(n) + p] = r.ox; P.st.ray[1 * static_cast<size_t>(n) + p] = r.oy;
            P.st.ray[2 * static_cast<size_t>(n) + p] = r.oz; P.st.ray[3 * static_cast<size_t>(n) + p] = r.dx;
            P.st.ray[4 * static_cast<size_t>(n) + p] = r.dy; P.st.ray[5 * static_cast<size_t>(n) + p] = r.dz;
            const uint32_t tile_l = p / (P.tile_size * P.tile_size * P.sc);
            const uint32_t k = tile_l * kDirBins + direction_bin(r.dx, r.dy, r.dz);
            P.st.key[p] = k;
            atomicAdd(P.st.hist + k, 1u);
        }
    }
}

// Stage 3: exclusive scan of the key histogram (one workgroup), cursors and histogram reset for the next segment, and the
// number of live paths = ray segments of the next stage.
__global__ __launch_bounds__(1024) void wf_scan_kernel(WfParams P) {
    __shared__ uint32_t part[1024];
    const uint32_t nb = P.st.nbins, per = (nb + 1023u) / 1024u, t = threadIdx.x;
    uint32_t sum = 0;
    for (uint32_t i = t * per; i < min(nb, (t + 1u) * per); i++) sum += P.st.hist[i];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {  // Hillis-Steele inclusive scan of the per-thread sums
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (uint32_t i = t * per; i < min(nb, (t + 1u) * per); i++) {
        const uint32_t c = P.st.hist[i];
        P.st.offs[i] = run;
        P.st.cursor[i] = 0u;
        P.st.hist[i] = 0u;
        run += c;
    }
    if (t == 1023u) {
        P.st.offs[nb] = part[1023];
        if (P.segments) atomicAdd(P.segments, static_cast<unsigned long long>(part[1023]));
    }
}

// Stage 4: scatter the live paths to their key's range (order inside a key is arbitrary: results do not depend on it).
__global__ __launch_bounds__(256) void wf_scatter_kernel(WfParams P) {
    const uint32_t n = P.st.n;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        if (!(P.st.flags[p] & kWfAlive)) continue;
        const uint32_t k = P.st.key[p];
        P.st.idx[P.st.offs[k] + atomicAdd(P.st.cursor + k, 1u)] = p;
    }
}

// Stage 5: the sorted rays through the 8-lane-group traversal, 64 per wave.  (Walking 64 sorted rays as ONE packet was measured
// too: diffuse bounce rays do not share enough of the tree even when sorted -- 2 586 VALU per ray against ~500 here; see
// profiles/r01_notes.md.)  The sort serves cache locality.
template <bool OBJ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void wf_trace_groups_kernel(WfParams P) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
    float* q = reinterpret_cast<float*>(smem + static_cast<size_t>(wave) * P.lds_per_wave);
    uint2* stack = reinterpret_cast<uint2*>(q + kQueueFloats);
    const uint32_t n = P.st.n, live = P.st.offs[P.st.nbins];
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6), chunks = (live + 63u) / 64u;
    for (uint32_t c = blockIdx.x * (blockDim.x >> 6) + static_cast<uint32_t>(wave); c < chunks; c += n_waves) {
        const uint32_t slot = c * 64u + static_cast<uint32_t>(lane);
        const bool act = slot < live;
        const uint32_t p = act ? P.st.idx[slot] : 0u;
        Ray r;
        r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
        if (act) {
            r.ox = P.st.ray[0 * static_cast<size_t>(n) + p]; r.oy = P.st.ray[1 * static_cast<size_t>(n) + p];
            r.oz = P.st.ray[2 * static_cast<size_t>(n) + p]; r.dx = P.st.ray[3 * static_cast<size_t>(n) + p];
            r.dy = P.st.ray[4 * static_cast<size_t>(n) + p]; r.dz = P.st.ray[5 * static_cast<size_t>(n) + p];
            r.ix = (r.dx == 0.0f) ? INFINITY : 1.0f / r.dx;
            r.iy = (r.dy == 0.0f) ? INFINITY : 1.0f / r.dy;
            r.iz = (r.dz == 0.0f) ? INFINITY : 1.0f / r.dz;
        }
        // compaction of the rays that can reach the object into the wave's queue + the 8-lane-group walk (once per member of an
        // object group, closest wins)
        GroupHit gh;
        trace_objects<OBJ>(P.scene, r, act, q, stack, gh);
        if (act) {
            P.st.hit_t[p] = gh.t;
            P.st.hit_prim[p] = gh.prim;
            P.st.hit_u[p] = gh.u;
            P.st.hit_v[p] = gh.v;
            if (OBJ) P.st.hit_inst[p] = gh.inst;
        }
    }
}

// Stage 6: pixel_sum += sample in sample order (worker.rs:41-43), one thread per pixel of the batch.
__global__ __launch_bounds__(256) void wf_accumulate_kernel(WfParams P) {
    const uint32_t ts = P.tile_size, npx = P.n_tiles * ts * ts;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += gridDim.x * blockDim.x) {
        const uint32_t tile_l = i / (ts * ts), q = i % (ts * ts), x = q % ts, y = q / ts;
        const mp_block T = P.tiles[tile_l];
        if (!(T.min_x + x < T.max_x && T.min_y + y < T.max_y)) continue;
        float* o = P.out + (static_cast<size_t>(P.tile_base + tile_l) * ts * ts + q) * 4;
        if (P.st.nchan == 3u) {  // coloured / textured material table: slot = {sum r, sum g, sum b, hit count}; never chunked
            float a3[3] = {0.0f, 0.0f, 0.0f}, c3 = 0.0f;
            if (P.carry_in) {
                const float4 prev = *reinterpret_cast<const float4*>(o);
                a3[0] = prev.x; a3[1] = prev.y; a3[2] = prev.z; c3 = prev.w;
            }
            const uint32_t ns3 = min(P.sc, P.s_end - P.s0);
            const uint32_t pb3 = i * P.sc;
            for (uint32_t sl = 0; sl < ns3; sl++) {
                for (uint32_t c = 0; c < 3u; c++) a3[c] += P.st.L[c * static_cast<size_t>(P.st.n) + pb3 + sl];
                c3 += (P.st.flags[pb3 + sl] & kWfPrimaryHit) ? 1.0f : 0.0f;
            }
            const float sc3 = P.finalize ? P.inv_spp : 1.0f;
            *reinterpret_cast<float4*>(o) = make_float4(a3[0] * sc3, a3[1] * sc3, a3[2] * sc3, c3 * sc3);
            continue;
        }
        float acc = 0.0f, cnt = 0.0f;
        double tot = 0.0;  // MP_FLAG_CHUNKED_SUM: slot = {chunk sum, hit count, f64 total} (pixel_state_load)
        if (P.carry_in) {
            const float4 prev = *reinterpret_cast<const float4*>(o);
            acc = prev.x;
            cnt = P.chunked ? prev.y : prev.w;
            if (P.chunked) tot = *reinterpret_cast<const double*>(o + 2);
        }
        const uint32_t ns = min(P.sc, P.s_end - P.s0);
        const uint32_t pbase = i * P.sc;
        for (uint32_t sl = 0; sl < ns; sl++) {
            acc += P.st.L[pbase + sl];
            cnt += (P.st.flags[pbase + sl] & kWfPrimaryHit) ? 1.0f : 0.0f;
            if (P.chunked && ((P.s0 + sl + 1u) & (kSumChunk - 1u)) == 0u) { tot = tot + static_cast<double>(acc); acc = 0.0f; }
        }
        if (P.chunked) {
            if (!P.finalize) {
                *reinterpret_cast<float2*>(o) = make_float2(acc, cnt);
                *reinterpret_cast<double*>(o + 2) = tot;
                continue;
            }
            if (((P.s0 + ns) & (kSumChunk - 1u)) != 0u) tot = tot + static_cast<double>(acc);
            const double inv = 1.0 / static_cast<double>(P.gen.spp);
            const float m = static_cast<float>(tot * inv), a = static_cast<float>(static_cast<double>(cnt) * inv);
            *reinterpret_cast<float4*>(o) = make_float4(m, m, m, a);
            continue;
        }
        const float m = P.finalize ? acc * P.inv_spp : acc, a = P.finalize ? cnt * P.inv_spp : cnt;
        *reinterpret_cast<float4*>(o) = make_float4(m, m, m, a);
    }
}

// ---- CameraSampler::sample_ray batched (camera.rs:176-191) -----------------------------------------------------
__global__ __launch_bounds__(256) void generate_rays_kernel(RayGen G, mp_block blk, uint32_t sample, float* ox, float* oy,
                                                            float* oz, float* dx, float* dy, float* dz) {
    const uint32_t w = blk.max_x - blk.min_x, h = blk.max_y - blk.min_y;
    const uint64_t n = static_cast<uint64_t>(w) * h;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
         i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        Ray r;
        sample_ray(G, blk.min_x + static_cast<uint32_t>(i % w), blk.min_y + static_cast<uint32_t>(i / w), sample, r);
        ox[i] = r.ox; oy[i] = r.oy; oz[i] = r.oz;
        dx[i] = r.dx; dy[i] = r.dy; dz[i] = r.dz;
    }
}

// ---- tile buffer -> image (machinery.rs:78-89) + color_to_image (worker.rs:69-76) ----------------------------
__device__ __forceinline__ uint8_t to_u8(float c) {
    float x = roundf(c * 255.0f);  // half away from zero
    if (x != x) return 0;          // `as u8` on NaN
    x = fminf(fmaxf(x, 0.0f), 255.0f);
    return static_cast<uint8_t>(x);
}

// mode 0: the buffer holds finished pixels (means).  Preview of an unfinished MP_FLAG_ACCUMULATE buffer after k samples (the buffer
// is only read): mode 1: slot = {sum r, sum g, sum b, hits} (r = g = b for a grey table) -> each * inv_k with
// inv_k = 1.0f / (float)k (worker.rs:44 for the samples drawn so far); mode 2 (MP_FLAG_CHUNKED_SUM): slot = {chunk sum, hits, f64 total} ->
// (f32)((total + (f64)chunk sum) * (1.0 / (f64)k)), (f32)((f64)hits * (1.0 / (f64)k)) -- pixel_state_store's rule for k samples.
__global__ __launch_bounds__(256) void untile_kernel(uint32_t width, uint32_t height, uint32_t ts, const mp_block* tiles,
                                                     uint32_t n_tiles, const float* src, float* img_f32, uint8_t* img_u8,
                                                     uint32_t mode, float inv_k, double inv_k64) {
    const uint64_t per_tile = static_cast<uint64_t>(ts) * ts;
    const uint64_t n = per_tile * n_tiles;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
         i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint32_t tile_i = static_cast<uint32_t>(i / per_tile), p = static_cast<uint32_t>(i % per_tile);
        const mp_block T = tiles[tile_i];
        const uint32_t x = T.min_x + p % ts, y = T.min_y + p / ts;
        if (x >= T.max_x || y >= T.max_y || x >= width || y >= height) continue;
        float4 v = *reinterpret_cast<const float4*>(src + i * 4);
        if (mode == 1u) {  // every channel on its own: a grey slot {m, m, m, a} gives {m*inv_k, m*inv_k, m*inv_k, a*inv_k}
            v = make_float4(v.x * inv_k, v.y * inv_k, v.z * inv_k, v.w * inv_k);
        } else if (mode == 2u) {
            const double tot = *reinterpret_cast<const double*>(src + i * 4 + 2) + static_cast<double>(v.x);
            const float m = static_cast<float>(tot * inv_k64);
            v = make_float4(m, m, m, static_cast<float>(static_cast<double>(v.y) * inv_k64));
        }
        const size_t o = (static_cast<size_t>(y) * width + x) * 4;
        if (img_f32) *reinterpret_cast<float4*>(img_f32 + o) = v;
        if (img_u8) {
            uchar4 c = make_uchar4(to_u8(v.x), to_u8(v.y), to_u8(v.z), to_u8(v.w));
            *reinterpret_cast<uchar4*>(img_u8 + o) = c;
        }
    }
}

// color_to_image (worker.rs:69-76) over a tile-major pixel buffer: RGBA f32 -> RGBA u8, same layout (the render() worker reads
// both back and only copies rows on the host).
__global__ __launch_bounds__(256) void quantise_kernel(const float* src, uint8_t* dst, uint64_t n_pixels) {
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_pixels;
         i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const float4 v = *reinterpret_cast<const float4*>(src + i * 4);
        *reinterpret_cast<uchar4*>(dst + i * 4) = make_uchar4(to_u8(v.x), to_u8(v.y), to_u8(v.z), to_u8(v.w));
    }
}

__global__ void set_u64_kernel(unsigned long long* p, unsigned long long v) { *p = v; }

// UniformFloat::new_inclusive(low, high).scale (rand 0.9): (high-low)/max_rand, reduced by ulps until
// scale*max_rand + low <= high
float uniform_inclusive_scale(float low, float high) {
    const float max_rand = 1.0f - FLT_EPSILON;
    float scale = (high - low) / max_rand;
    for (;;) {
        volatile float top = scale * max_rand;
        top = top + low;
        if (!(top > high)) break;
        uint32_t b;
        __builtin_memcpy(&b, &scale, 4);
        b -= 1;
        __builtin_memcpy(&scale, &b, 4);
    }
    return scale;
}

// Seeded mode (include/minipath_hip.h): the first SplitMix64 output for state `seed`, so that consecutive seeds give unrelated
// sample streams; the per-sample index is added on the device (sample_key).
uint64_t mixed_seed(uint64_t seed) {
    uint64_t z = seed + 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

}  // namespace

int check(hipError_t e, const char* what, std::string& err) {
    if (e == hipSuccess) return MP_OK;
    err = std::string(what) + ": " + hipGetErrorString(e);
    return MP_ERR_HIP;
}

static_assert(kPlanQueueFloats == kQueueFloats && kPlanMaskCacheDwords == kMaskCacheDwords && kPlanDirBins == kDirBins &&
                  kPlanPoolFloatsPerSub == pool_floats_per_wave(1),
              "launch_plan.h sizes the launches with the device code's constants");

// Launch record (diagnostic, mp_ctx_last_kernels) and the one place that launches: launch() (family_launch.h) notes the row's name --
// the kernel with its template arguments as kernel_table.h writes them -- in the calling thread's list and then launches that row's
// kernel.  Distinct names, in launch order; the usual case is a compare against a handful of ids.
namespace {
thread_local std::vector<KernelId> t_launched;
}  // namespace
void note_launch(KernelId id) {
    if (std::find(t_launched.begin(), t_launched.end(), id) == t_launched.end()) t_launched.push_back(id);
}

int launched(KernelId id, std::string& err) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MP_OK : check(e, (std::string(kKernelNames[id]) + " launch").c_str(), err);
}

namespace {

// this unit's rows: the families that have no unit of their own yet, and the utilities
#define MP_KERNELS_HERE(X) MP_KERNELS_PATHS(X) MP_KERNELS_TILES(X) MP_KERNELS_AOV(X) MP_KERNELS_STAGED(X) MP_KERNELS_UTILITIES(X)
MP_FAMILY_LAUNCHER(MP_KERNELS_HERE)

void fill_raygen(RayGen& G, const mp_camera_sampler& s, uint32_t width, uint32_t spp, uint64_t seed) {
    G.s = s;
    G.jitter_scale = uniform_inclusive_scale(-0.5f, 0.5f);
    G.width = width;
    G.spp = spp;
    G.seed = mixed_seed(seed);
}

// the fields RenderParams and WfParams share
template <class Params>
void fill_common(Params& P, const RenderLaunch& L) {
    P.scene = L.scene;
    fill_raygen(P.gen, L.sampler, L.width, L.spp, L.seed);
    P.tile_size = L.tile_size;
    P.out = L.d_out;
    P.inv_spp = 1.0f / static_cast<float>(L.spp);
    P.chunked = L.chunked ? 1u : 0u;
    P.max_depth = L.max_depth;
    P.segments = L.d_segments;
}

void fill_render(RenderParams& P, const RenderLaunch& L, const LaunchPlan& plan) {
    fill_common(P, L);
    P.tiles = L.d_tiles;
    P.n_tiles = L.n_tiles;
    P.counter = L.d_counter;
    P.s_begin = L.pass_begin;
    P.s_end = L.pass_end;
    P.carry_in = L.carry_in ? 1u : 0u;
    P.finalize = L.finalize ? 1u : 0u;
    P.tile_order = L.d_tile_order;
    P.tile_cost = L.d_tile_cost;
    P.pool = nullptr;
    P.pool_stride = plan.pool_stride;
    P.lds_per_wave = plan.lds_per_wave;
}

int zero_work_queues(const RenderLaunch& L, hipStream_t st, std::string& err) {
    return check(hipMemsetAsync(L.d_counter, 0, kWorkQueues * kWorkQueueStride * sizeof(uint32_t), st), "hipMemsetAsync(counter)", err);
}

}  // namespace

void launch_log_clear() { t_launched.clear(); }

// the names noted since launch_log_clear() on this thread, one per line
std::string launch_log_text() {
    std::string out;
    for (KernelId id : t_launched) out += (out.empty() ? "" : "\n") + std::string(kKernelNames[id]);
    return out;
}

int launch_render_tiles(const RenderLaunch& L, void* stream, std::string& err) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (L.n_tiles == 0) return MP_OK;
    const LaunchPlan plan = plan_render_tiles(L);
    if (plan.rc) return refused(plan, err);
    RenderParams P;
    fill_render(P, L, plan);
    int rc = zero_work_queues(L, st, err);
    if (rc) return rc;
    if (plan.pool_bytes) {
        rc = check(hipMallocAsync(reinterpret_cast<void**>(&P.pool), plan.pool_bytes, st), "hipMallocAsync(path pool)", err);
        if (rc) return rc;
    }
    rc = launch(plan.kernel, plan.grid, 256, plan.lds, st, err, P);
    if (P.pool) (void)hipFreeAsync(P.pool, st);
    return rc;
}

// mp_render_aov_device / mp_render_aov_pass_device: samples [pass_begin, pass_end) on top of the planes' state, no path extension
int launch_render_aov(const RenderLaunch& L, const mp_aov_planes_ex& planes, void* stream, std::string& err) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (L.n_tiles == 0) return MP_OK;
    const LaunchPlan plan = plan_render_aov(L);
    if (plan.rc) return refused(plan, err);
    AovParams A;
    RenderParams& P = A.r;
    fill_render(P, L, plan);
    P.out = nullptr;
    P.chunked = 0u;
    P.max_depth = 0;
    P.segments = nullptr;
    A.shade = planes.d_shade;
    A.normal = planes.d_normal;
    A.albedo = planes.d_albedo;
    A.ids = planes.d_ids;
    A.position = planes.d_position;
    A.shade_sq = planes.d_shade_sq;
    A.park_pixel = plan.park_pixel;
    const int rc = zero_work_queues(L, st, err);
    if (rc) return rc;
    return launch(plan.kernel, plan.grid, 256, plan.lds, st, err, A);
}

int launch_render_paths_wavefront(const RenderLaunch& L, void* stream, std::string& err) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (L.n_tiles == 0) return MP_OK;
    const WavefrontPlan plan = plan_render_paths_wavefront(L);
    if (plan.rc) return refused(plan, err);
    WfParams P;
    fill_common(P, L);
    P.lds_per_wave = plan.cam_lds_per_wave;
    P.st.nchan = plan.nchan;
    const size_t n64 = plan.n64, bin_bytes = (static_cast<size_t>(plan.nbins) + 64) * 4;
    unsigned char* ws = nullptr;
    int rc = check(hipMallocAsync(reinterpret_cast<void**>(&ws), plan.ws_bytes, st), "hipMallocAsync(path state)", err);
    if (rc) return rc;
    unsigned char* w = ws;
    auto take = [&](size_t b) { unsigned char* r = w; w += b; return r; };
    P.st.rng = reinterpret_cast<uint64_t*>(take(n64 * 32));
    P.st.ray = reinterpret_cast<float*>(take(n64 * 24));
    P.st.thr = reinterpret_cast<float*>(take(n64 * 4 * plan.nchan));
    P.st.L = reinterpret_cast<float*>(take(n64 * 4 * plan.nchan));
    P.st.hit_t = reinterpret_cast<float*>(take(n64 * 4));
    P.st.hit_prim = reinterpret_cast<uint32_t*>(take(n64 * 4));
    P.st.hit_u = reinterpret_cast<float*>(take(n64 * 4));
    P.st.hit_v = reinterpret_cast<float*>(take(n64 * 4));
    P.st.hit_inst = reinterpret_cast<uint32_t*>(take(n64 * 4));
    P.st.flags = reinterpret_cast<uint32_t*>(take(n64 * 4));
    P.st.key = reinterpret_cast<uint32_t*>(take(n64 * 4));
    P.st.idx = reinterpret_cast<uint32_t*>(take(n64 * 4));
    P.st.hist = reinterpret_cast<uint32_t*>(take(bin_bytes));
    P.st.offs = reinterpret_cast<uint32_t*>(take(bin_bytes));
    P.st.cursor = reinterpret_cast<uint32_t*>(take(bin_bytes));
    for (uint32_t tile_base = 0; tile_base < L.n_tiles && !rc; tile_base += plan.tb) {
        const uint32_t ntb = std::min(plan.tb, L.n_tiles - tile_base);
        const WavefrontBatch B = plan.batch(ntb);
        P.tiles = L.d_tiles + tile_base;
        P.n_tiles = ntb;
        P.tile_base = tile_base;
        for (uint32_t s0 = L.pass_begin; s0 < L.pass_end && !rc; s0 += plan.sc) {
            P.s0 = s0;
            P.sc = plan.sc;
            P.s_end = L.pass_end;
            P.st.n = B.n;
            P.st.nbins = B.nbins;
            P.carry_in = (L.carry_in || s0 > L.pass_begin) ? 1u : 0u;
            P.finalize = (L.finalize && s0 + plan.sc >= L.pass_end) ? 1u : 0u;
            rc = check(hipMemsetAsync(P.st.hist, 0, (static_cast<size_t>(P.st.nbins) + 1) * 4, st), "hipMemsetAsync(histogram)", err);
            if (rc) break;
            // path slots of pixels outside a clipped tile are never written by the camera stage: they must read as dead
            rc = check(hipMemsetAsync(P.st.flags, 0, static_cast<size_t>(P.st.n) * 4, st), "hipMemsetAsync(path flags)", err);
            if (rc) break;
            rc = launch(plan.camera, B.cam_grid, 256, plan.cam_lds, st, err, P);
            WfParams G = P;  // bounce stage: LDS ray queue + eight traversal stacks per wave
            G.lds_per_wave = plan.trace_lds_per_wave;
            for (uint32_t depth = 1; depth <= L.max_depth && !rc; depth++) {
                P.depth = depth;
                rc = launch(plan.vertex, B.flat_grid, 256, 0, st, err, P);
                if (rc || depth == L.max_depth) break;
                rc = launch(K_WF_SCAN, 1, 1024, 0, st, err, P);
                if (!rc) rc = launch(K_WF_SCATTER, B.flat_grid, 256, 0, st, err, P);
                if (!rc) rc = launch(plan.trace, plan.trace_grid, 256, plan.trace_lds, st, err, G);
            }
            if (!rc) rc = launch(K_WF_ACCUMULATE, B.px_grid, 256, 0, st, err, P);
        }
    }
    (void)hipFreeAsync(ws, st);
    return rc;
}

int launch_trace_rays(const DevScene& sc, const float* ox, const float* oy, const float* oz, const float* dx,
                      const float* dy, const float* dz, uint64_t n, const mp_hits_soa& hits, int cu_count, void* stream,
                      std::string& err) {
    return launch_rays(kQueryClosest, sc, ox, oy, oz, dx, dy, dz, nullptr, n, &hits, nullptr, cu_count, stream, err);
}

// occluded != NULL: the any-hit kernel (hits unused), otherwise the bounded closest hit
int launch_query_rays(const DevScene& sc, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                      const float* dz, const float* tmax, uint64_t n, const mp_hits_soa* hits, uint8_t* occluded, int cu_count,
                      void* stream, std::string& err) {
    return launch_rays(occluded ? kQueryAnyHit : kQueryBounded, sc, ox, oy, oz, dx, dy, dz, tmax, n, hits, occluded, cu_count, stream, err);
}

int launch_set_u64(unsigned long long* d_ptr, unsigned long long value, void* stream, std::string& err) {
    return launch(K_SET_U64, 1, 1, 0, static_cast<hipStream_t>(stream), err, d_ptr, value);
}

int launch_generate_rays(const mp_camera_sampler& s, uint32_t width, uint32_t spp, uint64_t seed, mp_block block,
                         uint32_t sample, float* ox, float* oy, float* oz, float* dx, float* dy, float* dz, void* stream,
                         std::string& err) {
    const uint64_t n = static_cast<uint64_t>(block.max_x - block.min_x) * (block.max_y - block.min_y);
    if (n == 0) return MP_OK;
    RayGen G;
    fill_raygen(G, s, width, spp, seed);
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((n + 255) / 256, 8192));
    return launch(K_GENERATE_RAYS, grid, 256, 0, static_cast<hipStream_t>(stream), err, G, block, sample, ox, oy, oz, dx, dy, dz);
}

int launch_untile(uint32_t width, uint32_t height, uint32_t tile_size, const mp_block* d_tiles, uint32_t n_tiles,
                  const float* d_tiles_f32, float* d_image_f32, uint8_t* d_image_u8, void* stream, std::string& err,
                  uint32_t preview_mode, uint32_t preview_samples) {
    const uint64_t n = static_cast<uint64_t>(tile_size) * tile_size * n_tiles;
    if (n == 0) return MP_OK;
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((n + 255) / 256, 8192));
    const uint32_t k = std::max<uint32_t>(preview_samples, 1u);
    return launch(K_UNTILE, grid, 256, 0, static_cast<hipStream_t>(stream), err, width, height, tile_size, d_tiles, n_tiles, d_tiles_f32,
                  d_image_f32, d_image_u8, preview_mode, 1.0f / static_cast<float>(k), 1.0 / static_cast<double>(k));
}

int launch_quantise(const float* d_rgba_f32, uint8_t* d_rgba_u8, uint64_t n_pixels, void* stream, std::string& err) {
    if (n_pixels == 0) return MP_OK;
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((n_pixels + 255) / 256, 8192));
    return launch(K_QUANTISE, grid, 256, 0, static_cast<hipStream_t>(stream), err, d_rgba_f32, d_rgba_u8, n_pixels);
}

}  // namespace mp

#ifdef MP_PROF_MISSES
// the first n counters (n <= 10: every slot of g_prof); reset != 0 zeroes all of them afterwards
extern "C" int mp_prof_read_n(unsigned long long* out, int n, int reset) {
    constexpr int kSlots = static_cast<int>(sizeof(mp::g_prof) / sizeof(mp::g_prof[0]));
    if (n < 0 || n > kSlots) return 1;
    unsigned long long all[kSlots] = {};
    if (hipMemcpyFromSymbol(all, HIP_SYMBOL(mp::g_prof), sizeof(all)) != hipSuccess) return 1;
    for (int i = 0; i < n; i++) out[i] = all[i];
    if (reset) {
        const unsigned long long z[kSlots] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(mp::g_prof), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
// (the entry points from before the counters grew: the first eight, the first four)
extern "C" int mp_prof_read8(unsigned long long* out, int reset) { return mp_prof_read_n(out, 8, reset); }
extern "C" int mp_prof_read(unsigned long long* out, int reset) { return mp_prof_read_n(out, 4, reset); }
#endif
