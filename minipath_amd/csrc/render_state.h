// What the render kernels of the four families share around the walk: RenderParams and its short-lived kernarg views, the pixel
// state carried across launches (plain and MP_FLAG_CHUNKED_SUM), the work queues (MP_NEXT_UNIT), the in-order sample sums, the
// per-unit switches of the cached kernels, and the host code that fills these structs.  Used by kernels_tiles.hip, kernels_aov.hip,
// kernels_paths.hip and kernels_staged.hip (and path_shading.h): a change here rebuilds those four units.
#pragma once

#include "family_launch.h"
#include "wave_common.h"

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

// the fields RenderParams and WfParams (kernels_staged.hip) share
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

int zero_work_queues(const RenderLaunch& L, hipStream_t st, std::string& err) {
    return check(hipMemsetAsync(L.d_counter, 0, kWorkQueues * kWorkQueueStride * sizeof(uint32_t), st), "hipMemsetAsync(counter)", err);
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

}  // namespace
}  // namespace mp
