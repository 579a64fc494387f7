// libminipath_adaptive.so: the device operations of adaptive sampling of include/minipath_adaptive.h -- the kernels and the C ABI
// over them.  The header's text is the contract; tests/adaptive_model.py restates it in numpy and the kernels must give its bits,
// so every operation below is written out one rounding at a time (built with -ffp-contract=off, correctly rounded divide and
// sqrt, subnormals kept: the flags of libminipath_hip.so).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/minipath_adaptive.h"
#include "../post/post_abi.h"

namespace mpa {

constexpr uint32_t BLOCK = 256;
constexpr uint32_t WAVES = BLOCK / 64;
constexpr uint32_t CHUNK = 4 * BLOCK;  // pixels one block of move_tiles_kernel / finish_tiles_kernel takes: four per thread

// the header's max(a, b): b for a NaN a, +0 for max(-0, 0)
__device__ __forceinline__ float mx(float a, float b) { return a > b ? a : b; }

// The order -inf < ... < -0 < +0 < ... < +inf on non-NaN floats as an order on u32 keys; 0 is no float's key (it would be a
// negative NaN's), so it stands for "no pixel yet".
__device__ __forceinline__ uint32_t key_of(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t k) {
    return k == 0u ? 0.f : __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// One block per slot.  Each thread walks the slot's pixels 256 apart (one pass for ts <= 16, a loop above), 16-byte loads of both
// planes; open counts and error keys are reduced through the wave by __shfl_xor, across the four waves through LDS, and thread 0
// stores the slot's two results.
__global__ __launch_bounds__(BLOCK) void tile_error_kernel(const float4* __restrict__ shade, const float4* __restrict__ shade_sq,
                                                           const uint2* __restrict__ tile_wh, uint32_t ts, float r, float threshold,
                                                           float floor, uint32_t* __restrict__ open, float* __restrict__ max_err) {
    __shared__ uint32_t s_open[WAVES];
    __shared__ uint32_t s_key[WAVES];
    const uint32_t slot = blockIdx.x;
    const uint2 wh = tile_wh[slot];
    const uint32_t w = wh.x < ts ? wh.x : ts, h = wh.y < ts ? wh.y : ts;
    const uint32_t per_tile = ts * ts;  // ts < 2^16 (the host refuses more)
    const uint32_t rows_end = h * ts;   // owned pixels lie below it
    const float4* s1 = shade + static_cast<size_t>(slot) * per_tile;
    const float4* s2 = shade_sq + static_cast<size_t>(slot) * per_tile;

    uint32_t n_open = 0, key = 0;
    // four pixels per thread and trip, all eight loads issued before the first is used (rows_end + 3 * BLOCK < 2^32)
    for (uint32_t p0 = threadIdx.x; p0 < rows_end; p0 += 4 * BLOCK) {
        bool own[4];
        float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t p = p0 + i * BLOCK;
            own[i] = p < rows_end && p % ts < w;
            if (own[i]) {
                s[i] = s1[p].x;
                q[i] = s2[p].x;
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const float m = s[i] * r;
            const float m2 = q[i] * r;
            const float d = m2 - m * m;
            const float v = mx(d, 0.f) * r;
            float e = sqrtf(v) / (m + floor);
            if (!own[i]) continue;
            if (!(e <= threshold)) ++n_open;
            if (!(e == e)) e = INFINITY;
            const uint32_t k = key_of(e);
            key = k > key ? k : key;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        n_open += __shfl_xor(n_open, off);
        const uint32_t k = __shfl_xor(key, off);
        key = k > key ? k : key;
    }
    const uint32_t lane = threadIdx.x % 64u, wave = threadIdx.x / 64u;
    if (lane == 0) {
        s_open[wave] = n_open;
        s_key[wave] = key;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (uint32_t i = 1; i < WAVES; ++i) {
            n_open += s_open[i];
            key = s_key[i] > key ? s_key[i] : key;
        }
        open[slot] = n_open;
        max_err[slot] = float_of(key);
    }
}

// Block b takes chunk b % chunks of move j = b / chunks: four 16-byte pixels per thread, loads first.
__global__ __launch_bounds__(BLOCK) void move_tiles_kernel(const uint4* __restrict__ src, uint32_t src_slots,
                                                           const uint32_t* __restrict__ src_slot, uint4* __restrict__ dst,
                                                           uint32_t dst_slots, const uint32_t* __restrict__ dst_slot, uint32_t per_tile,
                                                           uint32_t chunks) {
    const uint32_t j = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const uint32_t from = src_slot ? src_slot[j] : j, to = dst_slot ? dst_slot[j] : j;
    if (from >= src_slots || to >= dst_slots) return;
    const uint4* s = src + static_cast<size_t>(from) * per_tile;
    uint4* d = dst + static_cast<size_t>(to) * per_tile;
    const uint32_t p0 = c * CHUNK + threadIdx.x;  // < per_tile + CHUNK < 2^32
    const uint32_t p1 = p0 + BLOCK, p2 = p0 + 2 * BLOCK, p3 = p0 + 3 * BLOCK;
    uint4 v0 = {}, v1 = {}, v2 = {}, v3 = {};
    if (p0 < per_tile) v0 = s[p0];
    if (p1 < per_tile) v1 = s[p1];
    if (p2 < per_tile) v2 = s[p2];
    if (p3 < per_tile) v3 = s[p3];
    if (p0 < per_tile) d[p0] = v0;
    if (p1 < per_tile) d[p1] = v1;
    if (p2 < per_tile) d[p2] = v2;
    if (p3 < per_tile) d[p3] = v3;
}

// Block b takes chunk b % chunks of slot b / chunks; a slot with nothing to scale leaves at once.
__global__ __launch_bounds__(BLOCK) void finish_tiles_kernel(float4* __restrict__ plane, const uint32_t* __restrict__ samples,
                                                             const uint2* __restrict__ tile_wh, uint32_t sample_count, uint32_t ts,
                                                             uint32_t per_tile, uint32_t chunks) {
    const uint32_t slot = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const uint32_t k = samples[slot];
    if (k == 0u || k >= sample_count) return;
    const float inv_k = 1.0f / static_cast<float>(k);
    const uint2 wh = tile_wh[slot];
    const uint32_t w = wh.x < ts ? wh.x : ts, h = wh.y < ts ? wh.y : ts;
    const uint32_t rows_end = h * ts;
    float4* t = plane + static_cast<size_t>(slot) * per_tile;
    const uint32_t p0 = c * CHUNK + threadIdx.x;  // < per_tile + CHUNK < 2^32
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t p = p0 + i * BLOCK;
        if (p >= rows_end || p % ts >= w) continue;
        const float4 v = t[p];
        t[p] = make_float4(v.x * inv_k, v.y * inv_k, v.z * inv_k, v.w * inv_k);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
namespace {

constexpr uint64_t kMaxBlocks = 0x7FFFFFFFull;  // a grid is one dimension of at most 2^31 - 1 blocks

}  // namespace
}  // namespace mpa

using namespace mpa;

extern "C" {

const char* mpa_last_error(void) { return g_last_error.c_str(); }

int mpa_last_kernels(char* buf, size_t cap, size_t* needed) {
    return guarded([&]() -> int { return copy_last_kernels(buf, cap, needed); });
}

int mpa_tile_error(int device_id, uint32_t tile_size, uint32_t n_slots, uint32_t samples_done, float threshold, float floor,
                   const float* d_shade, const float* d_shade_sq, const uint32_t* d_tile_wh, uint32_t* d_open, float* d_max_err,
                   void* stream) {
    return guarded([&]() -> int {
        if (!d_shade || !d_shade_sq || !d_tile_wh || !d_open || !d_max_err) return fail(MP_ERR_INVALID, "NULL argument");
        if (n_slots == 0 || tile_size == 0 || samples_done == 0) return fail(MP_ERR_INVALID, "n_slots, tile_size or samples_done is 0");
        if (threshold != threshold) return fail(MP_ERR_INVALID, "threshold is NaN");
        if (!(floor > 0.f) || std::isinf(floor)) return fail(MP_ERR_INVALID, "floor is not finite and > 0");
        if (device_id < 0) return fail(MP_ERR_INVALID, "negative device_id");
        const void* inputs[] = {d_shade, d_shade_sq, d_tile_wh};
        for (const void* in : inputs)
            if (in == d_open || in == d_max_err) return fail(MP_ERR_INVALID, "an output aliases an input");
        if (static_cast<const void*>(d_open) == static_cast<const void*>(d_max_err)) return fail(MP_ERR_INVALID, "d_max_err aliases d_open");
        if (!all_aligned({d_shade, d_shade_sq}, kPlaneAlign)) return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");
        if (tile_size > MPA_MAX_TILE_SIZE) return fail(MP_ERR_UNSUPPORTED, "tile_size above MPA_MAX_TILE_SIZE");
        if (n_slots > kMaxBlocks) return fail(MP_ERR_UNSUPPORTED, "too many slots for one launch");
        const float r = 1.0f / static_cast<float>(samples_done);

        DeviceScope dev;
        if (hipError_t e = dev.enter(device_id); e != hipSuccess) return hip_fail(e, "hipSetDevice");
        LaunchLog log;
        return launch(log, "tile_error_kernel", tile_error_kernel, dim3(n_slots), dim3(BLOCK), stream,
                      reinterpret_cast<const float4*>(d_shade), reinterpret_cast<const float4*>(d_shade_sq),
                      reinterpret_cast<const uint2*>(d_tile_wh), tile_size, r, threshold, floor, d_open, d_max_err);
    });
}

int mpa_move_tiles(int device_id, uint32_t tile_size, uint32_t n, const void* d_src, uint32_t src_slots, const uint32_t* d_src_slot,
                   void* d_dst, uint32_t dst_slots, const uint32_t* d_dst_slot, void* stream) {
    return guarded([&]() -> int {
        if (!d_src || !d_dst) return fail(MP_ERR_INVALID, "NULL argument");
        if (d_src == d_dst) return fail(MP_ERR_INVALID, "d_src == d_dst");
        if (tile_size == 0 || src_slots == 0 || dst_slots == 0) return fail(MP_ERR_INVALID, "tile_size, src_slots or dst_slots is 0");
        if (device_id < 0) return fail(MP_ERR_INVALID, "negative device_id");
        if (!all_aligned({d_src, d_dst}, kPlaneAlign)) return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");
        if (tile_size > MPA_MAX_TILE_SIZE) return fail(MP_ERR_UNSUPPORTED, "tile_size above MPA_MAX_TILE_SIZE");
        const uint32_t per_tile = tile_size * tile_size;
        const uint64_t chunks = (static_cast<uint64_t>(per_tile) + CHUNK - 1) / CHUNK;
        if (chunks * std::max<uint64_t>(n, 1) > kMaxBlocks) return fail(MP_ERR_UNSUPPORTED, "too many blocks for one launch");
        if (n == 0) return MP_OK;

        DeviceScope dev;
        if (hipError_t e = dev.enter(device_id); e != hipSuccess) return hip_fail(e, "hipSetDevice");
        LaunchLog log;
        return launch(log, "move_tiles_kernel", move_tiles_kernel, dim3(static_cast<uint32_t>(chunks * n)), dim3(BLOCK), stream,
                      static_cast<const uint4*>(d_src), src_slots, d_src_slot, static_cast<uint4*>(d_dst), dst_slots, d_dst_slot,
                      per_tile, static_cast<uint32_t>(chunks));
    });
}

int mpa_finish_tiles(int device_id, uint32_t tile_size, uint32_t n_slots, uint32_t sample_count, float* d_plane,
                     const uint32_t* d_samples, const uint32_t* d_tile_wh, void* stream) {
    return guarded([&]() -> int {
        if (!d_plane || !d_samples || !d_tile_wh) return fail(MP_ERR_INVALID, "NULL argument");
        if (n_slots == 0 || tile_size == 0 || sample_count == 0) return fail(MP_ERR_INVALID, "n_slots, tile_size or sample_count is 0");
        if (device_id < 0) return fail(MP_ERR_INVALID, "negative device_id");
        if (static_cast<const void*>(d_plane) == d_samples || static_cast<const void*>(d_plane) == d_tile_wh)
            return fail(MP_ERR_INVALID, "d_plane aliases an input");
        if (!all_aligned({d_plane}, kPlaneAlign)) return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");
        if (tile_size > MPA_MAX_TILE_SIZE) return fail(MP_ERR_UNSUPPORTED, "tile_size above MPA_MAX_TILE_SIZE");
        const uint32_t per_tile = tile_size * tile_size;
        const uint64_t chunks = (static_cast<uint64_t>(per_tile) + CHUNK - 1) / CHUNK;
        if (chunks * n_slots > kMaxBlocks) return fail(MP_ERR_UNSUPPORTED, "too many blocks for one launch");

        DeviceScope dev;
        if (hipError_t e = dev.enter(device_id); e != hipSuccess) return hip_fail(e, "hipSetDevice");
        LaunchLog log;
        return launch(log, "finish_tiles_kernel", finish_tiles_kernel, dim3(static_cast<uint32_t>(chunks * n_slots)), dim3(BLOCK),
                      stream, reinterpret_cast<float4*>(d_plane), d_samples, reinterpret_cast<const uint2*>(d_tile_wh), sample_count,
                      tile_size, per_tile, static_cast<uint32_t>(chunks));
    });
}

}  // extern "C"
