// Launch plans: everything a launcher (kernels.hip and the families' units) decides and sizes before it touches the GPU -- the instantiation (an id of
// kernel_table.h), grid, dynamic LDS, lds_per_wave, pool and batch geometry, or the refusal.  Pure host code without a HIP header:
// the rules are tested on any machine through libmp_plan_probe.so (tests/test_launch_plan_cpu.py).
#pragma once

#include "kernel_table.h"
#include "mp_internal.h"

#ifndef MP_PATHS_WPE
#define MP_PATHS_WPE 6  // waves per SIMD the path kernel's registers are held to (kernels_paths.hip; A/B-measured, profiles/r03_notes.md)
#endif

namespace mp {

// Sizes of the device code the plans depend on; the header or unit that defines the device's own constant asserts each against it.
constexpr uint32_t kPlanQueueFloats = 6 * 64;       // kQueueFloats
constexpr uint32_t kPlanMaskCacheDwords = 928;      // mc::kMaskCacheDwords: 3 712 bytes per wave
constexpr uint32_t kPlanDirBins = 512;              // kDirBins
constexpr uint32_t kPlanPoolFloatsPerSub = 24 * 64; // pool_floats_per_wave(1)

extern const char* const kKernelNames[K_COUNT];

// A refused call has rc != MP_OK and the message; nothing else is meaningful then.
struct LaunchPlan {
    int rc = MP_OK;
    const char* error = nullptr;
    KernelId kernel = K_COUNT;
    uint32_t grid = 0, lds = 0;    // blocks of 256 threads, dynamic LDS bytes per block
    uint32_t lds_per_wave = 0;
    uint32_t pool_stride = 0;      // pooled path kernel: floats per wave, and the bytes of the whole pool
    size_t pool_bytes = 0;
    uint64_t units2 = 0;           // two rays per lane: 8-pixel work units of the launch
    uint32_t park_pixel = 0;       // feature planes: bytes of parked sums per pixel (32, or 48 with RenderLaunch::aov_wide_park)
};

// Staged path evaluation.  A batch is tb tiles x sc samples; the last batch of a launch may hold fewer tiles.
struct WavefrontBatch {
    uint32_t n = 0, nbins = 0;     // path slots and sort bins of a batch of ntb tiles
    uint32_t cam_grid = 0, flat_grid = 0, px_grid = 0;
};
struct WavefrontPlan {
    int rc = MP_OK;
    const char* error = nullptr;
    KernelId camera = K_COUNT, vertex = K_COUNT, trace = K_COUNT;  // scan, scatter and accumulate have one form each
    uint32_t cam_lds = 0, cam_lds_per_wave = 0;
    uint32_t trace_lds = 0, trace_lds_per_wave = 0, trace_grid = 0;
    uint32_t sc = 0, tb = 0, n_max = 0, nbins = 0, nchan = 0;
    uint64_t per_tile = 0;
    size_t n64 = 0, ws_bytes = 0;
    WavefrontBatch batch(uint32_t ntb) const;
    // set by the plan for batch()
    uint32_t tile_size = 0, cus = 0, per_cu = 0;
};

LaunchPlan plan_render_tiles(const RenderLaunch& L);
LaunchPlan plan_render_aov(const RenderLaunch& L);
WavefrontPlan plan_render_paths_wavefront(const RenderLaunch& L);
enum QueryKind { kQueryClosest = 0, kQueryBounded = 1, kQueryAnyHit = 2 };  // mp_trace_rays, mp_trace_rays_bounded, mp_occluded_rays
LaunchPlan plan_ray_query(const DevScene& sc, uint64_t n, int cu_count, QueryKind kind);

}  // namespace mp
