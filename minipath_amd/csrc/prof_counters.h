// Profiling builds only (-DMP_PROF_MISSES: the shrunk, lists_tiny and noskip test variants of the Makefile, tools/build_variant.sh):
// counters of the mask cache's slow paths, bumped by the cached packet walk (packet_walk.h), the mask cache (mask_cache.h) and the
// kernels that set a unit up.  The array lives in the anonymous namespace like all device code of the library, so every unit that
// includes the packet walk counts into a copy of its own; the units that run the cached walk (kernels_tiles.hip, kernels_aov.hip,
// kernels_paths.hip) each expose a hidden reader over prof_add_unit (family_launch.h), and mp_prof_read_n (kernels.hip) reports the
// sum.  Included before mask_cache.h, which gives MP_PROF_COUNT an empty default: packet_walk.h does that.
#pragma once

#ifdef MP_PROF_MISSES  // profiling builds only (tools/build_variant.sh): slow-path calls of the mask cache, read by mp_prof_read_n
#ifdef MP_PROF_COUNT
#error "prof_counters.h comes before mask_cache.h: include packet_walk.h first"
#endif
#include <hip/hip_runtime.h>

#include "family_launch.h"

namespace mp {
namespace {
// The slots (tests/walk_frames.py names them in this order, PROF_SLOTS):
//   [0] list builds
//   [1] leaf-mask builds
//   [2] inner links followed (with -DMP_PROF_MASK_TRIS: triangles the built leaf masks keep, leaf_mask_slow)
//   [3] bound sets
//   [4] table evictions
//   [5] arena resets
//   [6] passes left to the uncached walk
//   [7] pops skipped on an empty-mask leaf
//   [8] units that skip the per-ray scene pre-test
//   [9] units that keep it
//   [10] passes that enter the cached walk on the one bounds test (packet_walk.h, trace_packet)
//   [11] passes that enter it through the full guards
__device__ unsigned long long g_prof[12];
static_assert(sizeof(g_prof) / sizeof(g_prof[0]) == kProfSlots, "family_launch.h's count of the slots");

// host side: sum[i] += this unit's counter i, for all kProfSlots of them; reset != 0 zeroes the unit's counters afterwards
inline int prof_add_unit(unsigned long long* sum, int reset) {
    unsigned long long all[kProfSlots] = {};
    if (hipMemcpyFromSymbol(all, HIP_SYMBOL(g_prof), sizeof(all)) != hipSuccess) return 1;
    for (int i = 0; i < kProfSlots; i++) sum[i] += all[i];
    if (reset) {
        const unsigned long long z[kProfSlots] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
}  // namespace
}  // namespace mp
#define MP_PROF_COUNT(i) do { if ((threadIdx.x & 63u) == 0u) atomicAdd(&g_prof[i], 1ull); } while (0)
#endif
