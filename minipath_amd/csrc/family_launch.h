// What the translation units of libminipath_hip.so share on the host side: the one statement that launches (MP_LAUNCH, beside the
// launch record), the switch over a sub-table of kernel_table.h, which every unit expands once over the rows of its own kernels
// (MP_FAMILY_LAUNCHER), and the calls from the launch unit (kernels.hip) into the families' units.  The kernels' parameter structs
// live in the anonymous namespace (the kernels' symbol names depend on it), so a family's fill-and-launch code stands in the
// family's own unit, and only named types cross between units.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "launch_plan.h"
#include "mp_internal.h"

namespace mp {

#pragma GCC visibility push(hidden)  // between the units of the library, not part of what it exports
// kernels.hip
int check(hipError_t e, const char* what, std::string& err);
void note_launch(KernelId id);
int launched(KernelId id, std::string& err);
// The families' units fill their kernels' parameters from an accepted plan and launch: kernels_tiles.hip and kernels_paths.hip
// (behind launch_render_tiles: without and with a path extension), kernels_aov.hip (launch_render_aov), kernels_staged.hip
// (launch_render_paths_wavefront, with its workspace and its batch / chunk / depth loops)
int launch_tiles(const RenderLaunch& L, const LaunchPlan& plan, hipStream_t st, std::string& err);
int launch_paths(const RenderLaunch& L, const LaunchPlan& plan, hipStream_t st, std::string& err);
int launch_aov(const RenderLaunch& L, const mp_aov_planes_ex& planes, const LaunchPlan& plan, hipStream_t st, std::string& err);
int launch_staged(const RenderLaunch& L, const WavefrontPlan& plan, hipStream_t st, std::string& err);
// kernels_queries.hip: the three ray queries (plan, fill, launch) behind launch_trace_rays and launch_query_rays
int launch_rays(QueryKind kind, const DevScene& sc, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                const float* dz, const float* tmax, uint64_t n, const mp_hits_soa* hits, uint8_t* occluded, int cu_count, void* stream,
                std::string& err);
#ifdef MP_PROF_MISSES
// counted builds (prof_counters.h): each unit that runs the cached packet walk adds its copy of the counters to sum[0 .. kProfSlots)
// and, with reset != 0, zeroes it; mp_prof_read_n (kernels.hip) reports the sum
constexpr int kProfSlots = 12;
int prof_add_tiles(unsigned long long* sum, int reset);
int prof_add_aov(unsigned long long* sum, int reset);
int prof_add_paths(unsigned long long* sum, int reset);
#endif
#pragma GCC visibility pop

// The statement that launches is the statement that records (note_launch, kernels.hip): there is no second selection to keep in step.
#define MP_LAUNCH(id, kernel, grid, block, lds, stream, ...)               \
    do {                                                                   \
        note_launch(id);                                                   \
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__); \
    } while (0)

// launch(): launches row `id` of SUBTABLE (the including unit's rows of kernel_table.h) with these arguments.  A row whose kernel
// does not take them is not instantiated for them; an id of such a row, or of another unit's, is a programming error
// (MP_ERR_INVALID).
#define MP_LAUNCH_ROW(row, ...)                                                          \
    case row:                                                                            \
        if constexpr (std::is_invocable_v<decltype(&__VA_ARGS__), Args...>) {            \
            MP_LAUNCH(row, (__VA_ARGS__), dim3(grid), dim3(block), lds, st, args...);    \
            return launched(row, err);                                                   \
        }                                                                                \
        break;
#define MP_FAMILY_LAUNCHER(SUBTABLE)                                                                                              \
    template <class... Args>                                                                                                      \
    int launch(KernelId id, uint32_t grid, uint32_t block, uint32_t lds, hipStream_t st, std::string& err, const Args&... args) { \
        switch (id) {                                                                                                             \
            SUBTABLE(MP_LAUNCH_ROW)                                                                                               \
            default: break;                                                                                                       \
        }                                                                                                                         \
        err = "kernel table: no such kernel for these arguments";                                                                 \
        return MP_ERR_INVALID;                                                                                                    \
    }

namespace {

template <class Plan>
int refused(const Plan& plan, std::string& err) {
    err = plan.error;
    return plan.rc;
}

}  // namespace
}  // namespace mp
