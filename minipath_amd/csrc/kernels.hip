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
// Translation units.  Every kernel family is a unit and a code object of its own, over the device headers it needs and with its own
// sub-table of kernel_table.h: kernels_tiles.hip (fused tiles), kernels_aov.hip (feature planes), kernels_paths.hip (fused paths),
// kernels_staged.hip (staged pipeline), kernels_queries.hip (ray queries).  The headers: wave_common.h and group_walk.h (all of
// them), render_state.h and packet_walk.h (the four render families), path_shading.h (paths, staged, feature planes).  This file is
// the launch unit: the launch_* entry points of mp_internal.h, which plan, return the refusal and hand the plan to the family's
// unit (family_launch.h is what the units share with it), the launch record, and the utility kernels.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "family_launch.h"
#include "wave_common.h"

namespace mp {
namespace {

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

MP_FAMILY_LAUNCHER(MP_KERNELS_UTILITIES)

}  // namespace

int check(hipError_t e, const char* what, std::string& err) {
    if (e == hipSuccess) return MP_OK;
    err = std::string(what) + ": " + hipGetErrorString(e);
    return MP_ERR_HIP;
}

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

void launch_log_clear() { t_launched.clear(); }

// the names noted since launch_log_clear() on this thread, one per line
std::string launch_log_text() {
    std::string out;
    for (KernelId id : t_launched) out += (out.empty() ? "" : "\n") + std::string(kKernelNames[id]);
    return out;
}

// the fused tiles and the fused paths share the entry point and the plan: plan_render_tiles gives a path row exactly when
// L.max_depth > 0 (launch_plan.cpp), and a unit's launch() refuses a row that is not its own
int launch_render_tiles(const RenderLaunch& L, void* stream, std::string& err) {
    if (L.n_tiles == 0) return MP_OK;
    const LaunchPlan plan = plan_render_tiles(L);
    if (plan.rc) return refused(plan, err);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return L.max_depth > 0 ? launch_paths(L, plan, st, err) : launch_tiles(L, plan, st, err);
}

// mp_render_aov_device / mp_render_aov_pass_device: samples [pass_begin, pass_end) on top of the planes' state, no path extension
int launch_render_aov(const RenderLaunch& L, const mp_aov_planes_ex& planes, void* stream, std::string& err) {
    if (L.n_tiles == 0) return MP_OK;
    const LaunchPlan plan = plan_render_aov(L);
    if (plan.rc) return refused(plan, err);
    return launch_aov(L, planes, plan, static_cast<hipStream_t>(stream), err);
}

int launch_render_paths_wavefront(const RenderLaunch& L, void* stream, std::string& err) {
    if (L.n_tiles == 0) return MP_OK;
    const WavefrontPlan plan = plan_render_paths_wavefront(L);
    if (plan.rc) return refused(plan, err);
    return launch_staged(L, plan, static_cast<hipStream_t>(stream), err);
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
// the first n counters (n <= kProfSlots, family_launch.h: every slot), summed over the units that run the cached walk, each of which counts
// into a copy of its own (prof_counters.h); reset != 0 zeroes all of them, in every unit, afterwards
extern "C" int mp_prof_read_n(unsigned long long* out, int n, int reset) {
    if (n < 0 || n > mp::kProfSlots) return 1;
    unsigned long long sum[mp::kProfSlots] = {};
    int rc = mp::prof_add_tiles(sum, reset);
    rc |= mp::prof_add_aov(sum, reset);
    rc |= mp::prof_add_paths(sum, reset);
    if (rc) return 1;
    for (int i = 0; i < n; i++) out[i] = sum[i];
    return 0;
}
#endif
