// C ABI (include/minipath_hip.h): the synchronous entry points -- ray queries, tile renders, feature planes, un-tile and
// mp_render_tile -- and what every render path shares: the settings checks and the one launch of a list of tiles.
#include <cmath>
#include <cstddef>

#include "api_common.h"

namespace mp {

bool valid_settings(const mp_settings* st) {
    if (!(st && st->tile_size > 0 && st->sample_count > 0 && st->width > 0 && st->height > 0 &&
          (!(st->flags & MP_FLAG_PATHS) || st->max_depth >= 1)))
        return false;
    if ((st->flags & MP_FLAG_WAVEFRONT) && !(st->flags & MP_FLAG_PATHS)) return false;
    if (!(st->flags & MP_FLAG_ACCUMULATE)) return st->pass_begin == 0 && st->pass_count == 0;
    return st->pass_begin < st->sample_count && st->pass_count <= st->sample_count - st->pass_begin;
}

uint32_t pass_samples(const mp_settings& st) {
    if (!(st.flags & MP_FLAG_ACCUMULATE)) return st.sample_count;
    return st.pass_count ? st.pass_count : st.sample_count - st.pass_begin;
}

uint64_t reference_segments(uint64_t pixels, const mp_settings& st) { return pixels * pass_samples(st); }

int render_refusal(const mp_scene* scene, const mp_settings& st) {
    if ((st.flags & MP_FLAG_PATHS) && (st.flags & MP_FLAG_CHUNKED_SUM) && scene->dev.materials_rgb)
        return fail(MP_ERR_UNSUPPORTED, "coloured / textured materials are not combined with MP_FLAG_CHUNKED_SUM (its pixel state carries one channel)");
    if ((st.flags & MP_FLAG_PATHS) && st.max_depth > 0 && scene->dev.kind != 0u)
        return fail(MP_ERR_UNSUPPORTED, "the path extension is defined for TriangleBvh scenes only");
    return MP_OK;
}

namespace {

// The fields of a launch that the beauty render and the feature planes fill alike.  The caller adds its own: d_out, the
// traversal, the path fields and the segment counter (the feature planes leave those at their defaults and pass no d_out).
RenderLaunch shared_launch(mp_ctx* ctx, const mp_scene* scene, const mp_camera_sampler& sampler, const mp_settings& st,
                           const mp_block* d_tiles, size_t n, const uint32_t* d_tile_order, uint64_t* d_tile_cost) {
    RenderLaunch L{};
    L.scene = scene->dev;
    L.scene.packet_stack_regs = ctx->packet_stack_regs.load();
    L.packet_samples = ctx->packet_samples.load();
    L.mask_cache = ctx->mask_cache.load();
    L.sampler = sampler;
    L.width = st.width, L.height = st.height, L.spp = st.sample_count, L.tile_size = st.tile_size;
    L.seed = st.seed;
    L.d_tiles = d_tiles, L.n_tiles = static_cast<uint32_t>(n);
    L.d_counter = ctx->take_counter();
    L.cu_count = ctx->launch_cus();
    L.d_tile_order = d_tile_order;
    L.d_tile_cost = reinterpret_cast<unsigned long long*>(d_tile_cost);
    L.pass_begin = (st.flags & MP_FLAG_ACCUMULATE) ? st.pass_begin : 0u;
    L.pass_end = L.pass_begin + pass_samples(st);
    L.carry_in = L.pass_begin > 0;
    L.finalize = L.pass_end == st.sample_count;
    return L;
}

}  // namespace

int render_tiles_device(mp_ctx* ctx, const mp_scene* scene, const mp_camera_sampler& sampler, const mp_settings& st,
                        const mp_block* d_tiles, size_t n, float* d_out, void* stream, uint64_t* d_segments,
                        const uint32_t* d_tile_order, uint64_t* d_tile_cost) {
    if (int rc = render_refusal(scene, st)) return rc;
    RenderLaunch L = shared_launch(ctx, scene, sampler, st, d_tiles, n, d_tile_order, d_tile_cost);
    L.rays_per_lane = ctx->rays_per_lane.load();
    L.paths_pooled = ctx->paths_pooled.load();
    L.d_out = d_out;
    L.traversal = (st.flags & MP_FLAG_TRAVERSAL_GROUPS) ? 1 : 0;
    L.max_depth = (st.flags & MP_FLAG_PATHS) ? st.max_depth : 0u;
    L.d_segments = reinterpret_cast<unsigned long long*>(d_segments);
    L.chunked = (st.flags & MP_FLAG_CHUNKED_SUM) != 0;
    std::string err;
    int rc = (st.flags & MP_FLAG_WAVEFRONT) ? launch_render_paths_wavefront(L, stream, err) : launch_render_tiles(L, stream, err);
    if (rc) return fail(rc, err);
    return MP_OK;
}

}  // namespace mp

using namespace mp;

namespace {

// worker.rs:69-76 on the host
inline uint8_t to_u8(float c) {
    float x = std::round(c * 255.0f);
    if (x != x) return 0;
    x = x < 0.0f ? 0.0f : (x > 255.0f ? 255.0f : x);
    return static_cast<uint8_t>(x);
}

// A caller's tile list and optional hand-out order: every tile inside the frame and no larger than tile_size, the order a
// permutation (every tile is rendered exactly once).  `pixels`: what the tiles cover.
int check_tiles(const mp_settings& st, const mp_block* tiles, size_t n, const uint32_t* tile_order, uint64_t& pixels) {
    pixels = 0;
    for (size_t i = 0; i < n; i++) {
        const mp_block& t = tiles[i];
        if (!(t.min_x < t.max_x && t.min_y < t.max_y) || t.max_x - t.min_x > st.tile_size || t.max_y - t.min_y > st.tile_size ||
            t.max_x > st.width || t.max_y > st.height)
            return fail(MP_ERR_INVALID, "tile empty, larger than tile_size, or outside the resolution");
        pixels += static_cast<uint64_t>(t.max_x - t.min_x) * (t.max_y - t.min_y);
    }
    if (tile_order) {
        std::vector<bool> seen(n, false);
        for (size_t i = 0; i < n; i++) {
            if (tile_order[i] >= n || seen[tile_order[i]]) return fail(MP_ERR_INVALID, "tile_order is not a permutation of 0..n_tiles-1");
            seen[tile_order[i]] = true;
        }
    }
    return MP_OK;
}

// the checks of mp_trace_rays; exactly one of hits / d_occluded is used
int query_rays(mp_ctx* ctx, const mp_scene* scene, const float* d_ox, const float* d_oy, const float* d_oz, const float* d_dx,
               const float* d_dy, const float* d_dz, const float* d_tmax, uint64_t n, const mp_hits_soa* hits, uint8_t* d_occluded,
               void* stream) {
    DeviceGuard g(ctx->device);
    LaunchScope record(ctx);
    std::string err;
    int rc = launch_query_rays(scene->dev, d_ox, d_oy, d_oz, d_dx, d_dy, d_dz, d_tmax, n, hits, d_occluded, ctx->launch_cus(), stream, err);
    if (rc) return fail(rc, err);
    return MP_OK;
}

// First-hit feature planes (build-defined, include/minipath_hip.h): validation as mp_render_tiles_device_ex, one launch.  What the
// two entry points share, after their refusals by flag: the pass of the settings (the whole frame without MP_FLAG_ACCUMULATE).
int render_aov_planes(mp_ctx* ctx, const mp_scene* scene, const mp_camera_sampler* sampler, const mp_settings* settings,
                      const mp_block* tiles, size_t n_tiles, const mp_aov_planes_ex* planes, const mp_launch_extras* extras,
                      void* stream) {
    if (!valid_settings(settings)) return fail(MP_ERR_INVALID, "bad argument");
    if (n_tiles && !tiles) return fail(MP_ERR_INVALID, "NULL tiles");
    if (scene->ctx != ctx) return fail(MP_ERR_INVALID, "scene belongs to another context");
    if (n_tiles == 0 || !(planes->d_shade || planes->d_normal || planes->d_albedo || planes->d_ids || planes->d_position || planes->d_shade_sq)) return MP_OK;
    if (n_tiles > 0xFFFFFFFFull) return fail(MP_ERR_INVALID, "too many tiles");
    uint64_t* d_ray_segments = extras ? extras->d_ray_segments : nullptr;
    const uint32_t* tile_order = extras ? extras->tile_order : nullptr;
    uint64_t pixels;
    if (int rc = check_tiles(*settings, tiles, n_tiles, tile_order, pixels)) return rc;
    DeviceGuard g(ctx->device);
    LaunchScope record(ctx);
    const mp_block* d_tiles = nullptr;
    const uint32_t* d_order = nullptr;
    mp_ctx::TileListRef keep;  // held until the launch below is enqueued
    int rc = ctx->device_tiles(tiles, n_tiles, tile_order, keep, &d_tiles, &d_order);
    if (rc) return rc;
    std::string err;
    if (d_ray_segments) {  // one Object::intersect per sample (MP_FLAG_PATHS / max_depth: accepted and ignored)
        rc = launch_set_u64(reinterpret_cast<unsigned long long*>(d_ray_segments), reference_segments(pixels, *settings), stream, err);
        if (rc) return fail(rc, err);
    }
    RenderLaunch L = shared_launch(ctx, scene, *sampler, *settings, d_tiles, n_tiles, d_order, extras ? extras->d_tile_cost : nullptr);
    L.aov_wide_park = planes->d_position || planes->d_shade_sq;
    rc = launch_render_aov(L, *planes, stream, err);
    if (rc) return fail(rc, err);
    return MP_OK;
}

// mp_untile / mp_untile_preview after their argument checks
int untile(mp_ctx* ctx, const mp_settings* settings, const mp_block* tiles, size_t n_tiles, const float* d_tiles_f32, float* d_image_f32,
           uint8_t* d_image_u8, void* stream, uint32_t mode, uint32_t samples) {
    if (n_tiles == 0) return MP_OK;
    if (!tiles || !d_tiles_f32) return fail(MP_ERR_INVALID, "NULL tiles/input");
    if (n_tiles > 0xFFFFFFFFull) return fail(MP_ERR_INVALID, "too many tiles");
    DeviceGuard g(ctx->device);
    LaunchScope record(ctx);
    const mp_block* d_tiles = nullptr;
    mp_ctx::TileListRef keep;
    int rc = ctx->device_tiles(tiles, n_tiles, nullptr, keep, &d_tiles, nullptr);  // cached: no per-frame upload
    if (rc) return rc;
    std::string err;
    rc = launch_untile(settings->width, settings->height, settings->tile_size, d_tiles, static_cast<uint32_t>(n_tiles), d_tiles_f32,
                       d_image_f32, d_image_u8, stream, err, mode, samples);
    if (rc) fail(rc, err);
    return rc;
}

}  // namespace

extern "C" {

// ---- rays -------------------------------------------------------------------------------------------------------
int mp_trace_rays(mp_ctx* ctx, const mp_scene* scene, const float* d_ox, const float* d_oy, const float* d_oz,
                  const float* d_dx, const float* d_dy, const float* d_dz, uint64_t n, const mp_hits_soa* hits,
                  void* stream) {
    return guarded([&]() -> int {
    if (!ctx || !scene || !hits) return fail(MP_ERR_INVALID, "NULL argument");
    if (n && (!d_ox || !d_oy || !d_oz || !d_dx || !d_dy || !d_dz)) return fail(MP_ERR_INVALID, "NULL ray array");
    if (scene->ctx != ctx) return fail(MP_ERR_INVALID, "scene belongs to another context");
    DeviceGuard g(ctx->device);
    LaunchScope record(ctx);
    std::string err;
    int rc = launch_trace_rays(scene->dev, d_ox, d_oy, d_oz, d_dx, d_dy, d_dz, n, *hits, ctx->launch_cus(), stream, err);
    if (rc) return fail(rc, err);
    return MP_OK;
    });
}

int mp_trace_rays_bounded(mp_ctx* ctx, const mp_scene* scene, const float* d_ox, const float* d_oy, const float* d_oz,
                          const float* d_dx, const float* d_dy, const float* d_dz, const float* d_tmax, uint64_t n,
                          const mp_hits_soa* hits, void* stream) {
    return guarded([&]() -> int {
    if (!ctx || !scene || !hits) return fail(MP_ERR_INVALID, "NULL argument");
    if (n && (!d_ox || !d_oy || !d_oz || !d_dx || !d_dy || !d_dz)) return fail(MP_ERR_INVALID, "NULL ray array");
    if (scene->ctx != ctx) return fail(MP_ERR_INVALID, "scene belongs to another context");
    return query_rays(ctx, scene, d_ox, d_oy, d_oz, d_dx, d_dy, d_dz, d_tmax, n, hits, nullptr, stream);
    });
}

int mp_occluded_rays(mp_ctx* ctx, const mp_scene* scene, const float* d_ox, const float* d_oy, const float* d_oz,
                     const float* d_dx, const float* d_dy, const float* d_dz, const float* d_tmax, uint64_t n,
                     uint8_t* d_occluded, void* stream) {
    return guarded([&]() -> int {
    if (!ctx || !scene) return fail(MP_ERR_INVALID, "NULL argument");
    if (n && (!d_ox || !d_oy || !d_oz || !d_dx || !d_dy || !d_dz)) return fail(MP_ERR_INVALID, "NULL ray array");
    if (n && !d_occluded) return fail(MP_ERR_INVALID, "NULL output array");
    if (scene->ctx != ctx) return fail(MP_ERR_INVALID, "scene belongs to another context");
    return query_rays(ctx, scene, d_ox, d_oy, d_oz, d_dx, d_dy, d_dz, d_tmax, n, nullptr, d_occluded, stream);
    });
}

int mp_generate_rays(mp_ctx* ctx, const mp_camera_sampler* sampler, const mp_settings* settings, mp_block block,
                     uint32_t sample, float* d_ox, float* d_oy, float* d_oz, float* d_dx, float* d_dy, float* d_dz,
                     void* stream) {
    return guarded([&]() -> int {
    if (!ctx || !sampler || !valid_settings(settings)) return fail(MP_ERR_INVALID, "bad argument");
    if (!(block.min_x <= block.max_x && block.min_y <= block.max_y)) return fail(MP_ERR_INVALID, "inverted block");
    if (!d_ox || !d_oy || !d_oz || !d_dx || !d_dy || !d_dz) return fail(MP_ERR_INVALID, "NULL ray array");
    DeviceGuard g(ctx->device);
    LaunchScope record(ctx);
    std::string err;
    int rc = launch_generate_rays(*sampler, settings->width, settings->sample_count, settings->seed, block, sample, d_ox,
                                  d_oy, d_oz, d_dx, d_dy, d_dz, stream, err);
    if (rc) return fail(rc, err);
    return MP_OK;
    });
}

// ---- tiles ------------------------------------------------------------------------------------------------------
int mp_render_tiles_device(mp_ctx* ctx, const mp_scene* scene, const mp_camera_sampler* sampler,
                           const mp_settings* settings, const mp_block* tiles, size_t n_tiles, float* d_rgba_f32,
                           void* stream) {
    return mp_render_tiles_device_counted(ctx, scene, sampler, settings, tiles, n_tiles, d_rgba_f32, nullptr, stream);
}

int mp_render_tiles_device_counted(mp_ctx* ctx, const mp_scene* scene, const mp_camera_sampler* sampler,
                                   const mp_settings* settings, const mp_block* tiles, size_t n_tiles, float* d_rgba_f32,
                                   uint64_t* d_ray_segments, void* stream) {
    const mp_launch_extras ex{d_ray_segments, nullptr, nullptr};
    return mp_render_tiles_device_ex(ctx, scene, sampler, settings, tiles, n_tiles, d_rgba_f32, &ex, stream);
}

int mp_render_tiles_device_ex(mp_ctx* ctx, const mp_scene* scene, const mp_camera_sampler* sampler, const mp_settings* settings,
                              const mp_block* tiles, size_t n_tiles, float* d_rgba_f32, const mp_launch_extras* extras,
                              void* stream) {
    return guarded([&]() -> int {
    if (!ctx || !scene || !sampler || !valid_settings(settings)) return fail(MP_ERR_INVALID, "bad argument");
    if (n_tiles && (!tiles || !d_rgba_f32)) return fail(MP_ERR_INVALID, "NULL tiles/output");
    if (scene->ctx != ctx) return fail(MP_ERR_INVALID, "scene belongs to another context");
    if (n_tiles == 0) return MP_OK;
    if (n_tiles > 0xFFFFFFFFull) return fail(MP_ERR_INVALID, "too many tiles");
    uint64_t* d_ray_segments = extras ? extras->d_ray_segments : nullptr;
    uint64_t* d_tile_cost = extras ? extras->d_tile_cost : nullptr;
    const uint32_t* tile_order = extras ? extras->tile_order : nullptr;
    uint64_t pixels;
    if (int rc = check_tiles(*settings, tiles, n_tiles, tile_order, pixels)) return rc;
    DeviceGuard g(ctx->device);
    LaunchScope record(ctx);
    const mp_block* d_tiles = nullptr;
    const uint32_t* d_order = nullptr;
    mp_ctx::TileListRef keep;  // held until the launch below is enqueued
    int rc = ctx->device_tiles(tiles, n_tiles, tile_order, keep, &d_tiles, &d_order);
    if (rc) return rc;
    if (d_ray_segments) {
        // reference semantics start at their count; the path extension's kernels add their segments to 0
        const uint64_t init = (settings->flags & MP_FLAG_PATHS) ? 0 : reference_segments(pixels, *settings);
        std::string err;  // the value travels as a kernel argument: no host memory is read after this call returns
        rc = launch_set_u64(reinterpret_cast<unsigned long long*>(d_ray_segments), init, stream, err);
        if (rc) return fail(rc, err);
    }
    return render_tiles_device(ctx, scene, *sampler, *settings, d_tiles, n_tiles, d_rgba_f32, stream, d_ray_segments, d_order, d_tile_cost);
    });
}

int mp_render_aov_device(mp_ctx* ctx, const mp_scene* scene, const mp_camera_sampler* sampler, const mp_settings* settings,
                         const mp_block* tiles, size_t n_tiles, const mp_aov_planes* planes, const mp_launch_extras* extras,
                         void* stream) {
    return guarded([&]() -> int {
    if (!ctx || !scene || !sampler || !planes || !settings) return fail(MP_ERR_INVALID, "bad argument");
    if (settings->flags & (MP_FLAG_ACCUMULATE | MP_FLAG_CHUNKED_SUM))
        return fail(MP_ERR_UNSUPPORTED, "the feature planes are written by one launch over all samples: MP_FLAG_ACCUMULATE / MP_FLAG_CHUNKED_SUM are not supported");
    if (settings->flags & (MP_FLAG_WAVEFRONT | MP_FLAG_TRAVERSAL_GROUPS))
        return fail(MP_ERR_UNSUPPORTED, "the feature planes run on the packet walk: MP_FLAG_WAVEFRONT / MP_FLAG_TRAVERSAL_GROUPS are not supported");
    const mp_aov_planes_ex pl{static_cast<uint32_t>(sizeof(mp_aov_planes_ex)), planes->d_shade, planes->d_normal, planes->d_albedo, planes->d_ids, nullptr, nullptr};
    return render_aov_planes(ctx, scene, sampler, settings, tiles, n_tiles, &pl, extras, stream);
    });
}

// The planes in progressive passes, with the point and the squared shade (build-defined, include/minipath_hip.h)
int mp_render_aov_pass_device(mp_ctx* ctx, const mp_scene* scene, const mp_camera_sampler* sampler, const mp_settings* settings,
                              const mp_block* tiles, size_t n_tiles, const mp_aov_planes_ex* planes, const mp_launch_extras* extras,
                              void* stream) {
    return guarded([&]() -> int {
    if (!ctx || !scene || !sampler || !planes || !settings) return fail(MP_ERR_INVALID, "bad argument");
    if (planes->struct_size < offsetof(mp_aov_planes_ex, d_shade_sq) + sizeof(float*))
        return fail(MP_ERR_INVALID, "mp_aov_planes_ex.struct_size is smaller than the struct through d_shade_sq");
    if (settings->flags & MP_FLAG_CHUNKED_SUM)
        return fail(MP_ERR_UNSUPPORTED, "the feature planes keep plain f32 sums between passes: MP_FLAG_CHUNKED_SUM is not supported");
    if (settings->flags & (MP_FLAG_WAVEFRONT | MP_FLAG_TRAVERSAL_GROUPS))
        return fail(MP_ERR_UNSUPPORTED, "the feature planes run on the packet walk: MP_FLAG_WAVEFRONT / MP_FLAG_TRAVERSAL_GROUPS are not supported");
    return render_aov_planes(ctx, scene, sampler, settings, tiles, n_tiles, planes, extras, stream);
    });
}

uint32_t mp_aov_planes_ex_size(void) { return static_cast<uint32_t>(sizeof(mp_aov_planes_ex)); }

int mp_untile(mp_ctx* ctx, const mp_settings* settings, const mp_block* tiles, size_t n_tiles, const float* d_tiles_f32,
              float* d_image_f32, uint8_t* d_image_u8, void* stream) {
    return guarded([&]() -> int {
    if (!ctx || !valid_settings(settings)) return fail(MP_ERR_INVALID, "bad argument");
    return untile(ctx, settings, tiles, n_tiles, d_tiles_f32, d_image_f32, d_image_u8, stream, 0, 0);
    });
}

int mp_untile_preview(mp_ctx* ctx, const mp_settings* settings, const mp_block* tiles, size_t n_tiles, const float* d_tiles_f32,
                      uint32_t samples_done, float* d_image_f32, uint8_t* d_image_u8, void* stream) {
    return guarded([&]() -> int {
    if (!ctx || !valid_settings(settings)) return fail(MP_ERR_INVALID, "bad argument");
    if (samples_done == 0 || samples_done > settings->sample_count) return fail(MP_ERR_INVALID, "samples_done must be in 1..sample_count");
    // after the last sample the buffer holds the means already (the launch that reaches sample_count finalises)
    const uint32_t mode = samples_done == settings->sample_count ? 0u : ((settings->flags & MP_FLAG_CHUNKED_SUM) ? 2u : 1u);
    return untile(ctx, settings, tiles, n_tiles, d_tiles_f32, d_image_f32, d_image_u8, stream, mode, samples_done);
    });
}

int mp_render_tile(mp_ctx* ctx, const mp_scene* scene, const mp_camera_sampler* sampler, const mp_settings* settings,
                   mp_block tile, float* rgba_f32, uint8_t* rgba_u8) {
    return guarded([&]() -> int {
    if (!ctx || !scene || !sampler || !valid_settings(settings)) return fail(MP_ERR_INVALID, "bad argument");
    if (settings->flags & MP_FLAG_ACCUMULATE) return fail(MP_ERR_INVALID, "MP_FLAG_ACCUMULATE needs a caller-owned device tile buffer: use mp_render_tiles_device");
    if (!(tile.min_x < tile.max_x && tile.min_y < tile.max_y)) return MP_OK;  // empty tile: internal_points yields nothing
    const uint32_t ts = settings->tile_size;
    const uint32_t w = tile.max_x - tile.min_x, h = tile.max_y - tile.min_y;
    DeviceGuard g(ctx->device);
    LaunchScope record(ctx);
    DeviceBuffer out;
    const size_t bytes = static_cast<size_t>(ts) * ts * 16;
    MP_HIP(out.grow(bytes));
    if (int rc = mp_render_tiles_device(ctx, scene, sampler, settings, &tile, 1, out.as<float>(), nullptr)) return rc;
    std::vector<float> host(static_cast<size_t>(ts) * ts * 4);
    hipError_t e = hipMemcpy(host.data(), out.get(), bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(tile)");
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const float* p = &host[(static_cast<size_t>(y) * ts + x) * 4];
            if (rgba_f32) std::memcpy(&rgba_f32[(static_cast<size_t>(y) * w + x) * 4], p, 16);
            if (rgba_u8)
                for (int k = 0; k < 4; k++) rgba_u8[(static_cast<size_t>(y) * w + x) * 4 + k] = to_u8(p[k]);
        }
    return MP_OK;
    });
}

}  // extern "C"
