// libmp_plan_probe.so: the launch plans (launch_plan.cpp) and the kernel table behind a C interface, for tests/test_launch_plan_cpu.py
// and tests/test_dispatch_census_cpu.py.  A test probe like libmp_rm_host.so: host code only, not part of include/minipath_hip.h.
#include <cstring>

#include "launch_plan.h"

using namespace mp;

struct mp_plan_in;
struct mp_plan_out;
// one plan into *out; *park_pixel (nullable): LaunchPlan::park_pixel
static void plan_into(int api, const mp_plan_in* in, uint64_t n_rays, bool aov_wide_park, mp_plan_out* out, uint32_t* park_pixel = nullptr);

extern "C" {

// the fields of RenderLaunch / DevScene a plan reads
struct mp_plan_in {
    uint32_t kind, inst_count, inner_count, packet_count, stack_cap, packet_stack_regs, boxes_ordered, tris_bounded, materials_rgb;
    uint32_t n_tiles, tile_size, spp, pass_begin, pass_end, cu_count, traversal, max_depth, chunked;
    uint32_t packet_samples, rays_per_lane, mask_cache, paths_pooled;
};

struct mp_plan_out {
    int32_t rc;
    char error[128];
    int32_t kernel;  // render, aov, query; staged: the camera kernel
    uint32_t grid, lds, lds_per_wave, pool_stride;
    uint64_t pool_bytes, units2;
    // staged path evaluation (api 2); the grids are those of a full batch of tb tiles
    int32_t vertex, trace;
    uint32_t trace_lds, trace_lds_per_wave, trace_grid, sc, tb, n_max, nbins, nchan, cam_grid, flat_grid, px_grid;
    uint64_t ws_bytes;
};

int mp_plan_kernel_count() { return K_COUNT; }
const char* mp_plan_kernel_name(int id) { return id >= 0 && id < K_COUNT ? kKernelNames[id] : nullptr; }

// api: 0 render tiles, 1 feature planes, 2 staged paths, 3 / 4 / 5 mp_trace_rays / bounded / occluded with n_rays rays
void mp_plan(int api, const mp_plan_in* in, uint64_t n_rays, mp_plan_out* out) { plan_into(api, in, n_rays, false, out); }

// the feature planes of mp_render_aov_pass_device: the pass [pass_begin, pass_end) of `in`; wide_park != 0: d_position or d_shade_sq
// is asked for.  *park_pixel (nullable) receives the bytes of parked sums per pixel.
void mp_plan_aov_pass(const mp_plan_in* in, int wide_park, mp_plan_out* out, uint32_t* park_pixel) {
    plan_into(1, in, 0, wide_park != 0, out, park_pixel);
}
}

static void plan_into(int api, const mp_plan_in* in, uint64_t n_rays, bool aov_wide_park, mp_plan_out* out, uint32_t* park_pixel) {
    RenderLaunch L{};
    L.aov_wide_park = aov_wide_park;
    L.scene.kind = in->kind;
    L.scene.inst_count = in->inst_count;
    L.scene.inner_count = in->inner_count;
    L.scene.packet_count = in->packet_count;
    L.scene.stack_cap = in->stack_cap;
    L.scene.packet_stack_regs = in->packet_stack_regs;
    L.scene.boxes_ordered = in->boxes_ordered;
    L.scene.tris_bounded = in->tris_bounded;
    L.scene.materials_rgb = in->materials_rgb;
    L.n_tiles = in->n_tiles;
    L.tile_size = in->tile_size;
    L.spp = in->spp;
    L.pass_begin = in->pass_begin;
    L.pass_end = in->pass_end;
    L.cu_count = static_cast<int>(in->cu_count);
    L.traversal = static_cast<int>(in->traversal);
    L.max_depth = in->max_depth;
    L.chunked = in->chunked != 0u;
    L.packet_samples = in->packet_samples;
    L.rays_per_lane = in->rays_per_lane;
    L.mask_cache = in->mask_cache;
    L.paths_pooled = in->paths_pooled;
    std::memset(out, 0, sizeof(*out));
    const char* error = nullptr;
    if (api == 2) {
        const WavefrontPlan w = plan_render_paths_wavefront(L);
        out->rc = w.rc;
        error = w.error;
        if (w.rc == MP_OK) {
            const WavefrontBatch b = w.batch(w.tb);
            out->kernel = w.camera; out->vertex = w.vertex; out->trace = w.trace;
            out->lds = w.cam_lds; out->lds_per_wave = w.cam_lds_per_wave;
            out->trace_lds = w.trace_lds; out->trace_lds_per_wave = w.trace_lds_per_wave; out->trace_grid = w.trace_grid;
            out->sc = w.sc; out->tb = w.tb; out->n_max = w.n_max; out->nbins = w.nbins; out->nchan = w.nchan;
            out->cam_grid = b.cam_grid; out->flat_grid = b.flat_grid; out->px_grid = b.px_grid;
            out->ws_bytes = w.ws_bytes;
        }
    } else {
        const LaunchPlan p = api == 0 ? plan_render_tiles(L) : api == 1 ? plan_render_aov(L)
                                                                       : plan_ray_query(L.scene, n_rays, L.cu_count, static_cast<QueryKind>(api - 3));
        out->rc = p.rc;
        error = p.error;
        out->kernel = p.kernel; out->grid = p.grid; out->lds = p.lds; out->lds_per_wave = p.lds_per_wave;
        out->pool_stride = p.pool_stride; out->pool_bytes = p.pool_bytes; out->units2 = p.units2;
        if (park_pixel) *park_pixel = p.park_pixel;
    }
    if (error) std::strncpy(out->error, error, sizeof(out->error) - 1);
}
