// The selection and sizing rules of the kernel launchers (launch_plan.h).  Host arithmetic only.
#include "launch_plan.h"

#include <algorithm>

namespace mp {

#define MP_STR_(...) #__VA_ARGS__
#define MP_STR(...) MP_STR_(__VA_ARGS__)
const char* const kKernelNames[K_COUNT] = {
#define MP_X(id, ...) MP_STR(__VA_ARGS__),
    MP_KERNEL_TABLE(MP_X)
#undef MP_X
};

namespace {

constexpr uint32_t kLdsPerCu = 160u * 1024u;

uint32_t lds_bytes_per_wave(uint32_t stack_cap) { return static_cast<uint32_t>(kPlanQueueFloats * 4 + 8u * stack_cap * 8u); }

// resident blocks of 256 threads per CU for `lds` bytes of dynamic LDS each
uint32_t blocks_per_cu(uint32_t lds) { return lds ? std::max<uint32_t>(1, std::min<uint32_t>(8, kLdsPerCu / lds)) : 8u; }

template <class Plan>
Plan refuse(const char* message) {
    Plan p;
    p.rc = MP_ERR_UNSUPPORTED;
    p.error = message;
    return p;
}
constexpr const char* kTooDeepStacks = "scene too deep for the LDS traversal stacks";  // the 8-lane-group walk: queue + eight stacks per wave
constexpr const char* kTooDeepStack = "scene too deep for the LDS traversal stack";    // the packet walk's entries beyond the registers
constexpr const char* kRgbChunked = "coloured / textured materials are not combined with MP_FLAG_CHUNKED_SUM";

// What the packet render and the feature planes both read off a launch.
struct PacketFacts {
    bool obj;            // object group: one packet walk per member (instantiated for 16 and 1 samples in flight)
    bool lds_stack;      // the packet walk's stack does not fit the registers
    bool big;            // traversal arrays over 1 MB
    bool cache_ok;       // the per-unit mask cache may be used (the sample count permitting)
    bool small_launch;
    uint64_t units, want;       // 8x8-pixel work units; blocks of four waves that cover them at one unit per wave
    uint32_t stack_lds_per_wave;  // one uint4 per entry beyond the register stack
};

PacketFacts packet_facts(const RenderLaunch& L) {
    PacketFacts f;
    f.units = static_cast<uint64_t>(L.n_tiles) * ((L.tile_size + 7) / 8) * ((L.tile_size + 7) / 8);
    f.want = (f.units + 3) / 4;
    // small launches (a rank's shard of a multi-GPU frame): 2-pixel units, so that the tail of the launch is half as long
    f.small_launch = f.units * 16u < static_cast<uint64_t>(L.cu_count) * 32u * 24u;
    // scenes whose traversal arrays exceed the 16 KB scalar data cache by far run 8 waves per SIMD, and at many samples per pixel
    // 32 samples of a pixel in flight (a 1x2 pixel footprint: measured 42.1 against 42.6 ms on the metric's frame, tools/s_sweep.py)
    f.big = (static_cast<uint64_t>(L.scene.inner_count) * 256u + static_cast<uint64_t>(L.scene.packet_count) * 384u) > (1u << 20);
    f.obj = L.scene.inst_count != 0u;
    f.lds_stack = L.scene.stack_cap > L.scene.packet_stack_regs;
    // per-unit mask cache of the packet-level child rejection: stack in registers, node indices that fit the cache tag, triangle
    // coordinates within the bound of the triangle masks; 3 712 bytes of LDS per wave
    f.cache_ok = L.mask_cache != 0u && !f.lds_stack && !f.obj && L.scene.kind == 0u && L.scene.inner_count < (1u << 24) && L.scene.tris_bounded != 0u;
    f.stack_lds_per_wave = f.lds_stack ? (L.scene.stack_cap - L.scene.packet_stack_regs) * 16u : 0u;
    return f;
}

int log2_of(int s) { return s == 1 ? 0 : s == 2 ? 1 : s == 4 ? 2 : s == 8 ? 3 : s == 16 ? 4 : s == 32 ? 5 : s == 64 ? 6 : -1; }

// ---- the instantiations each rule reaches, as tables ---------------------------------------------------------------------------
// render_paths_kernel<S, OBJ, RGB>: [log2 S][obj][rgb]
constexpr KernelId kPaths[4][2][2] = {{{K_PATHS_1_GREY, K_PATHS_1_RGB}, {K_PATHS_1_OBJ_GREY, K_PATHS_1_OBJ_RGB}},
                                      {{K_PATHS_2_GREY, K_PATHS_2_RGB}, {K_PATHS_2_OBJ_GREY, K_PATHS_2_OBJ_RGB}},
                                      {{K_PATHS_4_GREY, K_PATHS_4_RGB}, {K_PATHS_4_OBJ_GREY, K_PATHS_4_OBJ_RGB}},
                                      {{K_PATHS_8_GREY, K_PATHS_8_RGB}, {K_PATHS_8_OBJ_GREY, K_PATHS_8_OBJ_RGB}}};
// render_tiles_packet_kernel<S, LDS_STACK, 7>: [log2 S][lds_stack]; <S, LDS_STACK, 8> for big scenes: [S == 32][lds_stack]
constexpr KernelId kPacket[7][2] = {{K_PACKET_1, K_PACKET_1_LDS},   {K_PACKET_2, K_PACKET_2_LDS},   {K_PACKET_4, K_PACKET_4_LDS}, {K_PACKET_8, K_PACKET_8_LDS},
                                    {K_PACKET_16, K_PACKET_16_LDS}, {K_PACKET_32, K_PACKET_32_LDS}, {K_PACKET_64, K_PACKET_64_LDS}};
constexpr KernelId kPacketBig[2][2] = {{K_PACKET_16_BIG, K_PACKET_16_BIG_LDS}, {K_PACKET_32_BIG, K_PACKET_32_BIG_LDS}};
// <S, LDS_STACK, 6, true>, object groups: [S == 16][lds_stack]
constexpr KernelId kPacketObj[2][2] = {{K_PACKET_1_OBJ, K_PACKET_1_OBJ_LDS}, {K_PACKET_16_OBJ, K_PACKET_16_OBJ_LDS}};
constexpr KernelId kAovObj[2][2] = {{K_AOV_1_OBJ, K_AOV_1_OBJ_LDS}, {K_AOV_16_OBJ, K_AOV_16_OBJ_LDS}};

LaunchPlan plan_paths(const RenderLaunch& L, const PacketFacts& f, uint32_t lds_wave, uint32_t lds) {
    LaunchPlan p;
    const uint32_t per_cu = blocks_per_cu(lds);
    const uint32_t nspp = L.pass_end - L.pass_begin;  // samples per pixel in this launch
    const int S = nspp >= 8 ? 8 : nspp >= 4 ? 4 : nspp >= 2 ? 2 : 1;  // 16 in flight measured slower here (teapot depth 8: 17.1 vs 15.7 ms)
    p.grid = static_cast<uint32_t>(std::min<uint64_t>(f.want * S, static_cast<uint64_t>(L.cu_count) * per_cu));
    p.lds = lds;
    p.lds_per_wave = lds_wave;
    const bool rgb = L.scene.materials_rgb != 0u;  // a coloured / textured material table: three channels
    if (rgb && L.chunked) return refuse<LaunchPlan>(kRgbChunked);
    // pooled form (render_paths_pooled_kernel): plain TriangleBvh scenes with a grey table, at least two passes of 8 samples.
    // By default for scenes whose traversal arrays exceed 1 MB -- there the 8-lane-group walk dominates and the longer queue
    // pays (stand-in depth 8: 564 against 628 ms); on the teapot, where most paths end after one or two segments and ray
    // generation and shading dominate, the one-pass kernel is faster (50.2 against 54.3 ms).  paths_pooled: 0 never, 1 auto,
    // 2 always with two passes, 3 always with up to four.
    const bool pooled = L.paths_pooled >= 2u || (L.paths_pooled == 1u && f.big);
    if (pooled && !rgb && !f.obj && L.max_depth >= 2 && nspp >= 16) {
        const int nsub = (nspp >= 32 && L.paths_pooled != 2u) ? 4 : 2;
        const uint32_t plds_wave = 8u * L.scene.stack_cap * 8u;  // the eight traversal stacks; the ray queue lives in the pool
        p.lds_per_wave = plds_wave;
        const uint32_t plds = plds_wave * 4u;
        if (plds > kLdsPerCu) return refuse<LaunchPlan>(kTooDeepStacks);
        p.lds = plds;
        p.grid = static_cast<uint32_t>(std::min<uint64_t>(f.want * 8, static_cast<uint64_t>(L.cu_count) * blocks_per_cu(plds)));
        p.pool_stride = kPlanPoolFloatsPerSub * static_cast<uint32_t>(nsub);
        p.pool_bytes = static_cast<size_t>(p.grid) * 4u * p.pool_stride * sizeof(float);
        p.kernel = nsub == 4 ? K_PATHS_POOLED_4 : K_PATHS_POOLED_2;
        return p;
    }
    // camera pass on the cached packet walk (MaskCache): plain scenes whose stack fits the registers, units of at least four
    // passes, and only while the cache's 3 712 bytes per wave leave the six resident waves per SIMD their LDS
    const uint32_t clds_wave = lds_wave + kPlanMaskCacheDwords * 4u;
    if (f.cache_ok && S == 8 && nspp >= 32u && L.scene.boxes_ordered != 0u && clds_wave * 4u * MP_PATHS_WPE <= kLdsPerCu) {
        p.lds_per_wave = clds_wave;
        p.lds = clds_wave * 4u;
        p.kernel = rgb ? K_PATHS_8_RGB_CACHED : K_PATHS_8_GREY_CACHED;
        return p;
    }
    p.kernel = kPaths[log2_of(S)][f.obj][rgb];  // object group: every segment is walked member by member
    return p;
}

}  // namespace

LaunchPlan plan_render_tiles(const RenderLaunch& L) {
    const PacketFacts f = packet_facts(L);
    const uint32_t glds_wave = lds_bytes_per_wave(L.scene.stack_cap);
    const uint32_t glds = glds_wave * 4;
    if (glds > kLdsPerCu) return refuse<LaunchPlan>(kTooDeepStacks);
    if (L.max_depth > 0 && L.scene.kind != 0u) return refuse<LaunchPlan>("the path extension is defined for TriangleBvh scenes only");
    if (L.max_depth > 0) return plan_paths(L, f, glds_wave, glds);  // build-defined path extension
    LaunchPlan p;
    if (L.traversal == 1) {  // MP_FLAG_TRAVERSAL_GROUPS
        p.grid = static_cast<uint32_t>(std::min<uint64_t>(f.want, static_cast<uint64_t>(L.cu_count) * 8));
        p.lds = glds;
        p.lds_per_wave = glds_wave;
        p.kernel = f.obj ? K_GROUPS_OBJ : K_GROUPS;
        return p;
    }
    // samples of one pixel in flight per pass: 16 = one DPP row per pixel (ordered sums by row_newbcast), a 2x2 pixel footprint per
    // wave and 4-pixel work units (measured best on MI355X for full frames: profiles/r01_notes.md)
    const uint32_t nspp = L.pass_end - L.pass_begin;  // samples per pixel in this launch
    int S = nspp >= 16 ? 16 : nspp >= 8 ? 8 : nspp >= 4 ? 4 : nspp >= 2 ? 2 : 1;
    if (nspp >= 32 && f.small_launch) S = 32;
    if (f.big && nspp >= 128) S = 32;
    // The per-unit mask cache (MaskCache) wants units of at least four passes: with it, the samples in flight follow the sample
    // count -- 16 from 64 spp on (metric's frame, 256 spp: 21.7 ms against 22.1 with 32; 64 spp: 6.3 against 6.4 with 8), 8 for
    // 32-63 spp (3.5 against 5.5 ms uncached at 32 spp), 4 for 16-31 (2.2 against 2.9 ms at 16 spp) -- and small launches keep
    // their 2-pixel units where those still have four passes
    if (f.cache_ok && nspp >= 16) S = (f.small_launch && nspp >= 128) ? 32 : nspp >= 64 ? 16 : nspp >= 32 ? 8 : 4;
    if (L.packet_samples) S = static_cast<int>(std::min<uint32_t>(L.packet_samples, 64u));
    if (f.obj) S = (S >= 16 && nspp >= 16) ? 16 : 1;
    p.lds_per_wave = f.stack_lds_per_wave;
    const uint32_t plds = p.lds_per_wave * 4;
    if (plds > kLdsPerCu) return refuse<LaunchPlan>(kTooDeepStack);
    if (S == 16 && L.rays_per_lane == 2 && !f.lds_stack && !f.obj && L.scene.kind == 0u && L.scene.stack_cap <= 64u) {
        // 128-ray walks: two rays per lane (8-pixel units)
        p.units2 = static_cast<uint64_t>(L.n_tiles) * ((L.tile_size + 3) / 4) * ((L.tile_size + 1) / 2);
        p.grid = static_cast<uint32_t>(std::min<uint64_t>((p.units2 + 3) / 4, static_cast<uint64_t>(L.cu_count) * 8));
        p.kernel = K_PACKET2;
        return p;
    }
    p.grid = static_cast<uint32_t>(std::min<uint64_t>(f.want * S, static_cast<uint64_t>(L.cu_count) * blocks_per_cu(plds)));
    // units of at least four passes (every scene: with the triangle masks the teapot's frame gains too -- 9.9 against 11.8 ms)
    const bool mcache = f.cache_ok && (S == 4 || S == 8 || S == 16 || S == 32) && nspp >= 4u * static_cast<uint32_t>(S);
    if (mcache) {
        p.lds = 4u * kPlanMaskCacheDwords * 4u;
        p.kernel = S == 32 ? K_PACKET_32_CACHED : S == 8 ? K_PACKET_8_CACHED : S == 4 ? K_PACKET_4_CACHED : K_PACKET_16_CACHED;
        return p;
    }
    p.lds = f.lds_stack ? plds : 0u;
    if (f.obj) p.kernel = kPacketObj[S == 16][f.lds_stack];
    else if ((S == 32 || S == 16) && f.big) p.kernel = kPacketBig[S == 32][f.lds_stack];
    else p.kernel = kPacket[std::max(0, log2_of(S))][f.lds_stack];  // a requested count that is no power of two runs one in flight
    return p;
}

// mp_render_aov_device / mp_render_aov_pass_device: the packet kernel with feature planes (render_aov_packet_kernel).  Samples in
// flight and mask cache follow plan_render_tiles' facts on a shorter list of instantiations, by the samples per pixel of THIS
// launch (a pass of a progressive frame: pass_end - pass_begin, as plan_render_tiles; the whole frame: spp): S = 16 from 16 samples
// on, 4 from 4 on, else 1; with the mask cache (same cache_ok; units of at least four passes) 16 from 64 samples on and 4 for 16-63;
// object groups and LDS-stack scenes 16 or 1.  A packet_samples_in_flight request is rounded down to these.  The parked sums take
// 32 bytes per pixel, 48 with the point or the squared shade (aov_wide_park).
LaunchPlan plan_render_aov(const RenderLaunch& L) {
    const PacketFacts f = packet_facts(L);
    LaunchPlan p;
    const uint32_t nspp = L.pass_end - L.pass_begin;  // samples per pixel in this launch
    int S = nspp >= 16 ? 16 : nspp >= 4 ? 4 : 1;
    if (f.cache_ok && nspp >= 16) S = nspp >= 64 ? 16 : 4;
    if (L.packet_samples) S = L.packet_samples >= 16u ? 16 : L.packet_samples >= 4u ? 4 : 1;
    if ((f.obj || f.lds_stack) && S == 4) S = 1;
    const bool mcache = f.cache_ok && S >= 4 && nspp >= 4u * static_cast<uint32_t>(S);
    p.lds_per_wave = f.stack_lds_per_wave;
    p.park_pixel = L.aov_wide_park ? 48u : 32u;
    const uint32_t park = 4u * (64u / static_cast<uint32_t>(S)) * p.park_pixel;  // the parked sums of the block's four waves
    p.lds = park + (mcache ? 4u * kPlanMaskCacheDwords * 4u : p.lds_per_wave * 4u);
    if (p.lds > kLdsPerCu) return refuse<LaunchPlan>(kTooDeepStack);
    p.grid = static_cast<uint32_t>(std::min<uint64_t>(f.want * S, static_cast<uint64_t>(L.cu_count) * blocks_per_cu(p.lds)));
    if (mcache) p.kernel = S == 16 ? K_AOV_16_CACHED : K_AOV_4_CACHED;
    else if (f.obj) p.kernel = kAovObj[S == 16][f.lds_stack];
    else if (f.lds_stack) p.kernel = S == 16 ? K_AOV_16_LDS : K_AOV_1_LDS;
    else p.kernel = S == 16 ? K_AOV_16 : S == 4 ? K_AOV_4 : K_AOV_1;
    return p;
}

WavefrontPlan plan_render_paths_wavefront(const RenderLaunch& L) {
    if (L.scene.kind != 0u || L.max_depth == 0)
        return refuse<WavefrontPlan>("the staged path evaluation needs MP_FLAG_PATHS and a TriangleBvh scene or an object group");
    const PacketFacts f = packet_facts(L);
    WavefrontPlan p;
    p.cam_lds_per_wave = f.stack_lds_per_wave;
    p.cam_lds = p.cam_lds_per_wave * 4;
    if (p.cam_lds > kLdsPerCu) return refuse<WavefrontPlan>(kTooDeepStack);
    p.per_cu = blocks_per_cu(p.cam_lds);
    // a batch = tb tiles x sc samples, about two million paths: enough rays per (tile, direction bin) to fill packets
    const uint32_t ts = L.tile_size, nspp = L.pass_end - L.pass_begin;
    p.sc = std::min<uint32_t>(nspp, 64u);
    p.per_tile = static_cast<uint64_t>(ts) * ts * p.sc;
    if (p.per_tile > (1ull << 28)) return refuse<WavefrontPlan>("tile_size too large for the staged path evaluation");
    p.tb = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(L.n_tiles, (1ull << 21) / p.per_tile)));
    p.n_max = static_cast<uint32_t>(p.per_tile * p.tb);
    p.nbins = p.tb * kPlanDirBins;
    // workspace: rng 32 + ray 24 + thr, L 8 (24 for three channels) + hit 16 + flags, key, idx 12 = 92 (108) bytes per path,
    // stream-ordered allocation
    p.nchan = L.scene.materials_rgb ? 3u : 1u;
    if (p.nchan == 3u && L.chunked) return refuse<WavefrontPlan>(kRgbChunked);
    p.n64 = (static_cast<size_t>(p.n_max) + 63) & ~static_cast<size_t>(63);
    p.ws_bytes = p.n64 * (88 + 8 * p.nchan) + (static_cast<size_t>(p.nbins) + 64) * 4 * 3;
    // bounce stage: LDS ray queue + eight traversal stacks per wave
    p.trace_lds_per_wave = lds_bytes_per_wave(L.scene.stack_cap);
    p.trace_lds = p.trace_lds_per_wave * 4;
    if (p.trace_lds > kLdsPerCu) return refuse<WavefrontPlan>(kTooDeepStacks);
    p.cus = static_cast<uint32_t>(L.cu_count);
    p.trace_grid = p.cus * blocks_per_cu(p.trace_lds);
    p.tile_size = ts;
    p.camera = f.obj ? (f.lds_stack ? K_WF_CAMERA_LDS_OBJ : K_WF_CAMERA_OBJ) : (f.lds_stack ? K_WF_CAMERA_LDS : K_WF_CAMERA);
    p.vertex = p.nchan == 3u ? (f.obj ? K_WF_VERTEX_RGB_OBJ : K_WF_VERTEX_RGB) : (f.obj ? K_WF_VERTEX_OBJ : K_WF_VERTEX);
    p.trace = f.obj ? K_WF_TRACE_OBJ : K_WF_TRACE;
    return p;
}

WavefrontBatch WavefrontPlan::batch(uint32_t ntb) const {
    WavefrontBatch b;
    const uint32_t ts = tile_size;
    b.n = static_cast<uint32_t>(per_tile * ntb);
    b.nbins = ntb * kPlanDirBins;
    const uint32_t units = ntb * ((ts + 1) / 2) * ((ts + 1) / 2);
    b.cam_grid = std::min<uint32_t>((units + 3) / 4, cus * per_cu);
    b.flat_grid = std::min<uint32_t>((b.n + 255u) / 256u, cus * 16u);
    b.px_grid = std::min<uint32_t>((ntb * ts * ts + 255u) / 256u, cus * 16u);
    return b;
}

// mp_trace_rays and the two bounded queries: one chunk of 64 rays per wave and turn
LaunchPlan plan_ray_query(const DevScene& sc, uint64_t n, int cu_count, QueryKind kind) {
    LaunchPlan p;
    p.lds_per_wave = lds_bytes_per_wave(sc.stack_cap);
    p.lds = p.lds_per_wave * 4;
    if (p.lds > kLdsPerCu) return refuse<LaunchPlan>(kTooDeepStacks);
    const uint64_t chunks = (n + 63) / 64, want = (chunks + 3) / 4;
    p.grid = static_cast<uint32_t>(std::min<uint64_t>(want, static_cast<uint64_t>(cu_count) * 8));
    const bool obj = sc.inst_count != 0u;
    p.kernel = kind == kQueryAnyHit ? (obj ? K_QUERY_ANY_OBJ : K_QUERY_ANY)
               : kind == kQueryBounded ? (obj ? K_QUERY_BOUNDED_OBJ : K_QUERY_BOUNDED)
                                       : (obj ? K_TRACE_OBJ : K_TRACE);
    return p;
}

}  // namespace mp
