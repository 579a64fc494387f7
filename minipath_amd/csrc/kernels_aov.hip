// The first-hit feature planes: the packet render with up to six planes per pixel.
// One translation unit and one code object of libminipath_hip.so (kernel_table.h); the lane mapping and the arithmetic contract
// are described in kernels.hip.
#include "packet_walk.h"
#include "render_state.h"
#include "path_shading.h"

namespace mp {
namespace {

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

MP_FAMILY_LAUNCHER(MP_KERNELS_AOV)

}  // namespace

// launch_render_aov: `plan` is plan_render_aov(L), not refused
int launch_aov(const RenderLaunch& L, const mp_aov_planes_ex& planes, const LaunchPlan& plan, hipStream_t st, std::string& err) {
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

#ifdef MP_PROF_MISSES
int prof_add_aov(unsigned long long* sum, int reset) { return prof_add_unit(sum, reset); }
#endif

}  // namespace mp
