// Shading of the build-defined path extension: one path vertex (path_vertex), the texture coordinates of a hit and the
// three-channel pixel state.  Used by kernels_paths.hip (the fused kernels) and kernels_staged.hip (its vertex stage), so that both
// evaluate the very same operations, and by kernels_aov.hip for hit_tex: a change here rebuilds those three units.
#pragma once

#include "packet_walk.h"
#include "render_state.h"

namespace mp {
namespace {

// ---- build-defined path extension (MP_FLAG_PATHS; the reference has no bounce loop) -----------------
// Diffuse grey surfaces {albedo, emission} indexed by TriangleShadingData.material under a uniform sky (defaults: one material
// {0.75, 0}, sky 1), at most max_depth segments per path; the operations and their order are those of the oracle's
// render_sample_paths_impl (only + - * / sqrt and compares => bit-identical).
// Camera rays are coherent and go through the packet walk; bounce rays are incoherent: the lanes whose path is still
// alive are compacted (ballot + mbcnt) into the wave's LDS ray queue and traced by the 8-lane-group traversal.
constexpr float kPathEps = 1e-4f;

// HitRecord.texture_coords (geometry/mod.rs:78-79; BarycentricCoordinates::interpolate at ray_bvh_intersection.rs:80-83), x and y
__device__ __forceinline__ void hit_tex(const DevScene& so, uint32_t prim, float u, float v, float& tx, float& ty) {
    const uint32_t* vi = so.vidx + static_cast<size_t>(prim) * 3;
    const float *t0 = so.vtex + 3 * static_cast<size_t>(vi[0]), *t1 = so.vtex + 3 * static_cast<size_t>(vi[1]),
                *t2 = so.vtex + 3 * static_cast<size_t>(vi[2]);
    const float w = 1.0f - u - v;
    tx = t0[0] * w + t1[0] * u + t2[0] * v;
    ty = t0[1] * w + t1[1] * u + t2[1] * v;
}

// One path vertex of the build-defined extension (oracle: render_sample_paths_impl), shared by the fused and the staged kernels so
// that both evaluate the very same operations: `h` is the closest hit of segment `depth` along `r`.  Updates L / thr, and either
// ends the path (returns false) or replaces `r` by the bounce ray drawn from `rng` (returns true).
// N = colour channels carried: 3 when some material of the table is coloured or textured (DevScene::materials_rgb), else 1 -- a grey
// table makes the three channels the same number, so one is computed (same bits).  Material record = mp_material: albedo rgb,
// emission rgb, albedo2 rgb, texture, texture_scale.
template <bool OBJ, int N>
__device__ __forceinline__ bool path_vertex(const DevScene& sc, const PacketHit& h, uint32_t depth, uint32_t max_depth, Rng& rng,
                                            Ray& r, float (&L)[N], float (&thr)[N], bool& primary_hit, uint32_t inst = 0u) {
    if (h.prim == kNoPrim) {
#pragma unroll
        for (int c = 0; c < N; c++) L[c] = L[c] + thr[c] * sc.sky;
        return false;
    }
    if (depth == 1) primary_hit = true;
    float n[3];
    const uint32_t mat = OBJ ? object_normal(sc, inst, r, h.prim, h.u, h.v, n) : resolve_normal(sc, h.prim, h.u, h.v, n);
    const float* m = sc.materials + static_cast<size_t>(mat) * 12;
#pragma unroll
    for (int c = 0; c < N; c++) L[c] = L[c] + thr[c] * m[3 + c];
    const float dn = r.dx * n[0] + r.dy * n[1] + r.dz * n[2];
    if (dn > 0.0f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
    const float* alb = m;
    if (N == 3 && as_u(m[9]) == MP_TEXTURE_CHECKER) {  // reads HitRecord.texture_coords; a Sphere member's are the origin (primitives.rs:45)
        float tx = 0.0f, ty = 0.0f;
        if (OBJ) {
            DevScene so;
            object_scene(sc, inst, so);
            if (so.kind == 0u) hit_tex(so, h.prim, h.u, h.v, tx, ty);
        } else {
            hit_tex(sc, h.prim, h.u, h.v, tx, ty);
        }
        const float cell = floorf(tx * m[10]) + floorf(ty * m[10]);
        const float half = cell * 0.5f;
        if (half - floorf(half) != 0.0f) alb = m + 6;  // odd cell (NaN counts as odd): albedo2
    }
#pragma unroll
    for (int c = 0; c < N; c++) thr[c] = thr[c] * alb[c];
    if (depth == max_depth) return false;
    const float hx = r.ox + r.dx * h.t, hy = r.oy + r.dy * h.t, hz = r.oz + r.dz * h.t;  // geometry/mod.rs:56-58
    float x1, x2;
    unit_disc(rng, x1, x2);
    const float z = sqrtf(1.0f - (x1 * x1 + x2 * x2));
    const float sign = copysignf(1.0f, n[2]);
    const float a = -1.0f / (sign + n[2]);
    const float bb = n[0] * n[1] * a;
    const float t0 = 1.0f + sign * n[0] * n[0] * a, t1 = sign * bb, t2 = -sign * n[0];
    const float b0 = bb, b1 = sign + n[1] * n[1] * a, b2 = -n[1];
    ray_new(hx + n[0] * kPathEps, hy + n[1] * kPathEps, hz + n[2] * kPathEps, t0 * x1 + b0 * x2 + n[0] * z,
            t1 * x1 + b1 * x2 + n[1] * z, t2 * x1 + b2 * x2 + n[2] * z, r);
    return true;
}

// worker.rs:40-44 for three colour channels (coloured / textured material tables; never with MP_FLAG_CHUNKED_SUM): the slot holds
// {sum r, sum g, sum b, hit count} between MP_FLAG_ACCUMULATE launches
__device__ __forceinline__ void pixel_state_load3(const RenderParams& P, size_t off, bool inpix, float (&acc)[3], float& cnt) {
    acc[0] = acc[1] = acc[2] = 0.0f;
    cnt = 0.0f;
    if (P.carry_in && inpix) {
        const float4 prev = *reinterpret_cast<const float4*>(P.out + off);
        acc[0] = prev.x; acc[1] = prev.y; acc[2] = prev.z;
        cnt = prev.w;
    }
}
__device__ __forceinline__ void pixel_state_store3(const RenderParams& P, size_t off, const float (&acc)[3], float cnt) {
    const float s = P.finalize ? P.inv_spp : 1.0f;  // worker.rs:44 ; x * 1.0f is x
    *reinterpret_cast<float4*>(P.out + off) = make_float4(acc[0] * s, acc[1] * s, acc[2] * s, cnt * s);
}

}  // namespace
}  // namespace mp
