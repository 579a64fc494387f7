// Ray queries over SoA ray streams: closest hit, bounded closest hit, occlusion.
// One translation unit and one code object of libminipath_hip.so (kernel_table.h); the lane mapping and the arithmetic contract
// are described in kernels.hip.
#include "group_walk.h"
#include "family_launch.h"

namespace mp {
namespace {

// ---- batched Object::intersect over SoA ray streams (ray_bvh_intersection.rs:26-96) -------------------------
struct TraceParams {
    DevScene scene;
    const float *ox, *oy, *oz, *dx, *dy, *dz;
    uint64_t n;
    mp_hits_soa hits;
    uint32_t lds_per_wave;
};

// The stores of trace_rays_kernel's HitRecord, for query_rays_kernel.  (trace_rays_kernel keeps its own inline copy: calling these
// changes its scalar register allocation, and its code stays as measured.)
// HitRecord of a Sphere scene for ray i (primitives.rs:40-46): {t, point, normal, material 0, texture_coords origin}; a miss
// writes t = f32::MAX, MP_NO_PRIM and zeros
__device__ __forceinline__ void store_sphere_hit(const TraceParams& P, uint64_t i, const Ray& r, bool hit, float t, const float nn[3]) {
    if (P.hits.d_t) P.hits.d_t[i] = t;
    if (P.hits.d_prim) P.hits.d_prim[i] = hit ? 0u : kNoPrim;
    if (P.hits.d_u) P.hits.d_u[i] = 0.0f;
    if (P.hits.d_v) P.hits.d_v[i] = 0.0f;
    for (int k = 0; k < 3; k++) {
        const float o = k == 0 ? r.ox : k == 1 ? r.oy : r.oz, d = k == 0 ? r.dx : k == 1 ? r.dy : r.dz;
        if (P.hits.d_point) P.hits.d_point[i * 3 + k] = hit ? o + d * t : 0.0f;
        if (P.hits.d_normal) P.hits.d_normal[i * 3 + k] = hit ? nn[k] : 0.0f;
        if (P.hits.d_tex) P.hits.d_tex[i * 3 + k] = 0.0f;
    }
    if (P.hits.d_material) P.hits.d_material[i] = 0u;
    if (P.hits.d_instance) P.hits.d_instance[i] = 0u;
}

// HitRecord of ray i from the group walk's closest hit (ray_bvh_intersection.rs:66-95); a miss writes zeros beyond t / prim
template <bool OBJ>
__device__ __forceinline__ void store_group_hit(const TraceParams& P, uint64_t i, const GroupHit& gh) {
    const float t = gh.t, u = gh.u, v = gh.v;
    const uint32_t prim = gh.prim, inst = gh.inst;
    if (P.hits.d_t) P.hits.d_t[i] = t;
    if (P.hits.d_prim) P.hits.d_prim[i] = prim;
    if (P.hits.d_u) P.hits.d_u[i] = u;
    if (P.hits.d_v) P.hits.d_v[i] = v;
    if (P.hits.d_point || P.hits.d_normal || P.hits.d_tex || P.hits.d_material) {
        float pt[3] = {0, 0, 0}, nn[3] = {0, 0, 0}, tx[3] = {0, 0, 0};
        uint32_t mat = 0;  // HitRecord.material (geometry/mod.rs:78)
        if (prim != kNoPrim) {
            Ray r;  // rebuilt here so that no ray registers stay live across the walk
            ray_new(P.ox[i], P.oy[i], P.oz[i], P.dx[i], P.dy[i], P.dz[i], r);
            DevScene so = P.scene;  // the member the ray hit (its normals, texture coordinates, material ids)
            if (OBJ) object_scene(P.scene, inst, so);
            mat = OBJ ? object_normal(P.scene, inst, r, prim, u, v, nn) : resolve_normal(so, prim, u, v, nn);
            pt[0] = r.ox + r.dx * t; pt[1] = r.oy + r.dy * t; pt[2] = r.oz + r.dz * t;  // geometry/mod.rs:56-58
            if (!OBJ || so.kind == 0u) {  // a Sphere member's texture_coords are the origin (primitives.rs:45)
                const uint32_t* vi = so.vidx + static_cast<size_t>(prim) * 3;
                const float *t0 = so.vtex + 3 * static_cast<size_t>(vi[0]), *t1 = so.vtex + 3 * static_cast<size_t>(vi[1]),
                            *t2 = so.vtex + 3 * static_cast<size_t>(vi[2]);
                float w = 1.0f - u - v;
                for (int k = 0; k < 3; k++) tx[k] = t0[k] * w + t1[k] * u + t2[k] * v;
            }
        }
        for (int k = 0; k < 3; k++) {
            if (P.hits.d_point) P.hits.d_point[i * 3 + k] = pt[k];
            if (P.hits.d_normal) P.hits.d_normal[i * 3 + k] = nn[k];
            if (P.hits.d_tex) P.hits.d_tex[i * 3 + k] = tx[k];
        }
        if (P.hits.d_material) P.hits.d_material[i] = mat;
    }
    if (P.hits.d_instance) P.hits.d_instance[i] = inst;
}

template <bool OBJ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void trace_rays_kernel(TraceParams) {
    extern __shared__ __align__(16) unsigned char smem[];
    typedef const __attribute__((address_space(4))) TraceParams* ktrace_t;
    ktrace_t KP = (ktrace_t)__builtin_amdgcn_kernarg_segment_ptr();  // TraceParams through short-lived views (see params_view)
    const TraceParams& P0 = kernarg_view<TraceParams>(KP);
    const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
    float* q = reinterpret_cast<float*>(smem + static_cast<size_t>(wave) * P0.lds_per_wave);
    uint2* stack = reinterpret_cast<uint2*>(q + kQueueFloats);
    const uint64_t chunks = (P0.n + 63) / 64;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * (blockDim.x >> 6);
    for (uint64_t chunk = static_cast<uint64_t>(blockIdx.x) * (blockDim.x >> 6) + wave; chunk < chunks; chunk += stride) {
        const TraceParams& P = kernarg_view<TraceParams>(KP);  // one view per chunk of 64 rays
        const uint64_t i = chunk * 64 + lane;
        const bool act = i < P.n;
        Ray r0;
        r0.ox = r0.oy = r0.oz = r0.dx = r0.dy = r0.dz = r0.ix = r0.iy = r0.iz = 0.0f;
        if (act) ray_new(P.ox[i], P.oy[i], P.oz[i], P.dx[i], P.dy[i], P.dz[i], r0);
        if (P.scene.kind == 1u) {
            const Ray& r = r0;  // Sphere: HitRecord{t, point, normal, material 0, texture_coords origin} (primitives.rs:40-46)
            if (act) {
                float t = FLT_MAX, nn[3] = {0, 0, 0};
                const bool hit = sphere_intersect(P.scene, r, t, nn);
                if (!hit) t = FLT_MAX;
                if (P.hits.d_t) P.hits.d_t[i] = t;
                if (P.hits.d_prim) P.hits.d_prim[i] = hit ? 0u : kNoPrim;
                if (P.hits.d_u) P.hits.d_u[i] = 0.0f;
                if (P.hits.d_v) P.hits.d_v[i] = 0.0f;
                for (int k = 0; k < 3; k++) {
                    const float o = k == 0 ? r.ox : k == 1 ? r.oy : r.oz, d = k == 0 ? r.dx : k == 1 ? r.dy : r.dz;
                    if (P.hits.d_point) P.hits.d_point[i * 3 + k] = hit ? o + d * t : 0.0f;
                    if (P.hits.d_normal) P.hits.d_normal[i * 3 + k] = hit ? nn[k] : 0.0f;
                    if (P.hits.d_tex) P.hits.d_tex[i * 3 + k] = 0.0f;
                }
                if (P.hits.d_material) P.hits.d_material[i] = 0u;
                if (P.hits.d_instance) P.hits.d_instance[i] = 0u;
            }
            continue;
        }
        GroupHit gh;
        trace_objects<OBJ, true>(P.scene, r0, act, q, stack, gh);
        const float t = gh.t, u = gh.u, v = gh.v;
        const uint32_t prim = gh.prim, inst = gh.inst;
        if (act) {
            if (P.hits.d_t) P.hits.d_t[i] = t;
            if (P.hits.d_prim) P.hits.d_prim[i] = prim;
            if (P.hits.d_u) P.hits.d_u[i] = u;
            if (P.hits.d_v) P.hits.d_v[i] = v;
            if (P.hits.d_point || P.hits.d_normal || P.hits.d_tex || P.hits.d_material) {
                float pt[3] = {0, 0, 0}, nn[3] = {0, 0, 0}, tx[3] = {0, 0, 0};
                uint32_t mat = 0;  // HitRecord.material (geometry/mod.rs:78)
                if (prim != kNoPrim) {
                    Ray r;  // rebuilt here so that no ray registers stay live across the walk
                    ray_new(P.ox[i], P.oy[i], P.oz[i], P.dx[i], P.dy[i], P.dz[i], r);
                    DevScene so = P.scene;  // the member the ray hit (its normals, texture coordinates, material ids)
                    if (OBJ) object_scene(P.scene, inst, so);
                    mat = OBJ ? object_normal(P.scene, inst, r, prim, u, v, nn) : resolve_normal(so, prim, u, v, nn);
                    pt[0] = r.ox + r.dx * t; pt[1] = r.oy + r.dy * t; pt[2] = r.oz + r.dz * t;  // geometry/mod.rs:56-58
                    if (!OBJ || so.kind == 0u) {  // a Sphere member's texture_coords are the origin (primitives.rs:45)
                        const uint32_t* vi = so.vidx + static_cast<size_t>(prim) * 3;
                        const float *t0 = so.vtex + 3 * static_cast<size_t>(vi[0]), *t1 = so.vtex + 3 * static_cast<size_t>(vi[1]),
                                    *t2 = so.vtex + 3 * static_cast<size_t>(vi[2]);
                        float w = 1.0f - u - v;
                        for (int k = 0; k < 3; k++) tx[k] = t0[k] * w + t1[k] * u + t2[k] * v;
                    }
                }
                for (int k = 0; k < 3; k++) {
                    if (P.hits.d_point) P.hits.d_point[i * 3 + k] = pt[k];
                    if (P.hits.d_normal) P.hits.d_normal[i * 3 + k] = nn[k];
                    if (P.hits.d_tex) P.hits.d_tex[i * 3 + k] = tx[k];
                }
                if (P.hits.d_material) P.hits.d_material[i] = mat;
            }
            if (P.hits.d_instance) P.hits.d_instance[i] = inst;
        }
    }
}

// ---- bounded closest hit and occlusion over SoA ray streams (include/minipath_hip.h "Bounded and occlusion queries") ----------
// trace_rays_kernel with a per-ray bound b = min(tmax, f32::MAX) (d_tmax NULL: f32::MAX): MODE = kBounded writes the HitRecord of
// the walk with best.t = b (same fields, same miss record as mp_trace_rays), kAnyHit one byte per ray: 1 = that walk hits.
// A ray with NaN or non-positive tmax is a miss and is not walked.  Same grid, LDS and 8-waves-per-SIMD rules as trace_rays_kernel.
//
// Why the facts of include/minipath_hip.h hold (t* = the unbounded walk's distance, W(b) = the walk with best.t starting at b):
//  1. b = f32::MAX is the unbounded walk's own start: every push, cull, leaf test and acceptance is the same, so are the bits
//     written (the miss record included: tl = FLT_MAX, no candidate, u = v = 0, t = FLT_MAX).
//  2. The unbounded walk's best.t starts at f32::MAX >= b and never drops below t* >= b until it ends; W(b)'s never exceeds b.
//     Every slab limit and pop test of W(b) is therefore at least as strict, so W(b) visits a subset of the unbounded walk's
//     leaves, in the same relative order (children are pushed in ascending, popped in descending slot order in both).  A
//     triangle W(b) could accept has t < b <= t* and passes the leaf test in a leaf the unbounded walk visits with best.t >=
//     t* > t, which would have made its result < t*: there is none, W(b) misses.
//  3. W(b) accepts only t < b.  While W(b)'s best.t <= the unbounded walk's (true at the start), every box W(b) pushes and pops
//     the unbounded walk pushes and pops too, and every leaf both visit leaves W(b)'s best.t <= the unbounded walk's; so W(b)'s
//     result is >= t* unless the unbounded walk accepts a triangle in a leaf that W(b) culled.  That needs a triangle whose
//     distance lies below its box's floating-point entry (the band of 4), and W(b) then has to accept, in another such box,
//     a triangle below t*: two band boxes on one ray.  Outside that, t* <= t.
//  4. If b is at least the slab entry t1 of every box the ray enters, the bound b in t2 = min(exit, best.t) and in the pop
//     test removes no box that f32::MAX would keep before the first hit; from the first hit on both walks carry the same
//     best.t (the same leaves were visited with the same candidates).  So W(b) == the unbounded walk when t* < b, and a miss
//     otherwise (fact 2).
//  5. The wide tree's argument (device_tree.cpp) uses only that best.t never grows: it holds for any starting value.
// Occluded == (W(b) hits): the any-hit walk is W(b) up to its first accepting packet (best.t == b in both until then).
struct QueryParams {
    TraceParams tr;
    const float* tmax;
    uint8_t* occluded;
};

template <bool OBJ, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void query_rays_kernel(QueryParams) {
    static_assert(MODE == kBounded || MODE == kAnyHit, "a query mode");
    extern __shared__ __align__(16) unsigned char smem[];
    typedef const __attribute__((address_space(4))) QueryParams* kquery_t;
    kquery_t KP = (kquery_t)__builtin_amdgcn_kernarg_segment_ptr();  // QueryParams through short-lived views (see params_view)
    const QueryParams& P0 = kernarg_view<QueryParams>(KP);
    const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
    float* q = reinterpret_cast<float*>(smem + static_cast<size_t>(wave) * P0.tr.lds_per_wave);
    uint2* stack = reinterpret_cast<uint2*>(q + kQueueFloats);
    const uint64_t chunks = (P0.tr.n + 63) / 64;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * (blockDim.x >> 6);
    for (uint64_t chunk = static_cast<uint64_t>(blockIdx.x) * (blockDim.x >> 6) + wave; chunk < chunks; chunk += stride) {
        const QueryParams& Q = kernarg_view<QueryParams>(KP);  // one view per chunk of 64 rays
        const TraceParams& P = Q.tr;
        const uint64_t i = chunk * 64 + lane;
        const bool act = i < P.n;
        // effective bound: NaN and tmax <= 0 give b = 0 (a miss, not walked); +inf and anything above give f32::MAX
        float b = 0.0f;
        if (act) {
            const float tm = Q.tmax ? Q.tmax[i] : FLT_MAX;
            b = tm > 0.0f ? fminf(tm, FLT_MAX) : 0.0f;
        }
        const bool walk = b > 0.0f;
        Ray r0;
        r0.ox = r0.oy = r0.oz = r0.dx = r0.dy = r0.dz = r0.ix = r0.iy = r0.iz = 0.0f;
        if (walk) ray_new(P.ox[i], P.oy[i], P.oz[i], P.dx[i], P.dy[i], P.dz[i], r0);
        if (P.scene.kind == 1u) {  // Sphere: a hit counts below b (primitives.rs:16-48)
            if (act) {
                float t = FLT_MAX, nn[3] = {0, 0, 0};
                const bool hit = walk && sphere_intersect(P.scene, r0, t, nn) && t < b;
                if (!hit) t = FLT_MAX;
                if (MODE == kAnyHit) Q.occluded[i] = hit ? 1u : 0u;
                else store_sphere_hit(P, i, r0, hit, t, nn);
            }
            continue;
        }
        GroupHit gh;
        trace_objects<OBJ, true, MODE>(P.scene, r0, walk, q, stack, gh, b);
        if (act) {
            if (MODE == kAnyHit) Q.occluded[i] = gh.prim != kNoPrim ? 1u : 0u;
            else store_group_hit<OBJ>(P, i, gh);
        }
    }
}

MP_FAMILY_LAUNCHER(MP_KERNELS_QUERIES)

}  // namespace

// the three ray queries: one plan, one fill; mp_trace_rays launches on the TraceParams alone
int launch_rays(QueryKind kind, const DevScene& sc, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                const float* dz, const float* tmax, uint64_t n, const mp_hits_soa* hits, uint8_t* occluded, int cu_count, void* stream,
                std::string& err) {
    if (n == 0) return MP_OK;
    const LaunchPlan plan = plan_ray_query(sc, n, cu_count, kind);
    if (plan.rc) return refused(plan, err);
    QueryParams P;
    P.tr.scene = sc;
    P.tr.ox = ox; P.tr.oy = oy; P.tr.oz = oz; P.tr.dx = dx; P.tr.dy = dy; P.tr.dz = dz;
    P.tr.n = n;
    P.tr.hits = hits ? *hits : mp_hits_soa{};
    P.tr.lds_per_wave = plan.lds_per_wave;
    P.tmax = tmax;
    P.occluded = occluded;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (kind == kQueryClosest) return launch(plan.kernel, plan.grid, 256, plan.lds, st, err, P.tr);
    return launch(plan.kernel, plan.grid, 256, plan.lds, st, err, P);
}

}  // namespace mp
