// The 8-lane-group walk (DESIGN.md "Kernels"): a wavefront is 8 groups of 8 lanes, one ray per group, lane i owns child i of an
// inner node / triangle i of a leaf packet.  trace_wave* walk the wave's ray queue; trace_objects runs them once per member of an
// object group; normals, the sphere and the members' transforms.
#pragma once

#include "wave_common.h"

namespace mp {
namespace {

// ---- traversal --------------------------------------------------------------------------------------------------
// Lane masks straight from the compare unit (v_cmp writes the 64-bit mask; no bool -> int -> ballot round trip, which costs two
// VALU per use): LLVM CmpInst predicate numbers.
constexpr int kFcmpOGT = 2, kFcmpOGE = 3, kFcmpOLT = 4, kFcmpOLE = 5;
__device__ __forceinline__ uint64_t mask_gt(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kFcmpOGT); }
__device__ __forceinline__ uint64_t mask_lt(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kFcmpOLT); }
__device__ __forceinline__ uint64_t mask_le(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kFcmpOLE); }
__device__ __forceinline__ uint64_t mask_ge(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kFcmpOGE); }

// Traces `nrays` rays held in the wave's LDS queue `q` (rows ox,oy,oz,dx,dy,dz; slot = column).
// On return rows 0..3 of each slot hold the closest hit: t (f32::MAX on miss), prim (bits), u, v.
// impl Object for TriangleBvh::intersect, ray_bvh_intersection.rs:26-96, for 8 rays at a time.
// BFE: the count of passing children below a lane from v_bfe_u32 instead of a loop-invariant mask register (one VGPR less, one
// VALU more per node step): pays in trace_rays_kernel, which sits at the 64-VGPR cap, and costs 0.5 % in render_paths_kernel.
// QS = queue stride = ray slots.  QS == 64: the wave's LDS queue (rows ox,oy,oz,dx,dy,dz; the hit aliases rows 0..3; inverse
// directions computed here, one slot per lane).  QS > 64: the pooled path kernel's queue in global memory (rows 0..5 origin and
// direction, 6..8 inverse direction as Ray::new has it, 9..12 the hit: the rays are needed again for shading).
// MODE (ray queries, include/minipath_hip.h "Bounded and occlusion queries"; QS == 64 only): kClosest = the walk above, best.t
// starts at f32::MAX; kBounded = the same walk with best.t -- and every lane's candidate tl -- starting at the ray's bound b
// (`pb` = b of queue slot `lane`, fetched by the group that pulls the slot, like the inverse direction); kAnyHit = that walk
// ended at the first packet in which a lane accepts a triangle (t < b): row 1 of the slot then holds only prim = 0 (occluded)
// or MP_NO_PRIM.  Before its first hit the bounded walk's best.t is b, so both walks push, cull and test exactly alike up to
// that packet: occluded == (the bounded walk hits), for every ray and bound.
enum { kClosest = 0, kBounded = 1, kAnyHit = 2 };
template <bool PATCH_NAN, bool BFE, int QS = 64, int MODE = kClosest>
__device__ __forceinline__ void trace_wave_impl(const DevScene& sc, float* __restrict__ q, uint2* __restrict__ stack_base,
                                                int nrays, float pb = FLT_MAX) {
    static_assert(MODE == kClosest || QS == 64, "ray queries run on the wave's LDS queue");
    constexpr int HB = QS == 64 ? 0 : 9;  // first hit row
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int g = lane >> 3, li = lane & 7;
    uint2* stack = stack_base + g * sc.stack_cap;
    const uint32_t lanes_below = (1u << li) - 1u;

    int slot = -1, sp = 0, head = 0;
    uint32_t pk = 0, pk_end = 0, seq = 0;
    float ox = 0, oy = 0, oz = 0, dx = 0, dy = 0, dz = 0, ix = 0, iy = 0, iz = 0;
    // Lane li fetches child li / triangle li as whole 16-byte words from the AoS copies (two loads per node, three per packet)
    // PATCH_NAN = some queued ray has an infinite inverse direction component: literal reference tree; otherwise the wide tree
    // (thin nodes absorbed into their parents: same hits for finite inverses, device_tree.cpp)
    const float4* __restrict__ nodes4 = reinterpret_cast<const float4*>(PATCH_NAN ? sc.nodes_lit : sc.nodes_aos);
    const uint32_t root = PATCH_NAN ? sc.root_lit : sc.root;
    const float* __restrict__ tris = sc.tris_aos;
    float best_t = FLT_MAX;                 // best.t, group-uniform (ray_bvh_intersection.rs:34-37)
    float tl = FLT_MAX, ul = 0, vl = 0;     // this lane's earliest closest candidate
    uint32_t pkl = kNoPrim, seql = 0;
    // inv_direction as Ray::new has it (geometry/mod.rs:49-53) for the ray in queue slot `lane`, computed ONCE here for all 64
    // slots in parallel (three IEEE divisions per call instead of three per refill step); a group fetches its ray's inverse with
    // ds_bpermute when it pulls the ray.  Not queued in LDS: three rows more per wave would cost a resident wave on deep trees.
    float pix = 0.0f, piy = 0.0f, piz = 0.0f;
    if (QS == 64) {
        const float qx = q[3 * 64 + lane], qy = q[4 * 64 + lane], qz = q[5 * 64 + lane];
        pix = (qx == 0.0f) ? INFINITY : 1.0f / qx; piy = (qy == 0.0f) ? INFINITY : 1.0f / qy; piz = (qz == 0.0f) ? INFINITY : 1.0f / qz;
    }

    for (;;) {
        // -- ray finished: resolve the winner among the 8 lanes.  The reference takes candidates in (packet visit
        //    order, ascending lane) and replaces on strict `<` (:118-136, :59): the winner is the earliest candidate
        //    that attains the minimum t.  Every lane kept its own earliest minimum; ties across lanes go to the
        //    smaller (visit sequence, lane).
        if (MODE == kAnyHit && slot >= 0 && sp == 0 && pk == pk_end) {
            if (li == 0) q[1 * 64 + slot] = as_f(pkl);  // 0 = occluded (set where the walk stopped), MP_NO_PRIM = not
            slot = -1;
        }
        if (MODE != kAnyHit && slot >= 0 && sp == 0 && pk == pk_end) {
            float tmin = group_min_t(tl);
            uint32_t key = (pkl != kNoPrim && tl == tmin) ? ((seql << 3) | static_cast<uint32_t>(li)) : 0xFFFFFFFFu;
            uint32_t kmin = group_min_u(key);
            // winner's lane, recomputed from the lane id where it is needed (ds_bpermute takes a byte address: lane * 4)
            const int wl4 = (((static_cast<int>(threadIdx.x) & 56) | static_cast<int>(kmin & 7u))) << 2;
            const float wu = __int_as_float(__builtin_amdgcn_ds_bpermute(wl4, __float_as_int(ul)));
            const float wv = __int_as_float(__builtin_amdgcn_ds_bpermute(wl4, __float_as_int(vl)));
            const uint32_t wp = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(wl4, static_cast<int>(pkl)));
            if (li == 0) {
                bool hit = kmin != 0xFFFFFFFFu;
                q[(HB + 0) * QS + slot] = hit ? tmin : FLT_MAX;
                q[(HB + 1) * QS + slot] = as_f(hit ? (wp * 8u + (kmin & 7u)) : kNoPrim);
                q[(HB + 2) * QS + slot] = wu;
                q[(HB + 3) * QS + slot] = wv;
            }
            slot = -1;
        }
        // -- idle groups pull the next rays of the queue (wave-uniform head, no atomics)
        uint64_t idle = __ballot(slot < 0);
        if (idle != 0) {
            // the mask of the groups below this one is needed once per ray: recomputed here (3 VALU) rather than kept in -- or spilled
            // from -- two registers for the whole walk
            int g_ = g;
            asm volatile("" : "+v"(g_));
            const uint64_t groups_below = (1ull << (g_ * 8)) - 1ull;
            uint64_t gm = idle & 0x0101010101010101ull;
            int mine = head + __popcll(gm & groups_below);
            head += __popcll(gm);
            // (ds_bpermute reads the source lane's register whether or not that lane is enabled; an out-of-range `mine` wraps)
            float fix = 0.0f, fiy = 0.0f, fiz = 0.0f, fb = FLT_MAX;
            if (QS == 64) { fix = __shfl(pix, mine & 63); fiy = __shfl(piy, mine & 63); fiz = __shfl(piz, mine & 63); }
            if (MODE != kClosest) fb = __shfl(pb, mine & 63);
            if (slot < 0 && mine < nrays) {
                slot = mine;
                ox = q[0 * QS + mine]; oy = q[1 * QS + mine]; oz = q[2 * QS + mine];
                dx = q[3 * QS + mine]; dy = q[4 * QS + mine]; dz = q[5 * QS + mine];
                if (QS != 64) { fix = q[6 * QS + mine]; fiy = q[7 * QS + mine]; fiz = q[8 * QS + mine]; }
                ix = fix; iy = fiy; iz = fiz;
                best_t = fb; tl = fb; ul = 0; vl = 0; pkl = kNoPrim; seql = 0; seq = 0;  // :34-37, best.t = b
                pk = pk_end = 0;
                sp = 1;
                if (li == 0) stack[0] = make_uint2(root, as_u(-INFINITY));  // :28-32
            }
            if (__ballot(slot >= 0) == 0) break;
        }
        wave_lds_sync();
        // -- A: groups with no pending packet pop one stack entry (:39-62)
        if (slot >= 0 && pk == pk_end) {
            sp--;
            uint2 e = stack[sp];
            float node_t1 = as_f(e.y);
            if (!(node_t1 > best_t)) {  // :40-44
                uint32_t link = e.x;
                if ((link & 63u) == 0u) {  // device link (mp_internal.h): inner = index << 6
                    // InnerNode::intersect :149-162 ; lane li = child li.  Child boxes are stored decompressed
                    // (SURVEY A.4 box chain evaluated once on the host), so the slab test starts directly.
                    // (a uniform base + a 32-bit byte offset per lane: link = node << 6, a node is 256 bytes, a child record 32)
                    const float4* cp = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(nodes4) + ((link << 2) | (static_cast<uint32_t>(li) << 5)));
                    const float4 c0 = cp[0], c1 = cp[1];  // {min.xyz, max.x} {max.yz, link, -}
                    const uint32_t child = as_u(c1.z);
                    // aabb.rs:254-284
                    float ax = (c0.x - ox) * ix, ay = (c0.y - oy) * iy, az = (c0.z - oz) * iz;
                    float cx = (c0.w - ox) * ix, cy = (c1.x - oy) * iy, cz = (c1.y - oz) * iz;
                    // NaN (0 * inf) -> -inf on the min side, +inf on the max side (aabb.rs:262-267): maxNum / minNum return the
                    // other operand for a NaN and the value itself otherwise, one instruction each and no branch.  Only a ray with
                    // a zero direction component (infinite inverse) can produce one: queues without such a ray run the variant
                    // without the six patches (trace_wave)
                    if (PATCH_NAN) {
                        ax = fmaxf(ax, -INFINITY); ay = fmaxf(ay, -INFINITY); az = fmaxf(az, -INFINITY);
                        cx = fminf(cx, INFINITY); cy = fminf(cy, INFINITY); cz = fminf(cz, INFINITY);
                    }
                    const float t1 = fmaxf(fmaxf(fminf(ax, cx), 0.0f), fmaxf(fminf(ay, cy), fminf(az, cz)));
                    const float t2 = fminf(fminf(fmaxf(ax, cx), best_t), fminf(fmaxf(ay, cy), fmaxf(az, cz)));
                    // Null links are skipped at pop in the reference (:49).  The lane mask comes straight from the compare unit;
                    // lanes outside this branch contribute garbage bits to other groups' bytes, which are never looked at
                    const uint64_t okm = mask_le(t1, t2) & __builtin_amdgcn_uicmp(child, MP_LINK_NULL, 33);  // 33 = ICMP_NE
                    const bool ok = __builtin_amdgcn_inverse_ballot_w64(okm);
                    uint32_t m = static_cast<uint32_t>(okm >> (g * 8)) & 0xFFu;
                    const uint32_t below = BFE ? __builtin_amdgcn_ubfe(m, 0u, static_cast<uint32_t>(li)) : (m & lanes_below);
                    if (ok) stack[sp + __popc(below)] = make_uint2(child, as_u(t1));  // ascending lane :161
                    sp += __popc(m);
                } else {
                    pk = link >> 6;  // Leaf :56-62 ; device link = first packet << 6 | real triangles
                    pk_end = pk + (((link & 63u) + 7u) >> 3);
                }
            }
        }
        // -- B: one leaf packet per iteration (:104-140) ; lane li = triangle li
        if (slot >= 0 && pk < pk_end) {
            // 36-byte records: v0, e1, e2 ; a uniform base + a 32-bit byte offset per lane (fewer than 2^32 / 288 packets: upload_scene)
            const uint32_t toff = ((pk * 9u) << 5) + static_cast<uint32_t>(li) * 36u;
            const float* tp = reinterpret_cast<const float*>(reinterpret_cast<const char*>(tris) + toff);
            const float v0x = tp[0], v0y = tp[1], v0z = tp[2], e1x = tp[3], e1y = tp[4], e1z = tp[5], e2x = tp[6], e2y = tp[7], e2z = tp[8];
            // triangle.rs:183-217
            float hx = fms(dy, e2z, dz * e2y), hy = fms(dz, e2x, dx * e2z), hz = fms(dx, e2y, dy * e2x);
            float det = fma_dot(e1x, e1y, e1z, hx, hy, hz);
            float inv_det = 1.0f / det;
            float sx = ox - v0x, sy = oy - v0y, sz = oz - v0z;
            float u = inv_det * fma_dot(sx, sy, sz, hx, hy, hz);
            float qx = fms(sy, e1z, sz * e1y), qy = fms(sz, e1x, sx * e1z), qz = fms(sx, e1y, sy * e1x);
            float v = inv_det * fma_dot(dx, dy, dz, qx, qy, qz);
            float t = inv_det * fma_dot(e2x, e2y, e2z, qx, qy, qz);
            bool valid = (u >= 0.0f) & (v >= 0.0f) & ((u + v) <= 1.0f) & (t >= 0.0f) & (t <= best_t);  // :125
            if (MODE == kAnyHit) {
                // tl == best_t == b for the whole walk: a set bit in the group's byte of the ballot is :59's `hit.t < best.t` for
                // some triangle of this packet.  The ray is done: empty stack, no pending packet, the group pulls the next ray.
                if ((__ballot(valid && t < tl) >> (g * 8)) & 0xFFull) { sp = 0; pk = pk_end; pkl = 0u; }
                else pk++;
                continue;
            }
            if (valid && t < tl) { tl = t; ul = u; vl = v; pkl = pk; seql = seq; }
            seq++;
            pk++;
            if (pk == pk_end) best_t = group_min_t(tl);  // `if hit.t < best.t { best = hit }` :59-61
        }
    }
    wave_lds_sync();
}

// A queue without a ray that has an infinite inverse direction component (a zero -- or, denormals being kept, a tiny --
// direction component: geometry/mod.rs:49-53) cannot produce 0 * inf in the slab test: it runs the variant without the NaN
// patches (six VALU per node step less) on the wide tree.  Wave-uniform choice per call.
template <bool BFE = false, int MODE = kClosest>
__device__ __forceinline__ void trace_wave(const DevScene& sc, float* __restrict__ q, uint2* __restrict__ stack_base, int nrays,
                                           float pb = FLT_MAX) {
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const float qx = q[3 * 64 + lane], qy = q[4 * 64 + lane], qz = q[5 * 64 + lane];
    const float ix = (qx == 0.0f) ? INFINITY : 1.0f / qx, iy = (qy == 0.0f) ? INFINITY : 1.0f / qy, iz = (qz == 0.0f) ? INFINITY : 1.0f / qz;
    const bool inf = lane < nrays && (fabsf(ix) == INFINITY || fabsf(iy) == INFINITY || fabsf(iz) == INFINITY);
    if (__ballot(inf) != 0) trace_wave_impl<true, BFE, 64, MODE>(sc, q, stack_base, nrays, pb);
    else trace_wave_impl<false, BFE, 64, MODE>(sc, q, stack_base, nrays, pb);
}

// ... and for the pooled path kernel's queue of QS > 64 slots in global memory (inverse directions in rows 6..8)
template <int QS>
__device__ __forceinline__ void trace_wave_pool(const DevScene& sc, float* __restrict__ q, uint2* __restrict__ stack_base, int nrays) {
    int lane = static_cast<int>(threadIdx.x) & 63;
    asm volatile("" : "+v"(lane));  // (re-derived per call: the twelve row addresses below are not worth registers -- or spill slots -- across the kernel)
    bool inf = false;
#pragma unroll
    for (int k = 0; k < QS / 64; k++) {
        const int slot = lane + 64 * k;
        if (slot < nrays)
            inf = inf || fabsf(q[6 * QS + slot]) == INFINITY || fabsf(q[7 * QS + slot]) == INFINITY || fabsf(q[8 * QS + slot]) == INFINITY;
    }
    if (__ballot(inf) != 0) trace_wave_impl<true, true, QS>(sc, q, stack_base, nrays);
    else trace_wave_impl<false, true, QS>(sc, q, stack_base, nrays);
}

// Exact conservative pre-test against the union of the root node's child boxes (DevScene::pre_min/pre_max): every
// child box C lies inside that union U, and the slab interval of C is contained in the slab interval of U in
// floating point too (IEEE subtraction and multiplication are monotone, and the NaN patches of aabb.rs:262-267 map
// to the containing infinities), so a ray whose U interval is empty pushes no child of the root and is a miss.
__device__ __forceinline__ bool may_hit_scene(const DevScene& sc, const Ray& r) {
    if (!sc.has_pre) return true;
    float ax = (sc.pre_min[0] - r.ox) * r.ix, ay = (sc.pre_min[1] - r.oy) * r.iy, az = (sc.pre_min[2] - r.oz) * r.iz;
    float cx = (sc.pre_max[0] - r.ox) * r.ix, cy = (sc.pre_max[1] - r.oy) * r.iy, cz = (sc.pre_max[2] - r.oz) * r.iz;
    ax = (ax != ax) ? -INFINITY : ax; ay = (ay != ay) ? -INFINITY : ay; az = (az != az) ? -INFINITY : az;
    cx = (cx != cx) ? INFINITY : cx; cy = (cy != cy) ? INFINITY : cy; cz = (cz != cz) ? INFINITY : cz;
    float lox = fminf(ax, cx), loy = fminf(ay, cy), loz = fminf(az, cz);
    float hix = fmaxf(ax, cx), hiy = fmaxf(ay, cy), hiz = fmaxf(az, cz);
    float t1 = fmaxf(fmaxf(lox, 0.0f), fmaxf(loy, loz));
    float t2 = fminf(fminf(hix, FLT_MAX), fminf(hiy, hiz));
    return t1 <= t2;
}

// The triangle's un-normalised normal at (u, v); returns its material (below).  (Handed back through an array: with three reference
// parameters resolve_normal's callers compiled to other code -- swapped operands of an add in 64 kernels, tools/kernel_code_diff.py.)
__device__ __forceinline__ uint32_t raw_normal(const DevScene& sc, uint32_t prim, float u, float v, float raw[3]) {
    const float4* sh = reinterpret_cast<const float4*>(sc.shade) + static_cast<size_t>(prim) * 3;
    float4 a = sh[0], b = sh[1], c = sh[2];
    float nx, ny, nz;
    if (as_u(c.y) != 0u) {
        // flat: Triangle::normal (triangle.rs:141-144), unfused cross of the decompressed edges
        const float* tp = sc.tris_aos + static_cast<size_t>(prim) * kTriDwords;
        float e1x = tp[3], e1y = tp[4], e1z = tp[5], e2x = tp[6], e2y = tp[7], e2z = tp[8];
        nx = e1y * e2z - e1z * e2y;
        ny = e1z * e2x - e1x * e2z;
        nz = e1x * e2y - e1y * e2x;
    } else {
        float w = 1.0f - u - v;  // triangle.rs:235-236
        nx = a.x * w + a.w * u + b.z * v;
        ny = a.y * w + b.x * u + b.w * v;
        nz = a.z * w + b.y * u + c.x * v;
    }
    raw[0] = nx; raw[1] = ny; raw[2] = nz;
    return as_u(c.z);
}
// Hit resolve + shade: tail of intersect (ray_bvh_intersection.rs:66-95) and render_sample (worker.rs:59-65).
// Returns |dot(ray.direction, normal)|.
// Returns TriangleShadingData.material of the triangle (mod.rs:44; 0 for everything the reference builds).
__device__ __forceinline__ uint32_t resolve_normal(const DevScene& sc, uint32_t prim, float u, float v, float n[3]) {
    float raw[3];
    const uint32_t mat = raw_normal(sc, prim, u, v, raw);
    const float nx = raw[0], ny = raw[1], nz = raw[2];
    float len = sqrtf(nx * nx + ny * ny + nz * nz);
    n[0] = nx / len; n[1] = ny / len; n[2] = nz / len;
    return mat;
}
// resolve_normal as the cached packet kernels call it: the same normal, normalised by rm::unit_normal -- the short square root and
// divisions when every lane of the wave that has a hit (the lanes that call it) is inside their window (bit-identical: ray_math.h),
// the code above otherwise.  A variant of its own: the short sequences in resolve_normal itself raised the spills of
// render_paths_pooled_kernel<4> (profiles/r04_notes.md), and no kernel but the cached packet kernels is to compile differently.
__device__ __forceinline__ uint32_t resolve_normal_short(const DevScene& sc, uint32_t prim, float u, float v, float n[3]) {
    float raw[3];
    const uint32_t mat = raw_normal(sc, prim, u, v, raw);
    rm::unit_normal(raw[0], raw[1], raw[2], n);
    return mat;
}

// impl Object for Sphere::intersect, scene/primitives.rs:16-48 (lane-parallel; n = unit normal at the hit)
__device__ __forceinline__ bool sphere_intersect(const DevScene& sc, const Ray& r, float& t, float n[3]) {
    const float ocx = r.ox - sc.sphere_center[0], ocy = r.oy - sc.sphere_center[1], ocz = r.oz - sc.sphere_center[2];
    const float b = ocx * r.dx + ocy * r.dy + ocz * r.dz;
    const float c = (ocx * ocx + ocy * ocy + ocz * ocz) - sc.sphere_radius * sc.sphere_radius;
    const float disc = b * b - c;
    if (disc < 0.0f) return false;
    const float sq = sqrtf(disc);
    const float t1 = -b - sq, t2 = -b + sq;
    if (t1 > 0.0f) t = t1;
    else if (t2 > 0.0f) t = t2;
    else return false;
    const float px = r.ox + r.dx * t, py = r.oy + r.dy * t, pz = r.oz + r.dz * t;
    const float nx = px - sc.sphere_center[0], ny = py - sc.sphere_center[1], nz = pz - sc.sphere_center[2];
    const float len = sqrtf(nx * nx + ny * ny + nz * nz);
    n[0] = nx / len; n[1] = ny / len; n[2] = nz / len;
    return true;
}

// Build-defined object group (mp_scene_group / mp_scene_instances): the scene seen as member k -- the member's own traversal
// arrays under the group's material table and stack bound.  k is wave-uniform in the pass over member k (scalar loads) and per
// lane when a lane shades the member its ray hit.
__device__ __forceinline__ void object_scene(const DevScene& sc, uint32_t k, DevScene& sk) {
    sk = sc;
    const DevObject& o = sc.objects[k];
    sk.shade = o.shade; sk.nodes_aos = o.nodes_aos; sk.nodes_lit = o.nodes_lit; sk.tris_aos = o.tris_aos; sk.vidx = o.vidx; sk.vtex = o.vtex;
    sk.root = o.root; sk.root_lit = o.root_lit; sk.has_pre = o.has_pre;
    sk.kind = o.kind; sk.sphere_radius = o.sphere_radius;
    for (int i = 0; i < 3; i++) { sk.pre_min[i] = o.pre_min[i]; sk.pre_max[i] = o.pre_max[i]; sk.sphere_center[i] = o.sphere_center[i]; }
}
// UnitQuaternion * Vector3 as the oracle (and nalgebra) evaluate it: t = 2 * (qv x v); v' = t * w + (qv x t) + v, unfused
__device__ __forceinline__ void quat_rotate(float qi, float qj, float qk, float qw, float vx, float vy, float vz, float& ox,
                                            float& oy, float& oz) {
    const float tx = (qj * vz - qk * vy) * 2.0f, ty = (qk * vx - qi * vz) * 2.0f, tz = (qi * vy - qj * vx) * 2.0f;
    const float cx = qj * tz - qk * ty, cy = qk * tx - qi * tz, cz = qi * ty - qj * tx;
    ox = tx * qw + cx + vx; oy = ty * qw + cy + vy; oz = tz * qw + cz + vz;
}
// ... and the ray in member k's frame: origin - translation, then (rotated members) origin and direction through the inverse
// rotation; the direction is not re-normalised (t stays the world ray's), inv_direction by Ray::new's rule (geometry/mod.rs:49-53)
__device__ __forceinline__ void object_ray(const DevScene& sc, uint32_t k, const Ray& r, Ray& rk) {
    const DevObject& o = sc.objects[k];
    rk = r;
    rk.ox = r.ox - o.t[0]; rk.oy = r.oy - o.t[1]; rk.oz = r.oz - o.t[2];
    if (o.rotated) {
        const float qi = -o.q[0], qj = -o.q[1], qk = -o.q[2], qw = o.q[3];
        const float vx = rk.ox, vy = rk.oy, vz = rk.oz;
        quat_rotate(qi, qj, qk, qw, vx, vy, vz, rk.ox, rk.oy, rk.oz);
        quat_rotate(qi, qj, qk, qw, r.dx, r.dy, r.dz, rk.dx, rk.dy, rk.dz);
        rk.ix = (rk.dx == 0.0f) ? INFINITY : 1.0f / rk.dx;
        rk.iy = (rk.dy == 0.0f) ? INFINITY : 1.0f / rk.dy;
        rk.iz = (rk.dz == 0.0f) ? INFINITY : 1.0f / rk.dz;
    }
}

struct GroupHit {
    float t, u, v;
    uint32_t prim, inst;
};

// Closest hit of the wave's rays (one per lane, `act` = lane holds a ray) with the group walk: compaction of the lanes whose ray
// can reach the object into the wave's ray queue, trace_wave, results back to the lanes.  OBJ: once per member of the object
// group, in order, closest wins with a strict `<` (the first member keeps ties).
// MODE != kClosest (ray queries): `b` = this lane's bound (> 0, finite; include/minipath_hip.h).  Every member is walked with
// best.t = b and h.t starts at b, so a member's hit counts only below b and the combination is today's; h.t = f32::MAX again
// for a miss.  kAnyHit: a lane whose ray is occluded is not queued for later members; h.prim = 0 marks it.
template <bool OBJ, bool BFE = false, int MODE = kClosest>
__device__ __forceinline__ void trace_objects(const DevScene& sc, const Ray& r, bool act, float* __restrict__ q,
                                              uint2* __restrict__ stack, GroupHit& h, float b = FLT_MAX) {
    h.t = MODE == kClosest ? FLT_MAX : b; h.u = h.v = 0.0f; h.prim = kNoPrim; h.inst = 0u;
    auto pass = [&](const DevScene& sk, const Ray& rk, uint32_t k) {
        const bool open = act && (MODE != kAnyHit || h.prim == kNoPrim);
        if (OBJ && sk.kind == 1u) {  // a Sphere member (scene/primitives.rs:16-48): lane-parallel, no walk; prim 0
            float ts, nn[3];
            if (open && sphere_intersect(sk, rk, ts, nn) && ts < h.t) { h.t = ts; h.prim = 0u; h.u = h.v = 0.0f; h.inst = k; }
            return;
        }
        const bool queued = open && may_hit_scene(sk, rk);
        const uint64_t am = __ballot(queued);
        const int n = __popcll(am), rank = rank_below(am);
        if (queued) {
            q[0 * 64 + rank] = rk.ox; q[1 * 64 + rank] = rk.oy; q[2 * 64 + rank] = rk.oz;
            q[3 * 64 + rank] = rk.dx; q[4 * 64 + rank] = rk.dy; q[5 * 64 + rank] = rk.dz;
        }
        float pb = FLT_MAX;
        if (MODE != kClosest) {
            // the bound of queue slot `lane` into lane `lane` (ds_permute = scatter): queued lanes send to their rank, the others to
            // the slots above n, so that every lane has exactly one sender
            const int dst = queued ? rank : n + (static_cast<int>(threadIdx.x & 63) - rank);
            pb = __int_as_float(__builtin_amdgcn_ds_permute(dst << 2, __float_as_int(b)));
        }
        wave_lds_sync();
        trace_wave<BFE, MODE>(sk, q, stack, n, pb);
        if (queued) {
            const uint32_t prim = as_u(q[1 * 64 + rank]);
            if (MODE == kAnyHit) {
                if (prim != kNoPrim) { h.prim = 0u; h.inst = k; }
            } else {
                const float t = q[0 * 64 + rank];
                if (prim != kNoPrim && t < h.t) { h.t = t; h.prim = prim; h.u = q[2 * 64 + rank]; h.v = q[3 * 64 + rank]; h.inst = k; }
            }
        }
        wave_lds_sync();
    };
    if (!OBJ) {
        pass(sc, r, 0u);
    } else {
        for (uint32_t k = 0; k < sc.inst_count; k++) {
            DevScene sk;
            Ray rk;
            object_scene(sc, k, sk);
            object_ray(sc, k, r, rk);
            pass(sk, rk, k);
        }
    }
    if (MODE != kClosest && h.prim == kNoPrim) h.t = FLT_MAX;
}

// Normal and material id of a hit on member `inst` of an object group (r = the world ray).  A Sphere member's normal is that of
// its intersect, evaluated again on the ray in the member's frame (same operations, same bits); material 0 (primitives.rs:40-46).
__device__ __forceinline__ uint32_t object_normal(const DevScene& sc, uint32_t inst, const Ray& r, uint32_t prim, float u, float v,
                                                  float n[3]) {
    DevScene so;
    object_scene(sc, inst, so);
    uint32_t mat = 0u;
    if (so.kind == 1u) {
        Ray rk;
        object_ray(sc, inst, r, rk);
        float t;
        sphere_intersect(so, rk, t, n);
    } else {
        mat = resolve_normal(so, prim, u, v, n);
    }
    const DevObject& o = sc.objects[inst];
    if (o.rotated) quat_rotate(o.q[0], o.q[1], o.q[2], o.q[3], n[0], n[1], n[2], n[0], n[1], n[2]);  // back into the world frame
    return mat;
}

}  // namespace
}  // namespace mp
