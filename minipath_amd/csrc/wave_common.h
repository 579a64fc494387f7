// Device code every kernel family of libminipath_hip.so shares: small wave helpers, the 8-lane-group collectives on DPP, the RNG
// and camera ray generation (RayGen with the host code that fills it, sample_ray).  Like every device header of the library it keeps its code in the anonymous
// namespace inside mp: each family's translation unit compiles its own copy, and no device function is called across units.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdlib>

#include "launch_plan.h"
#include "mask_cache.h"
#include "mp_internal.h"
#include "ray_math.h"

namespace mp {
namespace {

// the mask-cache predicates and the per-ray helpers they share with the walk (mask_cache.h)
using namespace mc;

constexpr uint32_t kNoPrim = 0xFFFFFFFFu;
constexpr int kQueueFloats = 6 * 64;  // ox,oy,oz,dx,dy,dz (unit direction) x 64 slots ; hit (t,prim,u,v) aliases rows 0..3
static_assert(kPlanQueueFloats == kQueueFloats, "launch_plan.h sizes the launches with the device code's constants");

// set bits of a wave mask below this lane (v_mbcnt: no per-lane mask register to keep)
__device__ __forceinline__ int rank_below(uint64_t m) {
    return static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u)));
}

// Global memory written by some lanes of ONE wavefront and read by others (the pooled path kernel's ray queue): the wave's
// outstanding stores are waited for (workgroup-scope release / acquire; the vector L1 of a CU is coherent for its own waves).
__device__ __forceinline__ void wave_mem_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- 8-lane group collectives on DPP (no LDS traffic) ---------------------------------------------------------
// row_half_mirror (0x141) pairs lane i with 7-i inside every group of 8; quad_perm [1,0,3,2] (0xB1) and
// [2,3,0,1] (0x4E) finish the butterfly inside each quad.  All 8 lanes end with the group's reduction.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {
    return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, 0xF, 0xF, false));
}
// Minimum of hit distances (>= 0, possibly -0.0, never NaN): on those the signed-integer order of the bit patterns is the float
// order (-0.0 below +0.0, as v_min_f32 has it), and v_min_i32 takes the DPP operand directly (no canonicalising v_max).
__device__ __forceinline__ float group_min_t(float v) {
    int k = __float_as_int(v);
    k = min(k, __builtin_amdgcn_update_dpp(0, k, 0x141, 0xF, 0xF, false));
    k = min(k, __builtin_amdgcn_update_dpp(0, k, 0xB1, 0xF, 0xF, false));
    k = min(k, __builtin_amdgcn_update_dpp(0, k, 0x4E, 0xF, 0xF, false));
    return __int_as_float(k);
}
__device__ __forceinline__ uint32_t group_min_u(uint32_t v) {
    v = min(v, dpp_u<0x141>(v));
    v = min(v, dpp_u<0xB1>(v));
    v = min(v, dpp_u<0x4E>(v));
    return v;
}

// ---- RNG: rand 0.9.3 SmallRng = Xoshiro256++ (seeded mode, include/minipath_hip.h), on 32-bit halves (ray_math.h) -------
using rm::Rng;
using rm::rng_seed;
using rm::rng_value0_1;
using rm::unit_disc;
__device__ __forceinline__ void rng_zero(Rng& r) { r.s0 = r.s1 = r.s2 = r.s3 = rm::U64{0u, 0u}; }

struct RayGen {
    mp_camera_sampler s;
    float jitter_scale;  // UniformFloat::new_inclusive(-0.5, 0.5).scale, computed on the host
    uint32_t width, spp;
    uint64_t seed;  // mix(settings.seed), see mixed_seed()
};

// ---- host side: filling RayGen ------------------------------------------------------------------------------------
// UniformFloat::new_inclusive(low, high).scale (rand 0.9): (high-low)/max_rand, reduced by ulps until
// scale*max_rand + low <= high
float uniform_inclusive_scale(float low, float high) {
    const float max_rand = 1.0f - FLT_EPSILON;
    float scale = (high - low) / max_rand;
    for (;;) {
        volatile float top = scale * max_rand;
        top = top + low;
        if (!(top > high)) break;
        uint32_t b;
        __builtin_memcpy(&b, &scale, 4);
        b -= 1;
        __builtin_memcpy(&scale, &b, 4);
    }
    return scale;
}

// Seeded mode (include/minipath_hip.h): the first SplitMix64 output for state `seed`, so that consecutive seeds give unrelated
// sample streams; the per-sample index is added on the device (sample_key).
uint64_t mixed_seed(uint64_t seed) {
    uint64_t z = seed + 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

void fill_raygen(RayGen& G, const mp_camera_sampler& s, uint32_t width, uint32_t spp, uint64_t seed) {
    G.s = s;
    G.jitter_scale = uniform_inclusive_scale(-0.5f, 0.5f);
    G.width = width;
    G.spp = spp;
    G.seed = mixed_seed(seed);
}

// CameraSampler::sample_ray camera.rs:176-191 on an already seeded stream (ADVANCE = false: nothing is drawn from it afterwards);
// ray_new and the arithmetic from the film point on are camera_rays.h's (camera_film, camera_lens_ray): the mask cache's corner rays share it
template <bool ADVANCE = true>
__device__ __forceinline__ void sample_ray_rng(const RayGen& P, uint32_t x, uint32_t y, Rng& rng, Ray& r) {
    float film_u = static_cast<float>(x) + (rng_value0_1(rng) * P.jitter_scale + (-0.5f));
    float film_v = static_cast<float>(y) + (rng_value0_1(rng) * P.jitter_scale + (-0.5f));
    float f[3];
    camera_film(P.s, film_u, film_v, f);
    float x1, x2;
    unit_disc<ADVANCE>(rng, x1, x2);
    camera_lens_ray(P.s, f, x1, x2, r);
}

// key = mix(seed) + sample index; `P.seed` already holds mix(seed) (mixed_seed(), on the host)
__device__ __forceinline__ uint64_t sample_key(const RayGen& P, uint32_t x, uint32_t y, uint32_t sample) {
    return rm::sample_key_u64(P.seed, P.width, P.spp, x, y, sample);
}

// seeded per (pixel, sample): include/minipath_hip.h "Seeded mode"
__device__ __forceinline__ void sample_ray(const RayGen& P, uint32_t x, uint32_t y, uint32_t sample, Ray& r) {
    Rng rng;
    rng_seed(rng, sample_key(P, x, y, sample));
    sample_ray_rng<false>(P, x, y, rng, r);
}
// ... with the key handed in: the cached packet kernels form it per pass as sample_key(P, x, y, 0), computed once per work unit,
// plus the sample index (rm::key_add_sample, ray_math.h), which is the same integer as sample_key(P, x, y, sample)
__device__ __forceinline__ void sample_ray_keyed(const RayGen& P, uint32_t x, uint32_t y, uint64_t key, Ray& r) {
    Rng rng;
    rng_seed(rng, key);
    sample_ray_rng<false>(P, x, y, rng, r);
}

// A short-lived view of a kernel's arguments through the kernarg segment pointer: the compiler barrier on the pointer ends the
// life of everything loaded through the previous view (why: render_state.h, above params_view).
template <class T>
__device__ __forceinline__ const T& kernarg_view(const __attribute__((address_space(4))) T* kp) {
    asm volatile("" : "+s"(kp));
    return *(const T*)kp;
}

}  // namespace
}  // namespace mp
