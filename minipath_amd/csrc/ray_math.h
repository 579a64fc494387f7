// Per-ray arithmetic of ray generation and shading, written for the gfx950 issue port and bit-identical to the plain formulas:
//
//   * the seeded RNG (SplitMix64 seeding, Xoshiro256++ draws) on 32-bit halves: every 64-bit shift, rotate and add of the
//     reference formulas becomes v_alignbit_b32 / 32-bit shifts / v_add_co + v_addc (the same integer functions);
//   * Ray::new's normalisation and inverse direction through the IEEE f32 division and square-root sequences the compiler emits, minus the range fix-ups (v_div_scale, v_div_fixup, sqrt's denormal scaling
//     and zero / infinity select) -- taken only by waves whose every lane is inside a window where those fix-ups are identities.
//
// The RNG part compiles for the host as well (v_alignbit_b32 emulated), so that a host build can check it against the 64-bit
// formulas (tests/test_ray_math_cpu.py).  The division / sqrt part is device code; tests/test_ray_math_gpu.py checks it against
// `/` and sqrtf on the GPU through libmp_probe.so (probe.hip).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MP_RM_FN __host__ __device__ __forceinline__
#else
#define MP_RM_FN inline
#endif

namespace mp {
namespace rm {

// ---- 64-bit integer arithmetic on 32-bit halves --------------------------------------------------------------------------
// low word of the 64-bit funnel (hi:lo) >> s, 0 < s < 32: one v_alignbit_b32
MP_RM_FN uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, s);
#else
    return static_cast<uint32_t>(((static_cast<uint64_t>(hi) << 32) | lo) >> s);
#endif
}

struct U64 {
    uint32_t lo, hi;
};
MP_RM_FN U64 u64_split(uint64_t v) { return U64{static_cast<uint32_t>(v), static_cast<uint32_t>(v >> 32)}; }
MP_RM_FN uint64_t u64_join(U64 v) { return (static_cast<uint64_t>(v.hi) << 32) | v.lo; }
// a + b mod 2^64: v_add_co_u32 + v_addc_co_u32
MP_RM_FN U64 add64(U64 a, U64 b) {
    uint32_t lo;
    const uint32_t c = __builtin_add_overflow(a.lo, b.lo, &lo) ? 1u : 0u;
    return U64{lo, a.hi + b.hi + c};
}
// high word of a + b
MP_RM_FN uint32_t add64_hi(U64 a, U64 b) {
    uint32_t lo;
    const uint32_t c = __builtin_add_overflow(a.lo, b.lo, &lo) ? 1u : 0u;
    return a.hi + b.hi + c;
}
// x ^ (x >> K), 0 < K < 32
template <uint32_t K>
MP_RM_FN U64 xorshr64(U64 x) { return U64{x.lo ^ alignbit(x.hi, x.lo, K), x.hi ^ (x.hi >> K)}; }
// x * C mod 2^64 (one 32 x 32 -> 64 product and two low products)
template <uint64_t C>
MP_RM_FN U64 mul64(U64 x) {
    constexpr uint32_t cl = static_cast<uint32_t>(C), ch = static_cast<uint32_t>(C >> 32);
    const uint64_t p = static_cast<uint64_t>(x.lo) * cl;
    return U64{static_cast<uint32_t>(p), static_cast<uint32_t>(p >> 32) + x.lo * ch + x.hi * cl};
}

// ---- RNG: rand 0.9.3 SmallRng = Xoshiro256++, seeded by SplitMix64 (include/minipath_hip.h "Seeded mode") ----------------
struct Rng {
    U64 s0, s1, s2, s3;
};
constexpr uint64_t kGolden = 0x9e3779b97f4a7c15ull;

// SplitMix64 (state += golden; mix) -- the four draws that seed the Xoshiro state
MP_RM_FN U64 splitmix(U64& state) {
    state = add64(state, u64_split(kGolden));
    U64 z = mul64<0xbf58476d1ce4e5b9ull>(xorshr64<30>(state));
    z = mul64<0x94d049bb133111ebull>(xorshr64<27>(z));
    return xorshr64<31>(z);
}
MP_RM_FN void rng_seed(Rng& r, uint64_t key) {
    U64 k = u64_split(key);
    r.s0 = splitmix(k);
    r.s1 = splitmix(k);
    r.s2 = splitmix(k);
    r.s3 = splitmix(k);
}
// Xoshiro256++ output of the current state, high word: (rotl(s0 + s3, 23) + s0) >> 32
MP_RM_FN uint32_t rng_peek_u32(const Rng& r) {
    const U64 s = add64(r.s0, r.s3);
    const U64 rot = U64{alignbit(s.lo, s.hi, 9), alignbit(s.hi, s.lo, 9)};  // rotl 23
    return add64_hi(rot, r.s0);
}
// the state update that follows a draw
MP_RM_FN void rng_advance(Rng& r) {
    const U64 t = U64{r.s1.lo << 17, alignbit(r.s1.hi, r.s1.lo, 15)};  // s1 << 17
    r.s2.lo ^= r.s0.lo; r.s2.hi ^= r.s0.hi;
    r.s3.lo ^= r.s1.lo; r.s3.hi ^= r.s1.hi;
    r.s1.lo ^= r.s2.lo; r.s1.hi ^= r.s2.hi;
    r.s0.lo ^= r.s3.lo; r.s0.hi ^= r.s3.hi;
    r.s2.lo ^= t.lo; r.s2.hi ^= t.hi;
    r.s3 = U64{alignbit(r.s3.hi, r.s3.lo, 19), alignbit(r.s3.lo, r.s3.hi, 19)};  // rotl 45 = halves swapped, then rotl 13
}
MP_RM_FN uint32_t rng_next_u32(Rng& r) {
    const uint32_t v = rng_peek_u32(r);
    rng_advance(r);
    return v;
}
// StandardUniform f32 in [0, 1): 23 high bits of the draw as the mantissa of [1, 2), minus 1
MP_RM_FN float u32_to_01(uint32_t v) {
    union { uint32_t u; float f; } b;
    b.u = 0x3F800000u | (v >> 9);
    return b.f - 1.0f;
}
MP_RM_FN float rng_value0_1(Rng& r) { return u32_to_01(rng_next_u32(r)); }

// rand_distr::UnitDisc (camera.rs:184): rejection on two Uniform(-1, 1) draws.  ADVANCE = false leaves the stream after the
// accepted pair one update behind, for callers that draw nothing more from it: the update after the last draw is not computed.
// (ADVANCE = true keeps the plain loop: the path kernels, which go on drawing, allocate it with fewer spills.)
template <bool ADVANCE = true>
MP_RM_FN void unit_disc(Rng& rng, float& x1, float& x2) {
    if (ADVANCE) {
        for (;;) {
            x1 = rng_value0_1(rng) * 2.0f + (-1.0f);
            x2 = rng_value0_1(rng) * 2.0f + (-1.0f);
            if (x1 * x1 + x2 * x2 <= 1.0f) return;
        }
    }
    for (;;) {
        x1 = rng_value0_1(rng) * 2.0f + (-1.0f);
        x2 = u32_to_01(rng_peek_u32(rng)) * 2.0f + (-1.0f);
        if (x1 * x1 + x2 * x2 <= 1.0f) return;
        rng_advance(rng);
    }
}

// ---- the sample key, per pass from the pixel's key at sample 0 --------------------------------------------------------------
// key = seed + ((y * width + x) * spp + s), every operation in u64 mod 2^64 (include/minipath_hip.h "Seeded mode"; sample_key,
// wave_common.h).  Only s changes between the passes of a work unit, and sums associate mod 2^64, so
//     key(x, y, s) = key(x, y, 0) + s
// for every seed, image and sample index, wraps of the low word and of the whole sum included: a kernel whose lane keeps its pixel
// for a unit computes key(x, y, 0) once per unit and adds s per pass -- one add with carry (v_add_co_u32 + v_addc_co_u32) in place
// of three 64-bit multiply-adds.
MP_RM_FN uint64_t sample_key_u64(uint64_t seed, uint32_t width, uint32_t spp, uint32_t x, uint32_t y, uint32_t s) {
    return seed + ((static_cast<uint64_t>(y) * width + x) * spp + s);
}
MP_RM_FN uint64_t key_add_sample(uint64_t key0, uint32_t s) { return u64_join(add64(u64_split(key0), U64{s, 0u})); }

#if defined(__HIPCC__)
// ---- IEEE f32 division and sqrt without their range fix-ups ------------------------------------------------------------
// With f32 denormals enabled (the build's -fno-gpu-flush-denormals-to-zero), `a / b` compiles to
//     ds = v_div_scale(b, b, a); ns = v_div_scale(a, b, a); y0 = v_rcp(ds); e = fma(-ds, y0, 1); y = fma(e, y0, y0);
//     q = ns * y; r = fma(-ds, q, ns); q = fma(r, y, q); r = fma(-ds, q, ns); f = v_div_fmas(r, y, q); a / b = v_div_fixup(f, b, a)
// and sqrtf(x) to
//     x' = x < 2^-96 ? x * 2^32 : x; s = v_sqrt(x'); s- = s - 1 ulp; s+ = s + 1 ulp (integer adds on the bits);
//     s = fma(-s-, s, x') <= 0 ? s- : s; s = fma(-s+, s, x') > 0 ? s+ : s; s = x < 2^-96 ? s * 2^-16 : s; x' in {+-0, +inf} ? x' : s
// The short forms below are the same operations on the same operands with the fix-ups left out.  Where that is exact:
//
// DIVISION (V_DIV_SCALE_F32 / V_DIV_FIXUP_F32 as the CDNA4 ISA describes them).  Let a, b be finite with
//     |a| in [2^-40, 2^41) and |b| in [2^-40, 2^40]      (W)
// (so both are normal, non-zero, biased exponents 87..167).  V_DIV_SCALE leaves its operand unchanged (and VCC = 0) unless a or b is
// zero, exp(a) - exp(b) >= 96, b is denormal, 1/b or a/b is denormal, or exp(a) <= 23 (biased).  Under (W) exp(a) - exp(b) <= 80,
// 1/b lies in [2^-40, 2^40], a/b in (2^-81, 2^81), and exp(a) >= 87: none of these holds, so ds = b, ns = a, and V_DIV_FMAS with
// VCC = 0 is the plain fma.  V_DIV_FIXUP returns its first operand with its sign set to sign(a) ^ sign(b) unless an operand is NaN,
// zero or infinite, exp(a) - exp(b) < -150 or b's exponent is all ones: under (W) none holds, and f -- the correctly rounded
// quotient before the fix-up, of magnitude above 2^-81 -- already has that sign.  So div_short(a, b, div_rcp(b)) == a / b.
//   A zero numerator is left out of (W): the short form gives +0 for a = -0 (fma(-b, -0, -0) = +0, fma(+0, y, -0) = +0).
//   Reciprocal 1 / b (ns = 1.0, q = y): the same conditions with a = 1 (exp 127) hold for |b| in [2^-94, 2^125].
//
// SQRT.  For x in [2^-96, FLT_MAX] the compiler's sequence takes neither scaling branch and x is not +-0 or +inf: it is exactly
// sqrt_short(x).
__device__ __forceinline__ float div_rcp(float b) {
    const float y0 = __builtin_amdgcn_rcpf(b);
    const float e = __builtin_fmaf(-b, y0, 1.0f);
    return __builtin_fmaf(e, y0, y0);
}
__device__ __forceinline__ float div_short(float a, float b, float y) {
    float q = a * y;
    float r = __builtin_fmaf(-b, q, a);
    q = __builtin_fmaf(r, y, q);
    r = __builtin_fmaf(-b, q, a);
    return __builtin_fmaf(r, y, q);
}
__device__ __forceinline__ float rcp_short(float b) { return div_short(1.0f, b, div_rcp(b)); }
__device__ __forceinline__ float sqrt_short(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sd = __uint_as_float(__float_as_uint(s) - 1u), su = __uint_as_float(__float_as_uint(s) + 1u);
    float t = (__builtin_fmaf(-sd, s, x) <= 0.0f) ? sd : s;
    return (__builtin_fmaf(-su, s, x) > 0.0f) ? su : t;
}

// Window of a sum of three squares whose root is the divisor: x in [2^-80, 2^80) gives n = sqrt(x) in [2^-40, 2^40] (sqrt is
// correctly rounded and monotone, and 2^+-40 are exact roots).  Every component c has |c| <= sqrt(x / (1 - 2^-24)) < 2^41:
// fl(c*c) >= c*c * (1 - 2^-24) (c*c is a normal number when |c| >= 2^-40, and finite when x is) and the sum of non-negative terms
// rounds to no less than any of them.  A NaN or infinite component makes x NaN or +inf, outside the window.
constexpr float kSumLo = 0x1p-80f, kSumHi = 0x1p80f, kCompLo = 0x1p-40f;
__device__ __forceinline__ bool sum_in_window(float x) { return x >= kSumLo && x < kSumHi; }

// Ray::new (geometry/mod.rs:45-54): d = (dx, dy, dz) / |.|, inv = 1 / d with +inf for a zero component.  Returns whether the wave
// took the short sequences.  Short path, every lane: x in its window and every |component| >= 2^-40 (non-zero), so the three
// divisions are in (W); their quotients have |d| in [2^-40 / 2^40, 2^41 / 2^-40] and are never zero, so the three reciprocals are
// in their window [2^-94, 2^125] and the zero test of the inverse is false.
__device__ __forceinline__ bool ray_dir(float dx, float dy, float dz, float& ux, float& uy, float& uz, float& ix, float& iy,
                                        float& iz) {
    const float x = dx * dx + dy * dy + dz * dz;
    const bool ok = sum_in_window(x) && fminf(fminf(fabsf(dx), fabsf(dy)), fabsf(dz)) >= kCompLo;
    if (__ballot(!ok) == 0) {
        const float n = sqrt_short(x), y = div_rcp(n);
        ux = div_short(dx, n, y); uy = div_short(dy, n, y); uz = div_short(dz, n, y);
        ix = rcp_short(ux); iy = rcp_short(uy); iz = rcp_short(uz);
        return true;
    }
    const float n = sqrtf(x);
    ux = dx / n; uy = dy / n; uz = dz / n;
    ix = (ux == 0.0f) ? __builtin_inff() : 1.0f / ux;
    iy = (uy == 0.0f) ? __builtin_inff() : 1.0f / uy;
    iz = (uz == 0.0f) ? __builtin_inff() : 1.0f / uz;
    return false;
}

// A shading normal's normalisation (resolve_normal, group_walk.h): n = (nx, ny, nz) / sqrtf(nx^2 + ny^2 + nz^2).  Returns whether the
// wave took the short sequences.  Unlike a ray's direction a normal often has components that are zero, of either sign (a wall along
// an axis: the cross product's x * 0 - y * 0 is +0 or -0 by the signs of x and y), so the numerators admitted are
//     a = +-0   or   |a| in [2^-40, 2^41)      (W0)
// with the divisor as in (W): the sum x in [2^-80, 2^80), so len = sqrt_short(x) in [2^-40, 2^40] and positive; the bound |a| < 2^41
// is the window's argument above (trivial for a zero).  Non-zero numerators: (W) holds, div_short is a / len, and since len > 0 the
// quotient carries a's sign already.  Zero numerators: V_DIV_SCALE returns NaN for both scalings, and V_DIV_FIXUP, whose first test
// after the NaNs is the zero numerator over a non-zero finite divisor, returns a zero with the sign sign(a) ^ sign(len) = sign(a):
// a / len is a itself.  div_short gives +0 for either zero (the division's note above; with y > 0, a = +0: q = +0, r = (-0) + (+0)
// = +0, and every later sum is (+0) + (+0); a = -0: q = -0, r = (+0) + (-0) = +0, q = (+0) + (-0) = +0, r = (-0) + (-0) = -0, and
// the last sum is (-0) + (+0) = +0), so copying a's sign onto the short quotient (one v_bfi_b32) is the identity for a non-zero
// numerator and makes a zero one right.  A component that is neither -- non-zero below 2^-40, where the quotient may be denormal and V_DIV_SCALE rescales -- sends
// the whole wave to the plain code, like a sum outside its window (a NaN or infinite component, or all three zero).
//   The admission test on the bits: with the sign shifted out, m = bits << 1 is 0 for +-0 and monotone in |a| otherwise, so
// m - 1 (mod 2^32) >= (bits(2^-40) << 1) - 1  <=>  a = +-0 or |a| >= 2^-40 (a NaN passes here and fails the window of the sum).
__device__ __forceinline__ bool unit_normal(float nx, float ny, float nz, float n[3]) {
    const float x = nx * nx + ny * ny + nz * nz;
    constexpr uint32_t kLo2 = (0x2B800000u << 1) - 1u;  // 0x2B800000 = 2^-40
    static_assert(kCompLo == 0x1p-40f, "kLo2 is kCompLo's bit pattern, shifted");
    const uint32_t mx = (__float_as_uint(nx) << 1) - 1u, my = (__float_as_uint(ny) << 1) - 1u, mz = (__float_as_uint(nz) << 1) - 1u;
    const bool ok = sum_in_window(x) && min(min(mx, my), mz) >= kLo2;
    if (__ballot(!ok) == 0) {
        const float len = sqrt_short(x), y = div_rcp(len);
        n[0] = __builtin_copysignf(div_short(nx, len, y), nx);
        n[1] = __builtin_copysignf(div_short(ny, len, y), ny);
        n[2] = __builtin_copysignf(div_short(nz, len, y), nz);
        return true;
    }
    const float len = sqrtf(x);
    n[0] = nx / len; n[1] = ny / len; n[2] = nz / len;
    return false;
}

#endif

}  // namespace rm
}  // namespace mp
