// libmp_probe.so: test probes of ray_math.h on the GPU (tests/test_ray_math_gpu.py, tests/test_short_normal_gpu.py), built with the library's flags.  Each entry
// point launches kernels that compare a short sequence of ray_math.h with the compiler's `/` / sqrtf bit for bit and returns
// counters: out[0] = mismatches, out[1] = cases compared, out[2] = smallest mismatching case index (~0 if none), out[3] = waves
// that took the short path (ray and normal probes).  The kernels write nothing but these four counters.  The return value is 0 or the HIP error
// code of the first call that failed.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "ray_math.h"

namespace {

using namespace mp::rm;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
// A wave's mismatches with one atomic: its lowest mismatching lane (the wave's smallest case index) adds the count and keeps the index.
// Called by every lane of the wave.
__device__ __forceinline__ void record(unsigned long long* out, bool bad, uint64_t idx) {
    const uint64_t m = __ballot(bad);
    if (m == 0) return;
    if (static_cast<int>(threadIdx.x & 63) == __ffsll(static_cast<unsigned long long>(m)) - 1) {
        atomicAdd(out + 0, static_cast<unsigned long long>(__popcll(m)));
        atomicMin(out + 2, static_cast<unsigned long long>(idx));
    }
}
__device__ __forceinline__ bool differ(float a, float b) { return __float_as_uint(a) != __float_as_uint(b); }

// every f32 bit pattern base + thread: op 0 = sqrt_short against sqrtf on [2^-96, FLT_MAX], op 1 = rcp_short against 1 / x on
// |x| in [2^-94, 2^125] (the windows of ray_math.h's argument)
__global__ void unary_kernel(int op, uint64_t base, unsigned long long* out) {
    const uint64_t idx = base + static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const float x = __uint_as_float(static_cast<uint32_t>(idx));
    bool in, bad = false;
    if (op == 0) {
        in = x >= 0x1p-96f && x <= FLT_MAX;
        if (in) bad = differ(sqrt_short(x), sqrtf(x));
    } else {
        in = fabsf(x) >= 0x1p-94f && fabsf(x) <= 0x1p125f;
        if (in) bad = differ(rcp_short(x), 1.0f / x);
    }
    const uint64_t n = __popcll(__ballot(in));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(out + 1, n);
    record(out, bad, idx);
}

// a float with a random mantissa and sign and a biased exponent in [elo, ehi]; one draw in four at an end of the range, one in
// eight with an extreme mantissa
__device__ __forceinline__ float pick(uint64_t h, uint32_t elo, uint32_t ehi) {
    const uint32_t sel = static_cast<uint32_t>(h >> 56);
    uint32_t e = elo + static_cast<uint32_t>((h >> 32) & 0xFFFFu) % (ehi - elo + 1u);
    if ((sel & 3u) == 0u) e = (sel & 4u) ? ehi : elo;
    uint32_t m = static_cast<uint32_t>(h) & 0x7FFFFFu;
    if ((sel & 0x38u) == 0u) m = (sel & 0x40u) ? 0x7FFFFFu : 0u;
    return __uint_as_float(((sel & 0x80u) << 24) | (e << 23) | m);
}

// PAIRS pairs per thread in the division window (W): |a| in [2^-40, 2^41), |b| in [2^-40, 2^40]; pair index = thread * PAIRS + k,
// thread = base + global thread id
template <int PAIRS>
__global__ void div_kernel(uint64_t seed, uint64_t base, unsigned long long* out) {
    const uint64_t t = base + static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    for (int k = 0; k < PAIRS; k++) {
        const uint64_t idx = t * PAIRS + k;
        const uint64_t h1 = mix64(seed ^ (idx * 2 + 0)), h2 = mix64(seed ^ (idx * 2 + 1));
        const float a = pick(h1, 127 - 40, 127 + 40);
        float b = pick(h2, 127 - 40, 127 + 39);
        if ((h2 & 0xF00u) == 0u) b = __uint_as_float((__float_as_uint(b) & 0x80000000u) | (127u + 40u) << 23);  // 2^40 itself
        record(out, differ(div_short(a, b, div_rcp(b)), a / b), idx);
    }
    if ((threadIdx.x & 63) == 0) atomicAdd(out + 1, 64ull * PAIRS);
}

// one direction per lane, as ray_new takes it; mode 0: components of magnitude 2^-40 .. 2^38 (every wave short); mode 1: as 0, but
// in every odd wave one lane carries a zero, -0, denormal, tiny, huge, infinite or NaN component (those waves fall back);
// mode 2: components of random bits.  ray_dir against the plain Ray::new formulas, all six outputs.
__global__ void ray_kernel(uint64_t seed, int mode, unsigned long long* out) {
    const uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t wave = idx >> 6;
    const int lane = static_cast<int>(idx & 63);
    float d[3];
    for (int c = 0; c < 3; c++) {
        const uint64_t h = mix64(seed ^ (idx * 4 + c));
        d[c] = mode == 2 ? __uint_as_float(static_cast<uint32_t>(h)) : pick(h, 127 - 40, 127 + 38);
    }
    if (mode == 1 && (wave & 1u) && lane == static_cast<int>(mix64(seed ^ wave) & 63u)) {
        // +0, -0, denormal, tiny, huge, +inf, NaN, tiny negative (selected, not indexed: no private array)
        const uint32_t k = static_cast<uint32_t>(wave >> 1) & 7u;
        const float v = k == 0 ? 0.0f : k == 1 ? -0.0f : k == 2 ? 0x1p-140f : k == 3 ? 0x1p-41f : k == 4 ? 0x1p45f
                      : k == 5 ? __builtin_inff() : k == 6 ? __builtin_nanf("") : -0x1p-100f;
        const int c = static_cast<int>((wave >> 1) % 3);
        if (c == 0) d[0] = v; else if (c == 1) d[1] = v; else d[2] = v;
    }
    float ux, uy, uz, ix, iy, iz;
    const bool fast = ray_dir(d[0], d[1], d[2], ux, uy, uz, ix, iy, iz);
    const float n = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const float rx = d[0] / n, ry = d[1] / n, rz = d[2] / n;
    const float rix = (rx == 0.0f) ? __builtin_inff() : 1.0f / rx, riy = (ry == 0.0f) ? __builtin_inff() : 1.0f / ry,
                riz = (rz == 0.0f) ? __builtin_inff() : 1.0f / rz;
    const bool bad = differ(ux, rx) || differ(uy, ry) || differ(uz, rz) || differ(ix, rix) || differ(iy, riy) || differ(iz, riz);
    record(out, bad, idx);
    if (lane == 0) {
        atomicAdd(out + 1, 64ull);
        if (fast) atomicAdd(out + 3, 1ull);
    }
}

// one shading normal per lane, as resolve_normal_short hands it to unit_normal; mode 0: components of magnitude 2^-40 .. 2^38 (every
// wave short); mode 1: as 0 with components replaced by +0 or -0, one in three each, but never all three of a lane (walls along
// the axes: every wave short); mode 2: as 1, but in every odd wave one lane carries a denormal, tiny, huge, infinite or NaN
// component or is zero in all three (those waves fall back); mode 3: components of random bits.  unit_normal against sqrtf and
// the three `/`, all three outputs.
__global__ void normal_kernel(uint64_t seed, int mode, unsigned long long* out) {
    const uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t wave = idx >> 6;
    const int lane = static_cast<int>(idx & 63);
    float d[3];
    for (int c = 0; c < 3; c++) {
        const uint64_t h = mix64(seed ^ (idx * 4 + c));
        d[c] = mode == 3 ? __uint_as_float(static_cast<uint32_t>(h)) : pick(h, 127 - 40, 127 + 38);
    }
    if (mode == 1 || mode == 2) {
        const uint64_t z = mix64(seed ^ (idx * 4 + 3));
        const uint32_t keep = static_cast<uint32_t>(z >> 32) % 3u;  // this component stays as it is
        for (int c = 0; c < 3; c++) {
            const uint32_t sel = static_cast<uint32_t>(z >> (8 * c)) % 3u;  // 0: +0, 1: -0, 2: unchanged
            if (static_cast<uint32_t>(c) != keep && sel != 2u) d[c] = sel == 0u ? 0.0f : -0.0f;
        }
    }
    if (mode == 2 && (wave & 1u) && lane == static_cast<int>(mix64(seed ^ wave) & 63u)) {
        // denormal, tiny, tiny negative, huge, +inf, -inf, NaN in one component; or all three zero (selected, not indexed: no private array)
        const uint32_t k = static_cast<uint32_t>(wave >> 1) & 7u;
        const float v = k == 0 ? 0x1p-140f : k == 1 ? 0x1p-41f : k == 2 ? -0x1p-100f : k == 3 ? 0x1p45f : k == 4 ? __builtin_inff()
                      : k == 5 ? -__builtin_inff() : __builtin_nanf("");
        const int c = static_cast<int>((wave >> 4) % 3);
        if (k == 7u) { d[0] = 0.0f; d[1] = -0.0f; d[2] = 0.0f; }
        else if (c == 0) d[0] = v; else if (c == 1) d[1] = v; else d[2] = v;
    }
    float n[3];
    const bool fast = unit_normal(d[0], d[1], d[2], n);
    const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const bool bad = differ(n[0], d[0] / len) || differ(n[1], d[1] / len) || differ(n[2], d[2] / len);
    record(out, bad, idx);
    if (lane == 0) {
        atomicAdd(out + 1, 64ull);
        if (fast) atomicAdd(out + 3, 1ull);
    }
}

// One launch on a fresh counter buffer.  HIP's last-error state is per thread and sticky: an error that earlier work of the process
// left there (any library, any earlier call whose status nobody read) is not this probe's, so it is cleared before the launch, and
// every call's own status is checked.
int run(void (*launch)(unsigned long long*), unsigned long long* host) {
    (void)hipGetLastError();
    unsigned long long* dev = nullptr;
    unsigned long long init[4] = {0ull, 0ull, ~0ull, 0ull};
    hipError_t e = hipMalloc(&dev, sizeof(init));
    if (e != hipSuccess) return static_cast<int>(e);
    e = hipMemcpy(dev, init, sizeof(init), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch(dev);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(host, dev, sizeof(init), hipMemcpyDeviceToHost);
    }
    const hipError_t ef = hipFree(dev);
    return static_cast<int>(e != hipSuccess ? e : ef);
}
void merge(unsigned long long* acc, const unsigned long long* r) {
    acc[0] += r[0]; acc[1] += r[1]; acc[3] += r[3];
    if (r[2] < acc[2]) acc[2] = r[2];
}

int g_op, g_mode;
uint64_t g_seed, g_base, g_blocks;
constexpr int kDivPairs = 64;
constexpr uint64_t kDivBlocksPerLaunch = 4096;  // 2^26 pairs per launch

}  // namespace

extern "C" {
// all 2^32 bit patterns (op 0: sqrt, 1: reciprocal), in four launches of 2^30
int mp_probe_unary(int op, unsigned long long* out) {
    g_op = op;
    unsigned long long acc[4] = {0ull, 0ull, ~0ull, 0ull};
    for (uint64_t q = 0; q < 4; q++) {
        unsigned long long r[4];
        g_seed = q << 30;
        if (int rc = run([](unsigned long long* d) { hipLaunchKernelGGL(unary_kernel, dim3(1u << 22), dim3(256), 0, 0, g_op, g_seed, d); }, r))
            return rc;
        merge(acc, r);
    }
    for (int i = 0; i < 4; i++) out[i] = acc[i];
    return 0;
}
// blocks x 256 threads x 64 pairs, in launches of at most 4096 blocks
int mp_probe_div(uint64_t seed, uint64_t blocks, unsigned long long* out) {
    g_seed = seed;
    unsigned long long acc[4] = {0ull, 0ull, ~0ull, 0ull};
    for (uint64_t b0 = 0; b0 < blocks; b0 += kDivBlocksPerLaunch) {
        unsigned long long r[4];
        g_base = b0 * 256u;
        g_blocks = blocks - b0 < kDivBlocksPerLaunch ? blocks - b0 : kDivBlocksPerLaunch;
        if (int rc = run([](unsigned long long* d) {
                hipLaunchKernelGGL(div_kernel<kDivPairs>, dim3(static_cast<uint32_t>(g_blocks)), dim3(256), 0, 0, g_seed, g_base, d);
            }, r))
            return rc;
        merge(acc, r);
    }
    for (int i = 0; i < 4; i++) out[i] = acc[i];
    return 0;
}
// blocks x 256 rays
int mp_probe_ray(uint64_t seed, int mode, uint64_t blocks, unsigned long long* out) {
    g_seed = seed; g_mode = mode; g_blocks = blocks;
    return run([](unsigned long long* d) { hipLaunchKernelGGL(ray_kernel, dim3(static_cast<uint32_t>(g_blocks)), dim3(256), 0, 0, g_seed, g_mode, d); }, out);
}
// blocks x 256 shading normals
int mp_probe_normal(uint64_t seed, int mode, uint64_t blocks, unsigned long long* out) {
    g_seed = seed; g_mode = mode; g_blocks = blocks;
    return run([](unsigned long long* d) { hipLaunchKernelGGL(normal_kernel, dim3(static_cast<uint32_t>(g_blocks)), dim3(256), 0, 0, g_seed, g_mode, d); }, out);
}
}
