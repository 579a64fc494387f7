// libminipath_sky.so: the sky lighting of include/minipath_sky.h -- the kernels and the C ABI over them.  The header's text is the
// contract; tests/sky_model.py restates it in numpy and the kernels must give its bits, so every operation below is written out
// one rounding at a time (built with -ffp-contract=off, correctly rounded divide and sqrt, subnormals kept: the flags of
// libminipath_hip.so).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/minipath_sky.h"
#include "../post/post_abi.h"

namespace mpe {

// A thread per pixel, the image in row-major order: the 64 pixels of a wave are 64 neighbouring rays of every sample slab, so each
// of the five loads of a sample is one whole run per wave (256 bytes of an f32 array, 64 of the bytes) and the two plane stores are
// 1 KiB runs.  The four texels of a lookup are one 16-byte load each; where they lie is the scene's business (cosine-distributed
// directions about neighbouring normals: scattered over the map), which is why the map has to stay in the caches.
constexpr int BLOCK = 256;

struct ResArgs {
    const float4* env;
    const float* dx;
    const float* dy;
    const float* dz;
    const float* tmax;
    const uint8_t* occluded;
    float4* sums;
    float4* out;
    uint32_t pixels, batch, map_size, pole, accumulate;
};

struct GradArgs {
    float4* env;
    uint32_t map_size;
    float zenith[3], horizon[3], ground[3];
};

// One axis of step 2: from u (or v) to the two texel indices and the weight of the second.  The clamps in this form send a NaN to 0.
__device__ __forceinline__ void taps(float u, float Nf, uint32_t N, uint32_t& i0, uint32_t& i1, float& w) {
    float f = u * Nf - 0.5f;
    f = f > 0.0f ? f : 0.0f;
    const float top = Nf - 1.0f;
    f = f < top ? f : top;
    const float fl = floorf(f);
    i0 = static_cast<uint32_t>(static_cast<int>(fl));  // 0 <= fl <= N - 1
    i1 = i0 + 1 < N ? i0 + 1 : N - 1;
    w = f - fl;
}

// the fold of the lower hemisphere, both from the old values
__device__ __forceinline__ void fold(float& px, float& py) {
    const float qx = copysignf(1.0f - fabsf(py), px), qy = copysignf(1.0f - fabsf(px), py);
    px = qx;
    py = qy;
}

// One sample of a pixel: what the five streams hold for it.
struct Sample {
    float t, x, y, z;
    uint8_t occ;
};
__device__ __forceinline__ Sample load_sample(const ResArgs& a, uint32_t r) {
    return Sample{a.tmax[r], a.dx[r], a.dy[r], a.dz[r], a.occluded[r]};
}

template <bool WRITE_OUT>
__global__ __launch_bounds__(BLOCK) void sky_resolve_kernel(const ResArgs a) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.pixels) return;
    float Er = 0.0f, Eg = 0.0f, Eb = 0.0f, C = 0.0f;
    if (a.accumulate) {
        const float4 old = a.sums[p];
        Er = old.x; Eg = old.y; Eb = old.z; C = old.w;
    }
    const uint32_t N = a.map_size;
    const float Nf = static_cast<float>(N);
    uint32_t r = p;  // b * pixels + p < 2^31
    // The loads of the next sample are issued before this sample's lookup, whose four texel loads wait for the direction: the
    // streams' round trip to HBM and the map's to the caches then overlap instead of following each other once per sample.
    Sample next = load_sample(a, r);
    for (uint32_t b = 0; b < a.batch; ++b) {
        const Sample s = next;
        r += a.pixels;
        if (b + 1 < a.batch) next = load_sample(a, r);
        // step 1
        if (s.t > 0.0f || s.t == -1.0f) C = C + 1.0f;
        if (!(s.t > 0.0f && s.occ == 0)) continue;
        // step 2
        const float mx = a.pole == 2 ? s.x : a.pole == 1 ? s.z : s.y;
        const float my = a.pole == 2 ? s.y : a.pole == 1 ? s.x : s.z;
        const float mz = a.pole == 2 ? s.z : a.pole == 1 ? s.y : s.x;
        const float l1 = (fabsf(mx) + fabsf(my)) + fabsf(mz);
        float Lr = 0.0f, Lg = 0.0f, Lb = 0.0f;
        if (l1 > 0.0f && l1 < INFINITY) {
            float px = mx / l1, py = my / l1;
            if (mz < 0.0f) fold(px, py);
            const float u = px * 0.5f + 0.5f, v = py * 0.5f + 0.5f;
            uint32_t x0, x1, y0, y1;
            float wx, wy;
            taps(u, Nf, N, x0, x1, wx);
            taps(v, Nf, N, y0, y1, wy);
            const float4 t00 = a.env[y0 * N + x0], t01 = a.env[y0 * N + x1];  // y * N + x < 2^26
            const float4 t10 = a.env[y1 * N + x0], t11 = a.env[y1 * N + x1];
            const float ax = 1.0f - wx, ay = 1.0f - wy;
            const float top_r = t00.x * ax + t01.x * wx, top_g = t00.y * ax + t01.y * wx, top_b = t00.z * ax + t01.z * wx;
            const float bot_r = t10.x * ax + t11.x * wx, bot_g = t10.y * ax + t11.y * wx, bot_b = t10.z * ax + t11.z * wx;
            Lr = top_r * ay + bot_r * wy;
            Lg = top_g * ay + bot_g * wy;
            Lb = top_b * ay + bot_b * wy;
        }
        // step 3
        Er = Er + Lr; Eg = Eg + Lg; Eb = Eb + Lb;
    }
    a.sums[p] = make_float4(Er, Eg, Eb, C);
    if (WRITE_OUT) a.out[p] = C > 0.0f ? make_float4(Er / C, Eg / C, Eb / C, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// A thread per texel, row-major: a wave writes 1 KiB runs.
__global__ __launch_bounds__(BLOCK) void sky_gradient_kernel(const GradArgs a) {
    const uint32_t N = a.map_size;
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;  // j * N + i < 2^26
    if (k >= N * N) return;
    const uint32_t j = k / N, i = k - j * N;
    const float Nf = static_cast<float>(N);
    float px = ((static_cast<float>(i) + 0.5f) / Nf) * 2.0f - 1.0f;
    float py = ((static_cast<float>(j) + 0.5f) / Nf) * 2.0f - 1.0f;
    const float z = (1.0f - fabsf(px)) - fabsf(py);
    if (z < 0.0f) fold(px, py);
    const float len = sqrtf((px * px + py * py) + z * z);
    const float h = z / len;
    float c[3];
    for (int q = 0; q < 3; ++q) c[q] = h >= 0.0f ? a.horizon[q] + (a.zenith[q] - a.horizon[q]) * h : a.ground[q];
    a.env[k] = make_float4(c[0], c[1], c[2], 1.0f);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
namespace {

constexpr size_t kSettingsPublished = offsetof(mpe_settings, pole) + sizeof(uint32_t);

// Everything mpe_resolve refuses by the settings alone; nullptr = accepted.
const char* settings_refusal(const mpe_settings* st) {
    if (!st) return "settings is NULL";
    if (st->struct_size < kSettingsPublished) return "bad struct_size";
    if (st->width == 0 || st->height == 0) return "width * height == 0";
    if (st->width > MPE_MAX_DIM || st->height > MPE_MAX_DIM) return "width or height above MPE_MAX_DIM";
    if (st->batch == 0) return "batch == 0";
    // width * height <= 2^40, then below 2^31 with batch < 2^32: both products are compared without overflow
    const uint64_t pixels = static_cast<uint64_t>(st->width) * st->height;
    if (pixels >= MPE_MAX_RAYS || pixels * st->batch >= MPE_MAX_RAYS) return "width * height * batch >= 2^31";
    if (st->sample_count == 0 || st->sample_count > MPE_MAX_SAMPLES) return "sample_count outside 1 .. MPE_MAX_SAMPLES";
    if (static_cast<uint64_t>(st->sample_begin) + st->batch > st->sample_count) return "sample_begin + batch > sample_count";
    if (st->map_size == 0 || st->map_size > MPE_MAX_MAP) return "map_size outside 1 .. MPE_MAX_MAP";
    if (st->pole > 2) return "pole above 2";
    if (st->flags & ~MPE_FLAG_ACCUMULATE) return "unknown flag";
    return nullptr;
}

}  // namespace
}  // namespace mpe

using namespace mpe;

extern "C" {

const char* mpe_last_error(void) { return g_last_error.c_str(); }
uint32_t mpe_settings_size(void) { return static_cast<uint32_t>(sizeof(mpe_settings)); }

int mpe_check_settings(const mpe_settings* st) {
    return guarded([&]() -> int {
        if (const char* why = settings_refusal(st)) return fail(MP_ERR_INVALID, why);
        return MP_OK;
    });
}

int mpe_last_kernels(char* buf, size_t cap, size_t* needed) {
    return guarded([&]() -> int { return copy_last_kernels(buf, cap, needed); });
}

int mpe_resolve(int device_id, const mpe_settings* st, const float* d_env, const float* d_dx, const float* d_dy, const float* d_dz,
                const float* d_tmax, const uint8_t* d_occluded, float* d_sums, float* d_out, void* stream) {
    return guarded([&]() -> int {
        if (const char* why = settings_refusal(st)) return fail(MP_ERR_INVALID, why);
        if (device_id < 0) return fail(MP_ERR_INVALID, "negative device_id");
        if (!d_env || !d_dx || !d_dy || !d_dz || !d_tmax || !d_occluded || !d_sums) return fail(MP_ERR_INVALID, "NULL argument");
        const uint32_t pixels = st->width * st->height;  // < 2^31
        const size_t rays = static_cast<size_t>(pixels) * st->batch, plane = static_cast<size_t>(pixels) * 16;
        const size_t map = static_cast<size_t>(st->map_size) * st->map_size * 16;
        const Span spans[] = {{d_sums, plane}, {d_out, plane}, {d_env, map}, {d_dx, rays * 4}, {d_dy, rays * 4}, {d_dz, rays * 4},
                              {d_tmax, rays * 4}, {d_occluded, rays}};
        if (outputs_overlap(spans, 8, 2)) return fail(MP_ERR_INVALID, "an output overlaps another buffer of the call");
        if (!all_aligned({d_env, d_sums, d_out}, kPlaneAlign)) return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");
        if (!all_aligned({d_dx, d_dy, d_dz, d_tmax}, kWordAlign)) return fail(MP_ERR_INVALID, "a ray array is not 4-byte aligned");
        ResArgs a{};
        a.env = reinterpret_cast<const float4*>(d_env);
        a.dx = d_dx; a.dy = d_dy; a.dz = d_dz;
        a.tmax = d_tmax;
        a.occluded = d_occluded;
        a.sums = reinterpret_cast<float4*>(d_sums);
        a.out = reinterpret_cast<float4*>(d_out);
        a.pixels = pixels;
        a.batch = st->batch;
        a.map_size = st->map_size;
        a.pole = st->pole;
        a.accumulate = (st->flags & MPE_FLAG_ACCUMULATE) ? 1u : 0u;

        DeviceScope dev;
        if (hipError_t e = dev.enter(device_id); e != hipSuccess) return hip_fail(e, "hipSetDevice");
        const dim3 grid((pixels + BLOCK - 1) / BLOCK), block(BLOCK);
        LaunchLog log;
        return d_out ? launch(log, "sky_resolve_kernel<true>", sky_resolve_kernel<true>, grid, block, stream, a)
                     : launch(log, "sky_resolve_kernel<false>", sky_resolve_kernel<false>, grid, block, stream, a);
    });
}

int mpe_fill_gradient(int device_id, uint32_t map_size, const float* zenith, const float* horizon, const float* ground, float* d_env,
                      void* stream) {
    return guarded([&]() -> int {
        if (map_size == 0 || map_size > MPE_MAX_MAP) return fail(MP_ERR_INVALID, "map_size outside 1 .. MPE_MAX_MAP");
        if (device_id < 0) return fail(MP_ERR_INVALID, "negative device_id");
        if (!zenith || !horizon || !ground || !d_env) return fail(MP_ERR_INVALID, "NULL argument");
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(zenith[c]) || !std::isfinite(horizon[c]) || !std::isfinite(ground[c]))
                return fail(MP_ERR_INVALID, "a gradient colour is not finite");
        if (!all_aligned({d_env}, kPlaneAlign)) return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");
        GradArgs a{};
        a.env = reinterpret_cast<float4*>(d_env);
        a.map_size = map_size;
        for (int c = 0; c < 3; ++c) {
            a.zenith[c] = zenith[c];
            a.horizon[c] = horizon[c];
            a.ground[c] = ground[c];
        }

        DeviceScope dev;
        if (hipError_t e = dev.enter(device_id); e != hipSuccess) return hip_fail(e, "hipSetDevice");
        const dim3 grid((map_size * map_size + BLOCK - 1) / BLOCK), block(BLOCK);
        LaunchLog log;
        return launch(log, "sky_gradient_kernel", sky_gradient_kernel, grid, block, stream, a);
    });
}

}  // extern "C"
