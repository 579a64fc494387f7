// libminipath_secondary.so: the deferred secondary visibility of include/minipath_secondary.h -- the kernels and the C ABI over
// them.  The header's text is the contract; tests/secondary_model.py restates it in numpy and the kernels must give its bits, so
// every operation below is written out one rounding at a time (built with -ffp-contract=off, correctly rounded divide and sqrt,
// subnormals kept: the flags of libminipath_hip.so).  The RNG is the renderer's own (csrc/ray_math.h), not a copy.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/minipath_secondary.h"
#include "../post/post_abi.h"
#include "../csrc/ray_math.h"

namespace mps {

namespace rm = mp::rm;

// A thread per pixel, the image in row-major order: the 64 pixels of a wave are 64 neighbouring rays of every sample of the batch,
// so each of the seven stores of a sample is one whole 256-byte run per wave and the two plane loads are 1 KiB runs.
constexpr int BLOCK = 256;

struct GenArgs {
    const float4* position;
    const float4* normal;
    float *ox, *oy, *oz, *dx, *dy, *dz, *tmax;
    uint64_t key0;  // mix(seed) + sample_begin
    uint32_t pixels, batch, sample_count;
    float eye[3], light[3];
    float radius, bias, spread;
};

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// the header's basis(m)
__device__ __forceinline__ void basis(float mx, float my, float mz, float (&t)[3], float (&bt)[3]) {
    const float sg = copysignf(1.0f, mz);
    const float a = -1.0f / (sg + mz);
    const float bb = (mx * my) * a;
    t[0] = 1.0f + ((sg * mx) * mx) * a;
    t[1] = sg * bb;
    t[2] = -sg * mx;
    bt[0] = bb;
    bt[1] = sg + (my * my) * a;
    bt[2] = -my;
}

template <int MODE>
__global__ __launch_bounds__(BLOCK) void secondary_rays_kernel(const GenArgs a) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.pixels) return;
    const float4 pos = a.position[p];
    const float4 nrm = a.normal[p];
    // steps 1, 2 and (SUN) the light test: what the pixel alone decides
    const float A = pos.w;
    const float l2 = dot3(nrm.x, nrm.y, nrm.z, nrm.x, nrm.y, nrm.z);
    float code = 0.0f;  // tmax of a ray that is not traced: 0 = NONE, -1 = UNLIT
    bool live = A > 0.0f && l2 > 0.0f;
    float Px = 0.f, Py = 0.f, Pz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    float t[3] = {0.f, 0.f, 0.f}, bt[3] = {0.f, 0.f, 0.f};
    if (live) {
        Px = pos.x / A; Py = pos.y / A; Pz = pos.z / A;
        const float len = sqrtf(l2);
        nx = nrm.x / len; ny = nrm.y / len; nz = nrm.z / len;
        const float wx = Px - a.eye[0], wy = Py - a.eye[1], wz = Pz - a.eye[2];
        if (dot3(wx, wy, wz, nx, ny, nz) > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
        if (MODE == MPS_MODE_SUN) {
            if (dot3(nx, ny, nz, a.light[0], a.light[1], a.light[2]) > 0.0f) {
                basis(a.light[0], a.light[1], a.light[2], t, bt);
            } else {
                live = false;
                code = -1.0f;
            }
        } else {
            basis(nx, ny, nz, t, bt);
        }
    }
    const float Ox = Px + nx * a.bias, Oy = Py + ny * a.bias, Oz = Pz + nz * a.bias;
    const uint64_t key_p = a.key0 + static_cast<uint64_t>(p) * a.sample_count;
    size_t r = p;  // b * pixels + p < 2^31
    for (uint32_t b = 0; b < a.batch; ++b, r += a.pixels) {
        float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, tm = code;
        if (live) {
            rm::Rng rng;
            rm::rng_seed(rng, key_p + b);
            float u, v;
            rm::unit_disc<true>(rng, u, v);
            if (MODE == MPS_MODE_SUN) {
                const float us = u * a.spread, vs = v * a.spread;
                dx = (t[0] * us + bt[0] * vs) + a.light[0];
                dy = (t[1] * us + bt[1] * vs) + a.light[1];
                dz = (t[2] * us + bt[2] * vs) + a.light[2];
            } else {
                const float z = sqrtf(1.0f - (u * u + v * v));
                dx = (t[0] * u + bt[0] * v) + nx * z;
                dy = (t[1] * u + bt[1] * v) + ny * z;
                dz = (t[2] * u + bt[2] * v) + nz * z;
            }
            ox = Ox; oy = Oy; oz = Oz;
            tm = a.radius;
        }
        a.ox[r] = ox; a.oy[r] = oy; a.oz[r] = oz;
        a.dx[r] = dx; a.dy[r] = dy; a.dz[r] = dz;
        a.tmax[r] = tm;
    }
}

template <bool WRITE_OUT>
__global__ __launch_bounds__(BLOCK) void resolve_kernel(const float* __restrict__ tmax, const uint8_t* __restrict__ occluded,
                                                         float4* counts, float4* out, uint32_t pixels, uint32_t batch,
                                                         uint32_t accumulate) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= pixels) return;
    float V = 0.0f, C = 0.0f;
    size_t r = p;
    for (uint32_t b = 0; b < batch; ++b, r += pixels) {
        const float tm = tmax[r];
        const uint8_t occ = occluded[r];
        if (tm > 0.0f) {
            C = C + 1.0f;
            if (occ == 0) V = V + 1.0f;
        } else if (tm == -1.0f) {
            C = C + 1.0f;
        }
    }
    if (accumulate) {
        const float4 old = counts[p];
        V = old.x + V;
        C = old.y + C;
    }
    counts[p] = make_float4(V, C, 0.0f, 0.0f);
    if (WRITE_OUT) {
        const float v = C > 0.0f ? V / C : 1.0f;
        out[p] = make_float4(v, v, v, C > 0.0f ? 1.0f : 0.0f);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
namespace {

constexpr size_t kSettingsPublished = offsetof(mps_settings, spread) + sizeof(float);

// Everything both calls refuse by the settings alone; nullptr = accepted.  Every compare is false for a NaN.
const char* settings_refusal(const mps_settings* st) {
    if (!st) return "settings is NULL";
    if (st->struct_size < kSettingsPublished) return "bad struct_size";
    if (st->width == 0 || st->height == 0) return "width * height == 0";
    if (st->width > MPS_MAX_DIM || st->height > MPS_MAX_DIM) return "width or height above MPS_MAX_DIM";
    if (st->batch == 0) return "batch == 0";
    // width * height <= 2^40 and batch < 2^32: the product is compared without overflow in two steps
    const uint64_t pixels = static_cast<uint64_t>(st->width) * st->height;
    if (pixels >= MPS_MAX_RAYS || pixels * st->batch >= MPS_MAX_RAYS) return "width * height * batch >= 2^31";
    if (st->sample_count == 0 || st->sample_count > MPS_MAX_SAMPLES) return "sample_count outside 1 .. MPS_MAX_SAMPLES";
    if (static_cast<uint64_t>(st->sample_begin) + st->batch > st->sample_count) return "sample_begin + batch > sample_count";
    if (st->mode != MPS_MODE_AO && st->mode != MPS_MODE_SUN) return "unknown mode";
    if (st->flags & ~MPS_FLAG_ACCUMULATE) return "unknown flag";
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(st->eye[c])) return "eye is not finite";
        if (!std::isfinite(st->light[c])) return "light is not finite";
    }
    if (!(st->radius > 0.f)) return "radius is not > 0";
    if (!(st->bias >= 0.f) || !std::isfinite(st->bias)) return "bias is not finite and >= 0";
    if (!(st->spread >= 0.f) || !std::isfinite(st->spread)) return "spread is not finite and >= 0";
    return nullptr;
}

}  // namespace
}  // namespace mps

using namespace mps;

extern "C" {

const char* mps_last_error(void) { return g_last_error.c_str(); }
uint32_t mps_settings_size(void) { return static_cast<uint32_t>(sizeof(mps_settings)); }

int mps_check_settings(const mps_settings* st) {
    return guarded([&]() -> int {
        if (const char* why = settings_refusal(st)) return fail(MP_ERR_INVALID, why);
        return MP_OK;
    });
}

int mps_last_kernels(char* buf, size_t cap, size_t* needed) {
    return guarded([&]() -> int { return copy_last_kernels(buf, cap, needed); });
}

int mps_generate(int device_id, const mps_settings* st, const float* d_position, const float* d_normal, float* d_ox, float* d_oy,
                 float* d_oz, float* d_dx, float* d_dy, float* d_dz, float* d_tmax, void* stream) {
    return guarded([&]() -> int {
        if (const char* why = settings_refusal(st)) return fail(MP_ERR_INVALID, why);
        if (device_id < 0) return fail(MP_ERR_INVALID, "negative device_id");
        if (!d_position || !d_normal || !d_ox || !d_oy || !d_oz || !d_dx || !d_dy || !d_dz || !d_tmax)
            return fail(MP_ERR_INVALID, "NULL argument");
        const uint32_t pixels = st->width * st->height;  // < 2^31
        const size_t rays = static_cast<size_t>(pixels) * st->batch * 4, plane = static_cast<size_t>(pixels) * 16;
        const Span spans[] = {{d_ox, rays}, {d_oy, rays}, {d_oz, rays}, {d_dx, rays}, {d_dy, rays}, {d_dz, rays}, {d_tmax, rays},
                              {d_position, plane}, {d_normal, plane}};
        if (outputs_overlap(spans, 9, 7)) return fail(MP_ERR_INVALID, "a ray array overlaps another buffer of the call");
        if (!all_aligned({d_position, d_normal}, kPlaneAlign)) return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");
        if (!all_aligned({d_ox, d_oy, d_oz, d_dx, d_dy, d_dz, d_tmax}, kWordAlign))
            return fail(MP_ERR_INVALID, "a ray array is not 4-byte aligned");
        GenArgs a{};
        a.position = reinterpret_cast<const float4*>(d_position);
        a.normal = reinterpret_cast<const float4*>(d_normal);
        a.ox = d_ox; a.oy = d_oy; a.oz = d_oz;
        a.dx = d_dx; a.dy = d_dy; a.dz = d_dz;
        a.tmax = d_tmax;
        rm::U64 state = rm::u64_split(st->seed);
        a.key0 = rm::u64_join(rm::splitmix(state)) + st->sample_begin;  // mix(seed): the first SplitMix64 output for the state `seed`
        a.pixels = pixels;
        a.batch = st->batch;
        a.sample_count = st->sample_count;
        for (int c = 0; c < 3; ++c) {
            a.eye[c] = st->eye[c];
            a.light[c] = st->light[c];
        }
        a.radius = st->radius;
        a.bias = st->bias;
        a.spread = st->spread;

        DeviceScope dev;
        if (hipError_t e = dev.enter(device_id); e != hipSuccess) return hip_fail(e, "hipSetDevice");
        const dim3 grid((pixels + BLOCK - 1) / BLOCK), block(BLOCK);
        LaunchLog log;
        return st->mode == MPS_MODE_SUN ? launch(log, "secondary_rays_kernel<1>", secondary_rays_kernel<1>, grid, block, stream, a)
                                        : launch(log, "secondary_rays_kernel<0>", secondary_rays_kernel<0>, grid, block, stream, a);
    });
}

int mps_resolve(int device_id, const mps_settings* st, const float* d_tmax, const uint8_t* d_occluded, float* d_counts, float* d_out,
                void* stream) {
    return guarded([&]() -> int {
        if (const char* why = settings_refusal(st)) return fail(MP_ERR_INVALID, why);
        if (device_id < 0) return fail(MP_ERR_INVALID, "negative device_id");
        if (!d_tmax || !d_occluded || !d_counts) return fail(MP_ERR_INVALID, "NULL argument");
        const uint32_t pixels = st->width * st->height;
        const size_t rays = static_cast<size_t>(pixels) * st->batch, plane = static_cast<size_t>(pixels) * 16;
        const Span spans[] = {{d_counts, plane}, {d_out, plane}, {d_tmax, rays * 4}, {d_occluded, rays}};
        if (outputs_overlap(spans, 4, 2)) return fail(MP_ERR_INVALID, "an output overlaps another buffer of the call");
        if (!all_aligned({d_counts, d_out}, kPlaneAlign)) return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");
        if (!all_aligned({d_tmax}, kWordAlign)) return fail(MP_ERR_INVALID, "a ray array is not 4-byte aligned");

        DeviceScope dev;
        if (hipError_t e = dev.enter(device_id); e != hipSuccess) return hip_fail(e, "hipSetDevice");
        const dim3 grid((pixels + BLOCK - 1) / BLOCK), block(BLOCK);
        const uint32_t accumulate = (st->flags & MPS_FLAG_ACCUMULATE) ? 1u : 0u;
        float4* counts = reinterpret_cast<float4*>(d_counts);
        float4* out = reinterpret_cast<float4*>(d_out);
        LaunchLog log;
        return d_out ? launch(log, "resolve_kernel<true>", resolve_kernel<true>, grid, block, stream, d_tmax, d_occluded, counts, out,
                              pixels, st->batch, accumulate)
                     : launch(log, "resolve_kernel<false>", resolve_kernel<false>, grid, block, stream, d_tmax, d_occluded, counts, out,
                              pixels, st->batch, accumulate);
    });
}

}  // extern "C"
