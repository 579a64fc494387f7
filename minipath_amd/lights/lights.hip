// libminipath_lights.so: the point and sphere lights of include/minipath_lights.h -- the kernels and the C ABI over them.  The
// header's text is the contract; tests/lights_model.py restates it in numpy and the kernels must give its bits, so every operation
// below is written out one rounding at a time (built with -ffp-contract=off, correctly rounded divide and sqrt, subnormals kept:
// the flags of libminipath_hip.so).  The RNG is the renderer's own (csrc/ray_math.h), not a copy.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/minipath_lights.h"
#include "../post/post_abi.h"
#include "../csrc/ray_math.h"

namespace mpl {

namespace rm = mp::rm;

// A thread per pixel, the image in row-major order: the 64 pixels of a wave are 64 neighbouring rays of every (sample, light)
// slab, so each of the eight stores of a ray is one whole 256-byte run per wave and the two plane loads are 1 KiB runs.
constexpr int BLOCK = 256;

// The light table by value: kernel arguments, the same for every thread, indexed by the (uniform) light loop alone.
struct LightTable {
    mpl_light light[MPL_MAX_LIGHTS];
};

struct GenArgs {
    const float4* position;
    const float4* normal;
    float *ox, *oy, *oz, *dx, *dy, *dz, *tmax, *weight;
    uint64_t key0;  // mix(seed) + sample_begin
    uint32_t pixels, batch, sample_count, light_count;
    float eye[3];
    float bias, margin;
    LightTable table;
};

struct ResArgs {
    const float* tmax;
    const float* weight;
    const uint8_t* occluded;
    float4* sums;
    float4* out;
    uint32_t pixels, batch, light_count, accumulate;
    LightTable table;
};

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// basis(m) of include/minipath_secondary.h
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

template <bool SPHERES>
__global__ __launch_bounds__(BLOCK) void light_rays_kernel(const GenArgs a) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.pixels) return;
    const float4 pos = a.position[p];
    const float4 nrm = a.normal[p];
    // steps 1 and 2: what the pixel alone decides
    const float A = pos.w;
    const float l2 = dot3(nrm.x, nrm.y, nrm.z, nrm.x, nrm.y, nrm.z);
    const bool live = A > 0.0f && l2 > 0.0f;
    float nx = 0.f, ny = 0.f, nz = 0.f, Ox = 0.f, Oy = 0.f, Oz = 0.f;
    if (live) {
        const float Px = pos.x / A, Py = pos.y / A, Pz = pos.z / A;
        const float len = sqrtf(l2);
        nx = nrm.x / len; ny = nrm.y / len; nz = nrm.z / len;
        const float wx = Px - a.eye[0], wy = Py - a.eye[1], wz = Pz - a.eye[2];
        if (dot3(wx, wy, wz, nx, ny, nz) > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
        Ox = Px + nx * a.bias; Oy = Py + ny * a.bias; Oz = Pz + nz * a.bias;
    }
    const uint64_t key_p = a.key0 + static_cast<uint64_t>(p) * a.sample_count;
    uint32_t r = p;  // (b * L + l) * pixels + p < 2^31; after the last ray r < 2^31 + pixels < 2^32
    for (uint32_t b = 0; b < a.batch; ++b) {
        rm::Rng rng;
        if (SPHERES && live) rm::rng_seed(rng, key_p + b);
        for (uint32_t l = 0; l < a.light_count; ++l, r += a.pixels) {
            const mpl_light& lt = a.table.light[l];
            const float R = lt.radius;
            float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, tm = 0.0f, wt = 0.0f;  // NONE
            if (live) {
                const float cx = lt.position[0], cy = lt.position[1], cz = lt.position[2];
                float gx = cx, gy = cy, gz = cz;
                bool lit = true;
                if (SPHERES && R > 0.0f) {
                    float u, v;
                    rm::unit_disc<true>(rng, u, v);  // drawn whatever becomes of the ray
                    const float wx = cx - Ox, wy = cy - Oy, wz = cz - Oz;
                    const float q2 = dot3(wx, wy, wz, wx, wy, wz);
                    if (q2 > R * R) {
                        const float q = sqrtf(q2);
                        float t[3], bt[3];
                        basis(wx / q, wy / q, wz / q, t, bt);
                        const float ur = u * R, vr = v * R;
                        gx = cx + (t[0] * ur + bt[0] * vr);
                        gy = cy + (t[1] * ur + bt[1] * vr);
                        gz = cz + (t[2] * ur + bt[2] * vr);
                    } else {
                        lit = false;  // the point is inside the light
                    }
                }
                const float ex = gx - Ox, ey = gy - Oy, ez = gz - Oz;
                const float dd = dot3(ex, ey, ez, ex, ey, ez);
                const float len = sqrtf(dd);
                const float nd = dot3(nx, ny, nz, ex, ey, ez);
                const float reach = len - a.margin;
                if (lit && nd > 0.0f && dd > 0.0f && reach > 0.0f) {
                    ox = Ox; oy = Oy; oz = Oz;
                    dx = ex; dy = ey; dz = ez;
                    tm = reach;
                    wt = nd / (dd * len);
                } else {
                    tm = -1.0f;  // UNLIT
                }
            }
            a.ox[r] = ox; a.oy[r] = oy; a.oz[r] = oz;
            a.dx[r] = dx; a.dy[r] = dy; a.dz[r] = dz;
            a.tmax[r] = tm;
            a.weight[r] = wt;
        }
    }
}

template <bool WRITE_OUT>
__global__ __launch_bounds__(BLOCK) void irradiance_kernel(const ResArgs a) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.pixels) return;
    float Er = 0.0f, Eg = 0.0f, Eb = 0.0f, C = 0.0f;
    if (a.accumulate) {
        const float4 old = a.sums[p];
        Er = old.x; Eg = old.y; Eb = old.z; C = old.w;
    }
    uint32_t r = p;  // as in light_rays_kernel
    for (uint32_t b = 0; b < a.batch; ++b) {
        for (uint32_t l = 0; l < a.light_count; ++l, r += a.pixels) {
            const float tm = a.tmax[r];
            const float wt = a.weight[r];
            const uint8_t occ = a.occluded[r];
            const mpl_light& lt = a.table.light[l];
            if (l == 0 && (tm > 0.0f || tm == -1.0f)) C = C + 1.0f;
            // Selects, not a branch around the sum: under a branch the weight is loaded only once tmax and occluded have arrived,
            // two dependent round trips per ray; this way a ray's three loads wait for nothing.  The sum of a ray that is not
            // seen is computed and dropped (no operation here can trap), so a seen ray's operations are those of the header.
            const bool seen = tm > 0.0f && occ == 0;
            const float er = Er + lt.intensity[0] * wt, eg = Eg + lt.intensity[1] * wt, eb = Eb + lt.intensity[2] * wt;
            Er = seen ? er : Er;
            Eg = seen ? eg : Eg;
            Eb = seen ? eb : Eb;
        }
    }
    a.sums[p] = make_float4(Er, Eg, Eb, C);
    if (WRITE_OUT) a.out[p] = C > 0.0f ? make_float4(Er / C, Eg / C, Eb / C, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
namespace {

constexpr size_t kSettingsPublished = offsetof(mpl_settings, margin) + sizeof(float);
static_assert(sizeof(mpl_light) == 32, "mpl_light is 32 bytes");

// Everything both calls refuse by the settings and the light table alone; nullptr = accepted.  Every compare is false for a NaN.
const char* settings_refusal(const mpl_settings* st, const mpl_light* lights) {
    if (!st) return "settings is NULL";
    if (st->struct_size < kSettingsPublished) return "bad struct_size";
    if (st->width == 0 || st->height == 0) return "width * height == 0";
    if (st->width > MPL_MAX_DIM || st->height > MPL_MAX_DIM) return "width or height above MPL_MAX_DIM";
    if (st->batch == 0) return "batch == 0";
    if (st->light_count == 0 || st->light_count > MPL_MAX_LIGHTS) return "light_count outside 1 .. MPL_MAX_LIGHTS";
    // width * height <= 2^40, then below 2^31 with batch < 2^32 and light_count <= 8: every product is compared without overflow
    const uint64_t pixels = static_cast<uint64_t>(st->width) * st->height;
    if (pixels >= MPL_MAX_RAYS || pixels * st->batch >= MPL_MAX_RAYS || pixels * st->batch * st->light_count >= MPL_MAX_RAYS)
        return "width * height * batch * light_count >= 2^31";
    if (st->sample_count == 0 || st->sample_count > MPL_MAX_SAMPLES) return "sample_count outside 1 .. MPL_MAX_SAMPLES";
    if (static_cast<uint64_t>(st->sample_begin) + st->batch > st->sample_count) return "sample_begin + batch > sample_count";
    if (st->flags & ~MPL_FLAG_ACCUMULATE) return "unknown flag";
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(st->eye[c])) return "eye is not finite";
    if (!(st->bias >= 0.f) || !std::isfinite(st->bias)) return "bias is not finite and >= 0";
    if (!(st->margin >= 0.f) || !std::isfinite(st->margin)) return "margin is not finite and >= 0";
    if (!lights) return "lights is NULL";
    for (uint32_t l = 0; l < st->light_count; ++l) {
        const mpl_light& lt = lights[l];
        for (int c = 0; c < 3; ++c) {
            if (!std::isfinite(lt.position[c])) return "a light's position is not finite";
            if (!(lt.intensity[c] >= 0.f) || !std::isfinite(lt.intensity[c])) return "a light's intensity is not finite and >= 0";
        }
        if (!(lt.radius >= 0.f) || !std::isfinite(lt.radius)) return "a light's radius is not finite and >= 0";
        if (!(lt.reserved == 0.f)) return "a light's reserved is not 0";
    }
    return nullptr;
}

void copy_table(LightTable& t, const mpl_settings* st, const mpl_light* lights) {
    t = LightTable{};
    for (uint32_t l = 0; l < st->light_count; ++l) t.light[l] = lights[l];
}

}  // namespace
}  // namespace mpl

using namespace mpl;

extern "C" {

const char* mpl_last_error(void) { return g_last_error.c_str(); }
uint32_t mpl_settings_size(void) { return static_cast<uint32_t>(sizeof(mpl_settings)); }

int mpl_check_settings(const mpl_settings* st, const mpl_light* lights) {
    return guarded([&]() -> int {
        if (const char* why = settings_refusal(st, lights)) return fail(MP_ERR_INVALID, why);
        return MP_OK;
    });
}

int mpl_last_kernels(char* buf, size_t cap, size_t* needed) {
    return guarded([&]() -> int { return copy_last_kernels(buf, cap, needed); });
}

int mpl_generate(int device_id, const mpl_settings* st, const mpl_light* lights, const float* d_position, const float* d_normal,
                 float* d_ox, float* d_oy, float* d_oz, float* d_dx, float* d_dy, float* d_dz, float* d_tmax, float* d_weight,
                 void* stream) {
    return guarded([&]() -> int {
        if (const char* why = settings_refusal(st, lights)) return fail(MP_ERR_INVALID, why);
        if (device_id < 0) return fail(MP_ERR_INVALID, "negative device_id");
        if (!d_position || !d_normal || !d_ox || !d_oy || !d_oz || !d_dx || !d_dy || !d_dz || !d_tmax || !d_weight)
            return fail(MP_ERR_INVALID, "NULL argument");
        const uint32_t pixels = st->width * st->height;  // < 2^31
        const size_t rays = static_cast<size_t>(pixels) * st->batch * st->light_count * 4, plane = static_cast<size_t>(pixels) * 16;
        const Span spans[] = {{d_ox, rays}, {d_oy, rays}, {d_oz, rays}, {d_dx, rays}, {d_dy, rays}, {d_dz, rays}, {d_tmax, rays},
                              {d_weight, rays}, {d_position, plane}, {d_normal, plane}};
        if (outputs_overlap(spans, 10, 8)) return fail(MP_ERR_INVALID, "a ray array overlaps another buffer of the call");
        if (!all_aligned({d_position, d_normal}, kPlaneAlign)) return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");
        if (!all_aligned({d_ox, d_oy, d_oz, d_dx, d_dy, d_dz, d_tmax, d_weight}, kWordAlign))
            return fail(MP_ERR_INVALID, "a ray array is not 4-byte aligned");
        GenArgs a{};
        a.position = reinterpret_cast<const float4*>(d_position);
        a.normal = reinterpret_cast<const float4*>(d_normal);
        a.ox = d_ox; a.oy = d_oy; a.oz = d_oz;
        a.dx = d_dx; a.dy = d_dy; a.dz = d_dz;
        a.tmax = d_tmax;
        a.weight = d_weight;
        rm::U64 state = rm::u64_split(st->seed);
        a.key0 = rm::u64_join(rm::splitmix(state)) + st->sample_begin;  // mix(seed): the first SplitMix64 output for the state `seed`
        a.pixels = pixels;
        a.batch = st->batch;
        a.sample_count = st->sample_count;
        a.light_count = st->light_count;
        for (int c = 0; c < 3; ++c) a.eye[c] = st->eye[c];
        a.bias = st->bias;
        a.margin = st->margin;
        copy_table(a.table, st, lights);
        bool spheres = false;
        for (uint32_t l = 0; l < st->light_count; ++l) spheres = spheres || lights[l].radius > 0.f;

        DeviceScope dev;
        if (hipError_t e = dev.enter(device_id); e != hipSuccess) return hip_fail(e, "hipSetDevice");
        const dim3 grid((pixels + BLOCK - 1) / BLOCK), block(BLOCK);
        LaunchLog log;
        return spheres ? launch(log, "light_rays_kernel<true>", light_rays_kernel<true>, grid, block, stream, a)
                       : launch(log, "light_rays_kernel<false>", light_rays_kernel<false>, grid, block, stream, a);
    });
}

int mpl_resolve(int device_id, const mpl_settings* st, const mpl_light* lights, const float* d_tmax, const float* d_weight,
                const uint8_t* d_occluded, float* d_sums, float* d_out, void* stream) {
    return guarded([&]() -> int {
        if (const char* why = settings_refusal(st, lights)) return fail(MP_ERR_INVALID, why);
        if (device_id < 0) return fail(MP_ERR_INVALID, "negative device_id");
        if (!d_tmax || !d_weight || !d_occluded || !d_sums) return fail(MP_ERR_INVALID, "NULL argument");
        const uint32_t pixels = st->width * st->height;
        const size_t rays = static_cast<size_t>(pixels) * st->batch * st->light_count, plane = static_cast<size_t>(pixels) * 16;
        const Span spans[] = {{d_sums, plane}, {d_out, plane}, {d_tmax, rays * 4}, {d_weight, rays * 4}, {d_occluded, rays}};
        if (outputs_overlap(spans, 5, 2)) return fail(MP_ERR_INVALID, "an output overlaps another buffer of the call");
        if (!all_aligned({d_sums, d_out}, kPlaneAlign)) return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");
        if (!all_aligned({d_tmax, d_weight}, kWordAlign)) return fail(MP_ERR_INVALID, "a ray array is not 4-byte aligned");
        ResArgs a{};
        a.tmax = d_tmax;
        a.weight = d_weight;
        a.occluded = d_occluded;
        a.sums = reinterpret_cast<float4*>(d_sums);
        a.out = reinterpret_cast<float4*>(d_out);
        a.pixels = pixels;
        a.batch = st->batch;
        a.light_count = st->light_count;
        a.accumulate = (st->flags & MPL_FLAG_ACCUMULATE) ? 1u : 0u;
        copy_table(a.table, st, lights);

        DeviceScope dev;
        if (hipError_t e = dev.enter(device_id); e != hipSuccess) return hip_fail(e, "hipSetDevice");
        const dim3 grid((pixels + BLOCK - 1) / BLOCK), block(BLOCK);
        LaunchLog log;
        return d_out ? launch(log, "irradiance_kernel<true>", irradiance_kernel<true>, grid, block, stream, a)
                     : launch(log, "irradiance_kernel<false>", irradiance_kernel<false>, grid, block, stream, a);
    });
}

}  // extern "C"
