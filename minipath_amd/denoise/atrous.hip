// libminipath_denoise.so: the edge-avoiding a-trous filter of include/minipath_denoise.h -- the kernels and the C ABI over them.
// The header's text is the contract; tests/denoise_model.py restates it in numpy and the kernels must give its bits, so every
// operation below is written out one rounding at a time (built with -ffp-contract=off, correctly rounded divide and sqrt,
// subnormals kept: the flags of libminipath_hip.so).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/minipath_denoise.h"
#include "../post/post_abi.h"

namespace mpd {

// ---- the lattice tiling --------------------------------------------------------------------------------------------------
// At step s the 25 taps of a pixel are s apart, so a block of neighbouring pixels shares none of them.  A block therefore takes
// a TILE x TILE tile of ONE residue class (cx, cy) of the lattice: the pixels (cx + s*(TILE*tx + i), cy + s*(TILE*ty + j)).  On
// that lattice the stencil is a dense 5 x 5 over (TILE + 4)^2 entries, staged once in LDS: each plane element is loaded
// (20/16)^2 = 1.56 times per pass.  Lanes walk x along a lattice row: 16-byte accesses s * 16 bytes apart.
constexpr int TILE = 16;
constexpr int HALO = 2;
constexpr int LT = TILE + 2 * HALO;  // 20
// Row strides against bank conflicts.  A ds_read_b128 is served in groups of 16 lanes that hold 8 + 4 + 4 consecutive entries of
// two neighbouring tile rows ({0-3, 12-15} of one, {4-11} of the next): with a row stride of 0 mod 16 entries (0 mod 64 banks) the
// three pieces tile the 64 banks exactly.  20 rows x 32 entries x 16 B = 10 KB per float4 plane.  The variance plane is read by
// ds_read_b32, whose 32-lane halves hold two tile rows of 16 floats: a stride of 16 mod 32 floats puts them on disjoint banks.
constexpr int LDC = 32;
constexpr int LDV = 48;

struct PassArgs {
    const float4* c_in;    // C_i (pass 0: the colour plane)
    const float4* nd;      // {n.x, n.y, n.z, t}
    const float4* albedo;  // read only when demod_in / demod_out
    const float4* v_in;    // V_i, .x read (VARIANCE)
    float4* c_out;         // C_{i+1} (last pass: d_out)
    float4* v_out;         // V_{i+1}, nullable (VARIANCE)
    uint32_t width, height;
    uint32_t step;                 // s = 2^i
    uint32_t classes_x, classes_y; // min(s, width), min(s, height): the residue classes that hold a pixel
    uint32_t tiles_x, tiles_y;     // tiles of the longest class per direction
    uint32_t k;                    // sigma_normal_pow2
    float sd;                      // sigma_depth * (float)s
    float sigma_l;
    uint32_t demod_in, demod_out;
};

// the header's max(a, b): b for a NaN a, +0 for max(-0, 0)
__device__ __forceinline__ float mx(float a, float b) { return a > b ? a : b; }

template <bool VARIANCE>
__global__ __launch_bounds__(TILE * TILE) void atrous_kernel(const PassArgs a) {
    __shared__ float4 s_c[LT * LDC];
    __shared__ float4 s_n[LT * LDC];
    __shared__ float s_v[VARIANCE ? LT * LDV : 1];

    // block -> (class, tile).  The class runs fastest in the order v: at step s the classes cx = 8m .. 8m+7 of one tile read the very
    // same 128-byte lines (8 pixels), 16 bytes of each.  Blocks are dealt to the 8 XCDs round robin, each with an L2 of its own, so
    // v is laid out XCD-major: blocks with neighbouring v share an XCD and are launched together, and a line comes in from beyond
    // the L2 once, not once per class.  A matter of speed only (the map is a bijection on [0, gridDim.x) whatever the placement is).
    uint32_t b;
    {
        const uint32_t n = gridDim.x, q = n / 8, r = n % 8, xcd = blockIdx.x % 8;
        b = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + blockIdx.x / 8;
    }
    const uint32_t cx = b % a.classes_x; b /= a.classes_x;
    const uint32_t tx = b % a.tiles_x;   b /= a.tiles_x;
    const uint32_t cy = b % a.classes_y; b /= a.classes_y;
    const uint32_t ty = b;
    const long long s = a.step, W = a.width, H = a.height;
    const long long x0 = cx + s * TILE * tx, y0 = cy + s * TILE * ty;
    if (x0 >= W || y0 >= H) return;  // a class shorter than the longest (the whole block leaves: no barrier is missed)

    const int tid = threadIdx.x;
    for (int e = tid; e < LT * LT; e += TILE * TILE) {
        const int li = e % LT, lj = e / LT;
        const long long x = x0 + s * (li - HALO), y = y0 + s * (lj - HALO);
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);  // outside the image: alpha 0, skipped as a miss is
        float4 n = c;
        float v = 0.f;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t p = static_cast<size_t>(y) * static_cast<size_t>(W) + static_cast<size_t>(x);
            c = a.c_in[p];
            n = a.nd[p];
            if (VARIANCE) v = a.v_in[p].x;
            if (a.demod_in && c.w != 0.f) {
                const float4 al = a.albedo[p];
                c.x = c.x / mx(al.x, 1e-3f);
                c.y = c.y / mx(al.y, 1e-3f);
                c.z = c.z / mx(al.z, 1e-3f);
            }
        }
        s_c[lj * LDC + li] = c;
        s_n[lj * LDC + li] = n;
        if (VARIANCE) s_v[lj * LDV + li] = v;
    }
    __syncthreads();

    const int i = tid % TILE, j = tid / TILE;
    const long long x = x0 + s * i, y = y0 + s * j;
    if (x >= W || y >= H) return;
    const size_t p = static_cast<size_t>(y) * static_cast<size_t>(W) + static_cast<size_t>(x);
    const float4 cp = s_c[(j + HALO) * LDC + i + HALO];
    const float vp = VARIANCE ? s_v[(j + HALO) * LDV + i + HALO] : 0.f;
    if (cp.w == 0.f) {  // a miss goes through unchanged
        a.c_out[p] = cp;
        if (VARIANCE && a.v_out) a.v_out[p] = make_float4(vp, 0.f, 0.f, 0.f);
        return;
    }
    const float4 np = s_n[(j + HALO) * LDC + i + HALO];
    const float lp = (cp.x + cp.y) + cp.z;
    float den = a.sigma_l;
    if (VARIANCE) den = a.sigma_l * sqrtf(mx(vp, 0.f)) + 1e-6f;

    float sw = 0.f, sx = 0.f, sy = 0.f, sz = 0.f, sv = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            constexpr float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
            const float hw = h[dx + 2] * h[dy + 2];
            const int at = (j + HALO + dy) * LDC + i + HALO + dx;
            const float4 cq = s_c[at];
            if (cq.w == 0.f) continue;  // a miss, or outside the image
            float w = hw;
            if (dx != 0 || dy != 0) {
                const float4 nq = s_n[at];
                const float d = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
                float wn = mx(d, 0.f);
                for (uint32_t r = 0; r < a.k; ++r) wn = wn * wn;
                // wn == 0 makes w +0 or NaN, which is +0 too: the tap adds nothing, whatever wz and wl are (wz, wl <= 1 or NaN)
                if (!(wn > 0.f)) continue;
                const float ta = fabsf(np.w - nq.w) / a.sd;
                const float wz = 1.f / (1.f + ta * ta);
                const float lq = (cq.x + cq.y) + cq.z;
                const float tb = fabsf(lp - lq) / den;
                const float wl = 1.f / (1.f + tb * tb);
                w = ((hw * wn) * wz) * wl;
                if (!(w == w)) w = 0.f;
                if (w == 0.f) continue;
            }
            sw = sw + w;
            sx = sx + w * cq.x;
            sy = sy + w * cq.y;
            sz = sz + w * cq.z;
            if (VARIANCE) sv = sv + (w * w) * s_v[(j + HALO + dy) * LDV + i + HALO + dx];
        }
    }
    float4 o = make_float4(sx / sw, sy / sw, sz / sw, cp.w);
    if (a.demod_out) {
        const float4 al = a.albedo[p];
        o.x = o.x * mx(al.x, 1e-3f);
        o.y = o.y * mx(al.y, 1e-3f);
        o.z = o.z * mx(al.z, 1e-3f);
    }
    a.c_out[p] = o;
    if (VARIANCE && a.v_out) a.v_out[p] = make_float4(sv / (sw * sw), 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(256) void moments_kernel(const float4* __restrict__ shade, const float4* __restrict__ shade_sq,
                                                      float4* __restrict__ var, size_t pixels, float count) {
    const size_t p = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
    if (p >= pixels) return;
    const float4 s1 = shade[p];
    const float alpha = s1.w;
    float v = 0.f;
    if (alpha != 0.f) {
        const float m = s1.x / alpha;
        const float q = shade_sq[p].x / alpha;
        v = mx(q - m * m, 0.f) / (count * alpha);
    }
    var[p] = make_float4(v, 0.f, 0.f, 0.f);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
namespace {

constexpr size_t kSettingsPublished = offsetof(mpd_settings, flags) + sizeof(uint32_t);

// Everything mpd_atrous refuses by its settings alone; nullptr = accepted.
const char* settings_refusal(const mpd_settings* st) {
    if (!st) return "settings is NULL";
    if (st->struct_size < kSettingsPublished) return "bad struct_size";
    if (st->width == 0 || st->height == 0) return "width * height == 0";
    if (st->width > MPD_MAX_DIM || st->height > MPD_MAX_DIM) return "width or height above MPD_MAX_DIM";
    if (st->iterations < 1 || st->iterations > MPD_MAX_ITERATIONS) return "iterations outside 1..8";
    const float k = st->sigma_normal_pow2;
    if (!(k >= 0.f && k <= 8.f) || k != static_cast<float>(static_cast<int>(k))) return "sigma_normal_pow2 is not a whole number in 0..8";
    if (!(st->sigma_depth > 0.f)) return "sigma_depth is not > 0";
    if (!(st->sigma_luminance > 0.f)) return "sigma_luminance is not > 0";
    if (st->flags & ~MPD_FLAG_DEMODULATE_ALBEDO) return "unknown flag";
    return nullptr;
}

uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

}  // namespace
}  // namespace mpd

using namespace mpd;

extern "C" {

const char* mpd_last_error(void) { return g_last_error.c_str(); }
uint32_t mpd_settings_size(void) { return static_cast<uint32_t>(sizeof(mpd_settings)); }

size_t mpd_scratch_floats(const mpd_settings* st, int with_variance) {
    if (settings_refusal(st)) return 0;
    const size_t plane = static_cast<size_t>(st->width) * st->height * 4;
    return (with_variance ? 4 : 2) * plane;
}

int mpd_last_kernels(char* buf, size_t cap, size_t* needed) {
    return guarded([&]() -> int { return copy_last_kernels(buf, cap, needed); });
}

int mpd_atrous(int device_id, const mpd_settings* st, const float* d_color, const float* d_normal_depth, const float* d_albedo,
               const float* d_variance, float* d_scratch, float* d_out, float* d_variance_out, void* stream) {
    return guarded([&]() -> int {
        if (const char* why = settings_refusal(st)) return fail(MP_ERR_INVALID, why);
        if (device_id < 0) return fail(MP_ERR_INVALID, "negative device_id");
        if (!d_color || !d_normal_depth || !d_scratch || !d_out) return fail(MP_ERR_INVALID, "NULL argument");
        const bool demod = (st->flags & MPD_FLAG_DEMODULATE_ALBEDO) != 0;
        if (demod && !d_albedo) return fail(MP_ERR_INVALID, "MPD_FLAG_DEMODULATE_ALBEDO without d_albedo");
        if (d_variance_out && !d_variance) return fail(MP_ERR_INVALID, "d_variance_out without d_variance");
        const void* others[] = {d_color, d_normal_depth, d_albedo, d_variance, d_scratch};
        for (const void* o : others)
            if (o && (o == d_out || o == d_variance_out)) return fail(MP_ERR_INVALID, "an output aliases another argument");
        if (d_variance_out == d_out) return fail(MP_ERR_INVALID, "d_variance_out aliases d_out");
        if (!all_aligned({d_color, d_normal_depth, d_albedo, d_variance, d_scratch, d_out, d_variance_out}, kPlaneAlign))
            return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");

        const uint32_t W = st->width, H = st->height;
        const size_t plane = static_cast<size_t>(W) * H;  // in pixels (float4)
        float4* scratch = reinterpret_cast<float4*>(d_scratch);
        float4* c_buf[2] = {scratch, scratch + plane};
        float4* v_buf[2] = {scratch + 2 * plane, scratch + 3 * plane};
        const bool variance = d_variance != nullptr;

        DeviceScope dev;
        if (hipError_t e = dev.enter(device_id); e != hipSuccess) return hip_fail(e, "hipSetDevice");
        LaunchLog log;
        for (uint32_t i = 0; i < st->iterations; ++i) {
            const bool last = i + 1 == st->iterations;
            PassArgs a{};
            a.c_in = i == 0 ? reinterpret_cast<const float4*>(d_color) : c_buf[(i - 1) & 1];
            a.v_in = i == 0 ? reinterpret_cast<const float4*>(d_variance) : v_buf[(i - 1) & 1];
            a.c_out = last ? reinterpret_cast<float4*>(d_out) : c_buf[i & 1];
            a.v_out = last ? reinterpret_cast<float4*>(d_variance_out) : v_buf[i & 1];
            a.nd = reinterpret_cast<const float4*>(d_normal_depth);
            a.albedo = reinterpret_cast<const float4*>(d_albedo);
            a.width = W;
            a.height = H;
            a.step = 1u << i;
            a.classes_x = std::min(a.step, W);
            a.classes_y = std::min(a.step, H);
            a.tiles_x = ceil_div(ceil_div(W, a.step), TILE);
            a.tiles_y = ceil_div(ceil_div(H, a.step), TILE);
            a.k = static_cast<uint32_t>(st->sigma_normal_pow2);
            a.sd = st->sigma_depth * static_cast<float>(a.step);
            a.sigma_l = st->sigma_luminance;
            a.demod_in = demod && i == 0;
            a.demod_out = demod && last;
            // at most (2^20 / 16 + 128)^2 < 2^33 in principle; a grid is one dimension of at most 2^31 - 1 blocks
            const uint64_t blocks = static_cast<uint64_t>(a.classes_x) * a.tiles_x * a.classes_y * a.tiles_y;
            if (blocks > 0x7FFFFFFFull) return fail(MP_ERR_UNSUPPORTED, "image too large for one launch per pass");
            const dim3 grid(static_cast<uint32_t>(blocks)), block(TILE * TILE);
            const int rc = variance ? launch(log, "atrous_kernel<true>", atrous_kernel<true>, grid, block, stream, a)
                                    : launch(log, "atrous_kernel<false>", atrous_kernel<false>, grid, block, stream, a);
            if (rc != MP_OK) return rc;
        }
        return MP_OK;
    });
}

int mpd_variance_from_moments(int device_id, uint32_t width, uint32_t height, uint32_t sample_count, const float* d_shade,
                              const float* d_shade_sq, float* d_variance, void* stream) {
    return guarded([&]() -> int {
        if (!d_shade || !d_shade_sq || !d_variance) return fail(MP_ERR_INVALID, "NULL argument");
        if (width == 0 || height == 0) return fail(MP_ERR_INVALID, "width * height == 0");
        if (width > MPD_MAX_DIM || height > MPD_MAX_DIM) return fail(MP_ERR_INVALID, "width or height above MPD_MAX_DIM");
        if (sample_count == 0) return fail(MP_ERR_INVALID, "sample_count == 0");
        if (device_id < 0) return fail(MP_ERR_INVALID, "negative device_id");
        if (d_variance == d_shade || d_variance == d_shade_sq) return fail(MP_ERR_INVALID, "d_variance aliases an input");
        if (!all_aligned({d_shade, d_shade_sq, d_variance}, kPlaneAlign)) return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");
        const size_t pixels = static_cast<size_t>(width) * height;
        const size_t blocks = (pixels + 255) / 256;
        if (blocks > 0x7FFFFFFFull) return fail(MP_ERR_UNSUPPORTED, "image too large for one launch");
        DeviceScope dev;
        if (hipError_t e = dev.enter(device_id); e != hipSuccess) return hip_fail(e, "hipSetDevice");
        LaunchLog log;
        return launch(log, "moments_kernel", moments_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(256), stream,
                      reinterpret_cast<const float4*>(d_shade), reinterpret_cast<const float4*>(d_shade_sq),
                      reinterpret_cast<float4*>(d_variance), pixels, static_cast<float>(sample_count));
    });
}

}  // extern "C"
