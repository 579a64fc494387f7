// libminipath_resample.so: the guided resampling of include/minipath_resample.h -- the kernels and the C ABI over them.  The
// header's text is the contract; tests/resample_model.py restates it in numpy and the kernels must give its bits, so every operation
// below is written out one rounding at a time (built with -ffp-contract=off, correctly rounded divide and sqrt, subnormals kept:
// the flags of libminipath_hip.so).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/minipath_resample.h"
#include "../post/post_abi.h"

namespace mpr {

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
// the header's max(a, 0): 0 for a NaN a, +0 for max(-0, 0)
__device__ __forceinline__ float mx0(float a) { return a > 0.f ? a : 0.f; }
// the header's VALID
__device__ __forceinline__ bool valid(const float4& pos, const float4& nrm) {
    return pos.w > 0.f && dot3(nrm.x, nrm.y, nrm.z, nrm.x, nrm.y, nrm.z) > 0.f;
}

// ---- mpr_downsample ------------------------------------------------------------------------------------------------------
// A thread per low pixel, the low image in row-major order: the stores (picks and every destination) are whole runs per wave, the
// guide loads are f * 16 bytes apart along a row.
constexpr int BLOCK = 256;

struct DownArgs {
    const float4* position;
    const float4* normal;
    const uint4* src[MPR_MAX_PLANES];
    uint4* dst[MPR_MAX_PLANES];
    uint32_t* picks;
    uint32_t W, H, w, h, f, n_planes;
    uint32_t cand_dx, cand_dy;  // phase % f, phase / f
};

template <int PICK>
__global__ __launch_bounds__(BLOCK) void downsample_kernel(const DownArgs a) {
    const size_t lp = static_cast<size_t>(blockIdx.x) * BLOCK + threadIdx.x;
    if (lp >= static_cast<size_t>(a.w) * a.h) return;
    const uint32_t X = static_cast<uint32_t>(lp % a.w), Y = static_cast<uint32_t>(lp / a.w);
    const uint32_t bx0 = X * a.f, by0 = Y * a.f;  // < W, < H: the block is never empty
    const uint32_t bx1 = min(bx0 + a.f, a.W), by1 = min(by0 + a.f, a.H);
    bool have = false;
    size_t pick = 0;
    if (PICK == MPR_PICK_PHASE) {
        // the candidate first; the scan only when it fails
        const uint32_t cx = bx0 + a.cand_dx, cy = by0 + a.cand_dy;
        if (cx < a.W && cy < a.H) {
            const size_t q = static_cast<size_t>(cy) * a.W + cx;
            if (valid(a.position[q], a.normal[q])) {
                have = true;
                pick = q;
            }
        }
        if (!have) {
            for (uint32_t y = by0; y < by1 && !have; ++y)
                for (uint32_t x = bx0; x < bx1; ++x) {
                    const size_t q = static_cast<size_t>(y) * a.W + x;
                    if (valid(a.position[q], a.normal[q])) {
                        have = true;
                        pick = q;
                        break;
                    }
                }
        }
    } else {
        float d_best = 0.f;
        for (uint32_t y = by0; y < by1; ++y)
            for (uint32_t x = bx0; x < bx1; ++x) {
                const size_t q = static_cast<size_t>(y) * a.W + x;
                const float4 pos = a.position[q], nrm = a.normal[q];
                if (!valid(pos, nrm)) continue;
                const float d = nrm.w / pos.w;
                if (!have || d < d_best) {
                    have = true;
                    pick = q;
                    d_best = d;
                }
            }
    }
    // W * H <= MPR_MAX_PIXELS: a pick fits its word
    a.picks[lp] = have ? static_cast<uint32_t>(pick) : MPR_PICK_NONE;
    for (uint32_t i = 0; i < a.n_planes; ++i) a.dst[i][lp] = have ? a.src[i][pick] : make_uint4(0u, 0u, 0u, 0u);
}

// ---- mpr_upsample --------------------------------------------------------------------------------------------------------
// A block takes a TILE x TILE tile of the full image.  Its taps reach the low pixels [x0/f - 1, (x0 + 15)/f + 1] by the same in
// y: at most 8 + 2 = 10 a side (f = 2).  What the header computes from the low pixel alone is done once per low pixel while those
// are staged in LDS, as three float4 planes:
//     s_p {Pq.x, Pq.y, Pq.z, bits of xq}   s_n {nq.x, nq.y, nq.z, bits of yq}   s_c {r, g, b, live ? 1 : 0}
// Row stride LT = 10 entries (40 banks of 64).  A ds_read_b128 is served in groups of 16 lanes holding 4 + 4 + 8 pixels of two
// neighbouring tile rows ({0-3, 12-15} of one, {4-11} of the next), that is at most 8 consecutive low entries of one staged row, or
// the pieces of two rows: one row occupies 8 consecutive 4-bank slots of the 16; the same columns a row further lie 10 slots on
// (mod 16), and over every f, tile origin and lane group the entries of a group fall on distinct slots (enumerated).
constexpr int TILE = 16;
constexpr int LT = 10;

struct UpArgs {
    const float4* position;
    const float4* normal;
    const float4* position_lo;
    const float4* normal_lo;
    const float4* color_lo;
    const uint32_t* picks;
    float4* out;
    uint32_t W, H, w, h, f, k;
    uint32_t tiles_x;
    float ff;           // (float)(f * f)
    float sigma_plane;
};

__global__ __launch_bounds__(TILE * TILE) void upsample_kernel(const UpArgs a) {
    __shared__ float4 s_p[LT * LT];
    __shared__ float4 s_n[LT * LT];
    __shared__ float4 s_c[LT * LT];

    const uint32_t x0 = (blockIdx.x % a.tiles_x) * TILE, y0 = (blockIdx.x / a.tiles_x) * TILE;  // < W, < H
    const int lx0 = static_cast<int>(x0 / a.f) - 1, ly0 = static_cast<int>(y0 / a.f) - 1;
    const int ex = static_cast<int>((x0 + TILE - 1) / a.f) + 2 - lx0, ey = static_cast<int>((y0 + TILE - 1) / a.f) + 2 - ly0;  // the staged extent: <= LT
    const int tid = threadIdx.x;
    const uint64_t full = static_cast<uint64_t>(a.W) * a.H;
    for (int e = tid; e < ex * ey; e += TILE * TILE) {
        const int li = e % ex, lj = e / ex;
        const int qx = lx0 + li, qy = ly0 + lj;
        float4 sp = make_float4(0.f, 0.f, 0.f, 0.f), sn = sp, sc = sp;  // sc.w == 0: skipped
        if (qx >= 0 && qx < static_cast<int>(a.w) && qy >= 0 && qy < static_cast<int>(a.h)) {
            const size_t q = static_cast<size_t>(qy) * a.w + static_cast<size_t>(qx);
            const uint32_t pick = a.picks[q];
            const float4 c = a.color_lo[q], pl = a.position_lo[q], nl = a.normal_lo[q];
            const float l2 = dot3(nl.x, nl.y, nl.z, nl.x, nl.y, nl.z);
            if (pick != MPR_PICK_NONE && pick < full && c.w != 0.f && pl.w > 0.f && l2 > 0.f) {
                const float len = sqrtf(l2);
                sp = make_float4(pl.x / pl.w, pl.y / pl.w, pl.z / pl.w, __int_as_float(static_cast<int>(pick % a.W)));
                sn = make_float4(nl.x / len, nl.y / len, nl.z / len, __int_as_float(static_cast<int>(pick / a.W)));
                sc = make_float4(c.x, c.y, c.z, 1.f);
            }
        }
        s_p[lj * LT + li] = sp;
        s_n[lj * LT + li] = sn;
        s_c[lj * LT + li] = sc;
    }
    __syncthreads();

    const uint32_t x = x0 + tid % TILE, y = y0 + tid / TILE;
    if (x >= a.W || y >= a.H) return;
    const size_t p = static_cast<size_t>(y) * a.W + x;
    const float4 pos = a.position[p], nrm = a.normal[p];
    const float A = pos.w;
    const float l2 = dot3(nrm.x, nrm.y, nrm.z, nrm.x, nrm.y, nrm.z);
    if (!(A > 0.f) || !(l2 > 0.f)) {
        a.out[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float Px = pos.x / A, Py = pos.y / A, Pz = pos.z / A;
    const float len = sqrtf(l2);
    const float nx = nrm.x / len, ny = nrm.y / len, nz = nrm.z / len;
    const float tp = nrm.w / A;
    const float sd = a.sigma_plane * tp;

    const int cx = static_cast<int>(x / a.f) - lx0, cy = static_cast<int>(y / a.f) - ly0;  // the centre tap's entry: 1 .. LT - 2
    float sw = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
    bool near_have = false;
    float near_d2 = 0.f;
    int near_at = 0;
#pragma unroll
    for (int dY = -1; dY <= 1; ++dY) {
#pragma unroll
        for (int dX = -1; dX <= 1; ++dX) {
            const int at = (cy + dY) * LT + cx + dX;
            const float4 cq = s_c[at];
            if (cq.w == 0.f) continue;  // skipped, or outside the low image
            const float4 pq = s_p[at], nq = s_n[at];
            const float ddx = static_cast<float>(static_cast<int>(x) - __float_as_int(pq.w));
            const float ddy = static_cast<float>(static_cast<int>(y) - __float_as_int(nq.w));
            const float d2 = ddx * ddx + ddy * ddy;
            if (!near_have || d2 < near_d2) {
                near_have = true;
                near_d2 = d2;
                near_at = at;
            }
            float wn = mx0(dot3(nx, ny, nz, nq.x, nq.y, nq.z));
            for (uint32_t r = 0; r < a.k; ++r) wn = wn * wn;
            // wn == 0 makes w +0 or NaN, which is +0 too: the tap adds nothing, whatever ws and wp are (both <= 1 or NaN)
            if (!(wn > 0.f)) continue;
            const float ws = 1.f / (1.f + d2 / a.ff);
            const float e = dot3(nx, ny, nz, pq.x - Px, pq.y - Py, pq.z - Pz);
            const float ta = fabsf(e) / sd;
            const float wp = 1.f / (1.f + ta * ta);
            float w = (ws * wn) * wp;
            if (!(w == w)) w = 0.f;
            if (w == 0.f) continue;
            sw = sw + w;
            sx = sx + w * cq.x;
            sy = sy + w * cq.y;
            sz = sz + w * cq.z;
        }
    }
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);  // a hole
    if (sw > 0.f) {
        o = make_float4(sx / sw, sy / sw, sz / sw, 1.f);
    } else if (near_have) {
        const float4 cq = s_c[near_at];
        o = make_float4(cq.x, cq.y, cq.z, 1.f);
    }
    a.out[p] = o;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
namespace {

constexpr size_t kSettingsPublished = offsetof(mpr_settings, sigma_plane) + sizeof(float);

// Everything both calls refuse by the settings alone; nullptr = accepted.  Every compare is false for a NaN.
const char* settings_refusal(const mpr_settings* st) {
    if (!st) return "settings is NULL";
    if (st->struct_size < kSettingsPublished) return "bad struct_size";
    if (st->width == 0 || st->height == 0) return "width * height == 0";
    if (st->width > MPR_MAX_DIM || st->height > MPR_MAX_DIM) return "width or height above MPR_MAX_DIM";
    // a pick y' * W + x' is a word below MPR_PICK_NONE
    if (static_cast<uint64_t>(st->width) * st->height > MPR_MAX_PIXELS) return "width * height above MPR_MAX_PIXELS";
    if (st->factor < MPR_MIN_FACTOR || st->factor > MPR_MAX_FACTOR) return "factor outside 2..4";
    if (st->pick_mode != MPR_PICK_PHASE && st->pick_mode != MPR_PICK_NEAREST) return "unknown pick mode";
    if (st->phase >= st->factor * st->factor) return "phase >= factor * factor";
    const float k = st->sigma_normal_pow2;
    if (!(k >= 0.f && k <= 8.f) || k != static_cast<float>(static_cast<int>(k))) return "sigma_normal_pow2 is not a whole number in 0..8";
    if (!(st->sigma_plane > 0.f)) return "sigma_plane is not > 0";
    return nullptr;
}

struct Sizes {
    uint32_t w, h;
    uint64_t full, low;  // pixels
};
Sizes sizes_of(const mpr_settings* st) {
    Sizes s;
    s.w = (st->width + st->factor - 1) / st->factor;
    s.h = (st->height + st->factor - 1) / st->factor;
    s.full = static_cast<uint64_t>(st->width) * st->height;
    s.low = static_cast<uint64_t>(s.w) * s.h;
    return s;
}

}  // namespace
}  // namespace mpr

using namespace mpr;

extern "C" {

const char* mpr_last_error(void) { return g_last_error.c_str(); }
uint32_t mpr_settings_size(void) { return static_cast<uint32_t>(sizeof(mpr_settings)); }

int mpr_check_settings(const mpr_settings* st) {
    return guarded([&]() -> int {
        if (const char* why = settings_refusal(st)) return fail(MP_ERR_INVALID, why);
        return MP_OK;
    });
}

int mpr_low_size(const mpr_settings* st, uint32_t* low_width, uint32_t* low_height) {
    return guarded([&]() -> int {
        if (const char* why = settings_refusal(st)) return fail(MP_ERR_INVALID, why);
        if (!low_width || !low_height) return fail(MP_ERR_INVALID, "NULL argument");
        const Sizes s = sizes_of(st);
        *low_width = s.w;
        *low_height = s.h;
        return MP_OK;
    });
}

int mpr_last_kernels(char* buf, size_t cap, size_t* needed) {
    return guarded([&]() -> int { return copy_last_kernels(buf, cap, needed); });
}

int mpr_downsample(int device_id, const mpr_settings* st, const float* d_position, const float* d_normal, uint32_t n_planes,
                   const void* const* d_sources, void* const* d_destinations, uint32_t* d_picks, void* stream) {
    return guarded([&]() -> int {
        if (const char* why = settings_refusal(st)) return fail(MP_ERR_INVALID, why);
        if (device_id < 0) return fail(MP_ERR_INVALID, "negative device_id");
        if (n_planes > MPR_MAX_PLANES) return fail(MP_ERR_INVALID, "more than MPR_MAX_PLANES plane pairs");
        if (!d_position || !d_normal || !d_picks || (n_planes && (!d_sources || !d_destinations))) return fail(MP_ERR_INVALID, "NULL argument");
        for (uint32_t i = 0; i < n_planes; ++i)
            if (!d_sources[i] || !d_destinations[i]) return fail(MP_ERR_INVALID, "NULL member of a plane pair");
        const Sizes s = sizes_of(st);
        const size_t plane = static_cast<size_t>(s.full) * 16, plane_lo = static_cast<size_t>(s.low) * 16;
        Span spans[3 + 2 * MPR_MAX_PLANES];
        size_t n = 0;
        spans[n++] = {d_picks, static_cast<size_t>(s.low) * 4};
        for (uint32_t i = 0; i < n_planes; ++i) spans[n++] = {d_destinations[i], plane_lo};
        const size_t n_outs = n;
        spans[n++] = {d_position, plane};
        spans[n++] = {d_normal, plane};
        for (uint32_t i = 0; i < n_planes; ++i) spans[n++] = {d_sources[i], plane};
        if (outputs_overlap(spans, n, n_outs)) return fail(MP_ERR_INVALID, "an output overlaps another buffer of the call");
        bool planes_aligned = all_aligned({d_position, d_normal}, kPlaneAlign);
        for (uint32_t i = 0; i < n_planes; ++i) planes_aligned = planes_aligned && all_aligned({d_sources[i], d_destinations[i]}, kPlaneAlign);
        if (!planes_aligned) return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");
        if (!all_aligned({d_picks}, kWordAlign)) return fail(MP_ERR_INVALID, "d_picks is not 4-byte aligned");
        DownArgs a{};
        a.position = reinterpret_cast<const float4*>(d_position);
        a.normal = reinterpret_cast<const float4*>(d_normal);
        for (uint32_t i = 0; i < n_planes; ++i) {
            a.src[i] = static_cast<const uint4*>(d_sources[i]);
            a.dst[i] = static_cast<uint4*>(d_destinations[i]);
        }
        a.picks = d_picks;
        a.W = st->width; a.H = st->height; a.w = s.w; a.h = s.h; a.f = st->factor;
        a.n_planes = n_planes;
        a.cand_dx = st->phase % st->factor;
        a.cand_dy = st->phase / st->factor;
        const uint64_t blocks = (s.low + BLOCK - 1) / BLOCK;  // < 2^23

        DeviceScope dev;
        if (hipError_t e = dev.enter(device_id); e != hipSuccess) return hip_fail(e, "hipSetDevice");
        const dim3 grid(static_cast<uint32_t>(blocks)), block(BLOCK);
        LaunchLog log;
        return st->pick_mode == MPR_PICK_NEAREST ? launch(log, "downsample_kernel<1>", downsample_kernel<1>, grid, block, stream, a)
                                                 : launch(log, "downsample_kernel<0>", downsample_kernel<0>, grid, block, stream, a);
    });
}

int mpr_upsample(int device_id, const mpr_settings* st, const float* d_position, const float* d_normal, const float* d_position_lo,
                 const float* d_normal_lo, const uint32_t* d_picks, const float* d_color_lo, float* d_out, void* stream) {
    return guarded([&]() -> int {
        if (const char* why = settings_refusal(st)) return fail(MP_ERR_INVALID, why);
        if (device_id < 0) return fail(MP_ERR_INVALID, "negative device_id");
        if (!d_position || !d_normal || !d_position_lo || !d_normal_lo || !d_picks || !d_color_lo || !d_out)
            return fail(MP_ERR_INVALID, "NULL argument");
        const Sizes s = sizes_of(st);
        const size_t plane = static_cast<size_t>(s.full) * 16, plane_lo = static_cast<size_t>(s.low) * 16;
        const Span spans[] = {{d_out, plane}, {d_position, plane}, {d_normal, plane}, {d_position_lo, plane_lo}, {d_normal_lo, plane_lo},
                              {d_color_lo, plane_lo}, {d_picks, static_cast<size_t>(s.low) * 4}};
        if (outputs_overlap(spans, 7, 1)) return fail(MP_ERR_INVALID, "d_out overlaps another buffer of the call");
        if (!all_aligned({d_out, d_position, d_normal, d_position_lo, d_normal_lo, d_color_lo}, kPlaneAlign))
            return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");
        if (!all_aligned({d_picks}, kWordAlign)) return fail(MP_ERR_INVALID, "d_picks is not 4-byte aligned");
        UpArgs a{};
        a.position = reinterpret_cast<const float4*>(d_position);
        a.normal = reinterpret_cast<const float4*>(d_normal);
        a.position_lo = reinterpret_cast<const float4*>(d_position_lo);
        a.normal_lo = reinterpret_cast<const float4*>(d_normal_lo);
        a.color_lo = reinterpret_cast<const float4*>(d_color_lo);
        a.picks = d_picks;
        a.out = reinterpret_cast<float4*>(d_out);
        a.W = st->width; a.H = st->height; a.w = s.w; a.h = s.h; a.f = st->factor;
        a.k = static_cast<uint32_t>(st->sigma_normal_pow2);
        a.tiles_x = (st->width + TILE - 1) / TILE;
        a.ff = static_cast<float>(st->factor * st->factor);
        a.sigma_plane = st->sigma_plane;
        const uint64_t blocks = static_cast<uint64_t>(a.tiles_x) * ((st->height + TILE - 1) / TILE);  // < 2^25

        DeviceScope dev;
        if (hipError_t e = dev.enter(device_id); e != hipSuccess) return hip_fail(e, "hipSetDevice");
        LaunchLog log;
        return launch(log, "upsample_kernel", upsample_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(TILE * TILE), stream, a);
    });
}

}  // extern "C"
