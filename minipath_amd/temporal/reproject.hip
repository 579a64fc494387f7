// libminipath_temporal.so: the temporal reprojection of include/minipath_temporal.h -- the kernels and the C ABI over them.
// The header's text is the contract; tests/temporal_model.py restates it in numpy and the kernels must give its bits, so every
// operation below is written out one rounding at a time (built with -ffp-contract=off, correctly rounded divide, subnormals kept:
// the flags of libminipath_hip.so and libminipath_denoise.so).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/minipath_temporal.h"
#include "../post/post_abi.h"

namespace mpt {

// A block takes a TILE_W x TILE_H pixel tile: 32 pixels of 16 bytes are four whole 128-byte lines per row and plane, and a wave is
// two such rows.  Neighbouring pixels project to neighbouring history pixels, so the taps of a block fall on a patch of about the
// same size: they are gathered straight from global memory and meet in the vector cache and the L2.
constexpr int TILE_W = 32;
constexpr int TILE_H = 8;

struct Args {
    const float4* color;
    const float4* position;
    const float4* normal;
    const uint4* ids;
    const float4* var_in;  // VARIANCE_IN
    const float4* prev_position;
    const float4* prev_normal;
    const uint4* prev_ids;
    const float4* hist_color;
    const float4* hist_moments;
    float4* out;
    float4* moments_out;
    float4* var_out;  // nullable
    mpt_view view;    // of the previous frame
    uint32_t width, height, tiles_x;
    uint32_t match_prim;
    float sigma_position, normal_min, max_history, alpha_color, alpha_moments, min_variance_history;
};

// the header's max(a, c) and min(a, c): c for a NaN a
__device__ __forceinline__ float mx(float a, float c) { return a > c ? a : c; }
__device__ __forceinline__ float mn(float a, float c) { return a < c ? a : c; }
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// block -> the pixel of this thread; false outside the image
__device__ __forceinline__ bool pixel_of(uint32_t tiles_x, uint32_t W, uint32_t H, uint32_t& x, uint32_t& y) {
    const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    x = tx * TILE_W + threadIdx.x % TILE_W;
    y = ty * TILE_H + threadIdx.x / TILE_W;
    return x < W && y < H;
}

template <bool VARIANCE_IN>
__global__ __launch_bounds__(TILE_W * TILE_H) void reproject_kernel(const Args a) {
    uint32_t x, y;
    const uint32_t W = a.width, H = a.height;
    if (!pixel_of(a.tiles_x, W, H, x, y)) return;
    const size_t p = static_cast<size_t>(y) * W + x;
    // the pixel's own five loads, all in flight before the first is used
    const float4 col = a.color[p];
    const float4 pos = a.position[p];
    const float4 nrm = a.normal[p];
    const uint4 id = a.ids[p];
    float vin = 0.f;
    if (VARIANCE_IN) vin = a.var_in[p].x;

    if (pos.w == 0.f) {  // 1. a miss
        a.out[p] = col;
        a.moments_out[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.var_out) a.var_out[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    // 2.
    const float A = pos.w;
    const float Px = pos.x / A, Py = pos.y / A, Pz = pos.z / A;
    const float tp = nrm.w / A;
    const float l = (col.x + col.y) + col.z;
    // 3.
    const float wx_ = Px - a.view.center[0], wy_ = Py - a.view.center[1], wz_ = Pz - a.view.center[2];
    const float ca = dot3(wx_, wy_, wz_, a.view.forward[0], a.view.forward[1], a.view.forward[2]);
    const float cb = dot3(wx_, wy_, wz_, a.view.right[0], a.view.right[1], a.view.right[2]);
    const float cc = dot3(wx_, wy_, wz_, a.view.up[0], a.view.up[1], a.view.up[2]);
    float sw = 0.f, sx = 0.f, sy = 0.f, sz = 0.f, s1 = 0.f, s2 = 0.f, sn = 0.f;
    if (ca > 0.f) {
        const float s = a.view.k / ca;
        const float u = a.view.cx + cb * s;
        const float v = a.view.cy - cc * s;
        if (u > -1.f && u < static_cast<float>(W) && v > -1.f && v < static_cast<float>(H)) {
            const float fu = floorf(u), fv = floorf(v);
            const int x0 = static_cast<int>(fu), y0 = static_cast<int>(fv);  // in [-1, W-1] x [-1, H-1]
            const float fx = u - static_cast<float>(x0), fy = v - static_cast<float>(y0);
            // 4. the guides of all four taps first; every address is inside the image
            size_t q[4];
            bool in[4];
            float4 qpos[4], qnrm[4];
            uint4 qid[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int qx = x0 + (t & 1), qy = y0 + (t >> 1);
                in[t] = qx >= 0 && qx < static_cast<int>(W) && qy >= 0 && qy < static_cast<int>(H);
                q[t] = in[t] ? static_cast<size_t>(qy) * W + static_cast<size_t>(qx) : p;
                qpos[t] = make_float4(0.f, 0.f, 0.f, 0.f);  // outside: skipped as a miss is
                qid[t] = make_uint4(0u, 0u, 0u, 0u);
                qnrm[t] = qpos[t];
                if (in[t]) {
                    qid[t] = a.prev_ids[q[t]];
                    qpos[t] = a.prev_position[q[t]];
                    qnrm[t] = a.prev_normal[q[t]];
                }
            }
            const float r = a.sigma_position * tp;
            const float rr = r * r;
            float wt[4];
            bool keep[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float B = qpos[t].w;
                bool k = in[t] && !(B == 0.f);
                k = k && qid[t].y == id.y && qid[t].z == id.z && (!a.match_prim || qid[t].x == id.x);
                const float ex = qpos[t].x / B - Px, ey = qpos[t].y / B - Py, ez = qpos[t].z / B - Pz;
                const float d2 = dot3(ex, ey, ez, ex, ey, ez);
                k = k && d2 <= rr;
                const float dn = dot3(nrm.x, nrm.y, nrm.z, qnrm[t].x, qnrm[t].y, qnrm[t].z);
                k = k && dn >= a.normal_min * (A * B);
                const float wx = (t & 1) ? fx : 1.f - fx;
                const float wy = (t >> 1) ? fy : 1.f - fy;
                wt[t] = wx * wy;
                keep[t] = k && !(wt[t] == 0.f);
            }
            // the history of the kept taps only; the loads of all of them are issued before the sums
            float4 hc[4], hm[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                hc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
                hm[t] = hc[t];
                if (keep[t]) {
                    hc[t] = a.hist_color[q[t]];
                    hm[t] = a.hist_moments[q[t]];
                }
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (keep[t]) {
                    sw = sw + wt[t];
                    sx = sx + wt[t] * hc[t].x;
                    sy = sy + wt[t] * hc[t].y;
                    sz = sz + wt[t] * hc[t].z;
                    s1 = s1 + wt[t] * hm[t].x;
                    s2 = s2 + wt[t] * hm[t].y;
                    sn = sn + wt[t] * hm[t].z;
                }
            }
        }
    }
    // 5.
    float4 o = col;
    float m1 = l, m2 = l * l, N = 1.f;
    if (sw > 0.f) {
        const float hx = sx / sw, hy = sy / sw, hz = sz / sw, h1 = s1 / sw, h2 = s2 / sw, n = sn / sw;
        N = mn(n + 1.f, a.max_history);
        const float ac = mx(1.f / N, a.alpha_color), am = mx(1.f / N, a.alpha_moments);
        o.x = hx + ac * (col.x - hx);
        o.y = hy + ac * (col.y - hy);
        o.z = hz + ac * (col.z - hz);
        m1 = h1 + am * (l - h1);
        m2 = h2 + am * (l * l - h2);
    }
    a.out[p] = o;
    a.moments_out[p] = make_float4(m1, m2, N, 0.f);
    // 6.
    if (a.var_out) {
        float v = mx(m2 - m1 * m1, 0.f);
        if (VARIANCE_IN && !(N >= a.min_variance_history)) v = vin;
        a.var_out[p] = make_float4(v, 0.f, 0.f, 0.f);
    }
}

__global__ __launch_bounds__(TILE_W * TILE_H) void reset_kernel(const float4* __restrict__ color, const float4* __restrict__ position,
                                                                 float4* __restrict__ out, float4* __restrict__ moments_out,
                                                                 uint32_t W, uint32_t H, uint32_t tiles_x) {
    uint32_t x, y;
    if (!pixel_of(tiles_x, W, H, x, y)) return;
    const size_t p = static_cast<size_t>(y) * W + x;
    const float4 col = color[p];
    const float4 pos = position[p];
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!(pos.w == 0.f)) {
        const float l = (col.x + col.y) + col.z;
        m = make_float4(l, l * l, 1.f, 0.f);
    }
    out[p] = col;
    moments_out[p] = m;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
namespace {

constexpr size_t kSettingsPublished = offsetof(mpt_settings, min_variance_history) + sizeof(float);

const char* dims_refusal(uint32_t w, uint32_t h) {
    if (w == 0 || h == 0) return "width * height == 0";
    if (w > MPT_MAX_DIM || h > MPT_MAX_DIM) return "width or height above MPT_MAX_DIM";
    return nullptr;
}

// Everything mpt_reproject refuses by its settings alone; nullptr = accepted.  Every compare is false for a NaN.
const char* settings_refusal(const mpt_settings* st) {
    if (!st) return "settings is NULL";
    if (st->struct_size < kSettingsPublished) return "bad struct_size";
    if (const char* why = dims_refusal(st->width, st->height)) return why;
    if (st->flags & ~MPT_FLAG_MATCH_PRIM) return "unknown flag";
    if (!(st->sigma_position > 0.f)) return "sigma_position is not > 0";
    if (!std::isfinite(st->normal_min)) return "normal_min is not finite";
    if (!(st->max_history >= 1.f)) return "max_history is not >= 1";
    if (!(st->alpha_color >= 0.f && st->alpha_color <= 1.f)) return "alpha_color outside [0, 1]";
    if (!(st->alpha_moments >= 0.f && st->alpha_moments <= 1.f)) return "alpha_moments outside [0, 1]";
    if (!(st->min_variance_history >= 0.f)) return "min_variance_history is not >= 0";
    return nullptr;
}

// Does one of the first n_outs planes, all of `bytes` bytes, share a byte with another plane of the call?  NULL planes are absent.
template <size_t N>
bool planes_overlap(const void* const (&planes)[N], size_t n_outs, size_t bytes) {
    Span spans[N];
    for (size_t i = 0; i < N; ++i) spans[i] = {planes[i], bytes};
    return outputs_overlap(spans, N, n_outs);
}

// the grid of one block per tile; 0 when it is more than one launch can hold
uint32_t grid_of(uint32_t W, uint32_t H, uint32_t& tiles_x) {
    tiles_x = (W + TILE_W - 1) / TILE_W;
    const uint64_t blocks = static_cast<uint64_t>(tiles_x) * ((H + TILE_H - 1) / TILE_H);
    return blocks > 0x7FFFFFFFull ? 0u : static_cast<uint32_t>(blocks);
}

}  // namespace
}  // namespace mpt

using namespace mpt;

extern "C" {

const char* mpt_last_error(void) { return g_last_error.c_str(); }
uint32_t mpt_settings_size(void) { return static_cast<uint32_t>(sizeof(mpt_settings)); }

int mpt_check_settings(const mpt_settings* st) {
    return guarded([&]() -> int {
        if (const char* why = settings_refusal(st)) return fail(MP_ERR_INVALID, why);
        return MP_OK;
    });
}

int mpt_last_kernels(char* buf, size_t cap, size_t* needed) {
    return guarded([&]() -> int { return copy_last_kernels(buf, cap, needed); });
}

int mpt_reproject(int device_id, const mpt_settings* st, const mpt_view* prev_view, const float* d_color, const float* d_position,
                  const float* d_normal, const uint32_t* d_ids, const float* d_variance_in, const float* d_prev_position,
                  const float* d_prev_normal, const uint32_t* d_prev_ids, const float* d_hist_color, const float* d_hist_moments,
                  float* d_out, float* d_moments_out, float* d_variance_out, void* stream) {
    return guarded([&]() -> int {
        if (const char* why = settings_refusal(st)) return fail(MP_ERR_INVALID, why);
        if (device_id < 0) return fail(MP_ERR_INVALID, "negative device_id");
        if (!prev_view) return fail(MP_ERR_INVALID, "prev_view is NULL");
        if (!d_color || !d_position || !d_normal || !d_ids || !d_prev_position || !d_prev_normal || !d_prev_ids || !d_hist_color ||
            !d_hist_moments || !d_out || !d_moments_out)
            return fail(MP_ERR_INVALID, "NULL argument");
        if (d_variance_in && !d_variance_out) return fail(MP_ERR_INVALID, "d_variance_in without d_variance_out");
        const uint32_t W = st->width, H = st->height;
        const void* planes[] = {d_out, d_moments_out, d_variance_out, d_color, d_position, d_normal, d_ids, d_variance_in,
                                d_prev_position, d_prev_normal, d_prev_ids, d_hist_color, d_hist_moments};
        if (planes_overlap(planes, 3, static_cast<size_t>(W) * H * 16))
            return fail(MP_ERR_INVALID, "an output overlaps another plane of the call");
        if (!all_aligned({d_out, d_moments_out, d_variance_out, d_color, d_position, d_normal, d_ids, d_variance_in, d_prev_position,
                          d_prev_normal, d_prev_ids, d_hist_color, d_hist_moments}, kPlaneAlign))
            return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");
        Args a{};
        const uint32_t blocks = grid_of(W, H, a.tiles_x);
        if (!blocks) return fail(MP_ERR_UNSUPPORTED, "image too large for one launch");
        a.color = reinterpret_cast<const float4*>(d_color);
        a.position = reinterpret_cast<const float4*>(d_position);
        a.normal = reinterpret_cast<const float4*>(d_normal);
        a.ids = reinterpret_cast<const uint4*>(d_ids);
        a.var_in = reinterpret_cast<const float4*>(d_variance_in);
        a.prev_position = reinterpret_cast<const float4*>(d_prev_position);
        a.prev_normal = reinterpret_cast<const float4*>(d_prev_normal);
        a.prev_ids = reinterpret_cast<const uint4*>(d_prev_ids);
        a.hist_color = reinterpret_cast<const float4*>(d_hist_color);
        a.hist_moments = reinterpret_cast<const float4*>(d_hist_moments);
        a.out = reinterpret_cast<float4*>(d_out);
        a.moments_out = reinterpret_cast<float4*>(d_moments_out);
        a.var_out = reinterpret_cast<float4*>(d_variance_out);
        a.view = *prev_view;
        a.width = W;
        a.height = H;
        a.match_prim = (st->flags & MPT_FLAG_MATCH_PRIM) ? 1u : 0u;
        a.sigma_position = st->sigma_position;
        a.normal_min = st->normal_min;
        a.max_history = st->max_history;
        a.alpha_color = st->alpha_color;
        a.alpha_moments = st->alpha_moments;
        a.min_variance_history = st->min_variance_history;

        DeviceScope dev;
        if (hipError_t e = dev.enter(device_id); e != hipSuccess) return hip_fail(e, "hipSetDevice");
        const dim3 grid(blocks), block(TILE_W * TILE_H);
        LaunchLog log;
        return d_variance_in ? launch(log, "reproject_kernel<true>", reproject_kernel<true>, grid, block, stream, a)
                             : launch(log, "reproject_kernel<false>", reproject_kernel<false>, grid, block, stream, a);
    });
}

int mpt_reset(int device_id, uint32_t width, uint32_t height, const float* d_color, const float* d_position, float* d_out,
              float* d_moments_out, void* stream) {
    return guarded([&]() -> int {
        if (!d_color || !d_position || !d_out || !d_moments_out) return fail(MP_ERR_INVALID, "NULL argument");
        if (const char* why = dims_refusal(width, height)) return fail(MP_ERR_INVALID, why);
        if (device_id < 0) return fail(MP_ERR_INVALID, "negative device_id");
        const void* planes[] = {d_out, d_moments_out, d_color, d_position};
        if (planes_overlap(planes, 2, static_cast<size_t>(width) * height * 16))
            return fail(MP_ERR_INVALID, "an output overlaps another plane of the call");
        if (!all_aligned({d_out, d_moments_out, d_color, d_position}, kPlaneAlign))
            return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");
        uint32_t tiles_x;
        const uint32_t blocks = grid_of(width, height, tiles_x);
        if (!blocks) return fail(MP_ERR_UNSUPPORTED, "image too large for one launch");
        DeviceScope dev;
        if (hipError_t e = dev.enter(device_id); e != hipSuccess) return hip_fail(e, "hipSetDevice");
        LaunchLog log;
        return launch(log, "reset_kernel", reset_kernel, dim3(blocks), dim3(TILE_W * TILE_H), stream,
                      reinterpret_cast<const float4*>(d_color), reinterpret_cast<const float4*>(d_position),
                      reinterpret_cast<float4*>(d_out), reinterpret_cast<float4*>(d_moments_out), width, height, tiles_x);
    });
}

}  // extern "C"
