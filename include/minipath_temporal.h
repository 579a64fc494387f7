/* minipath_temporal.h -- C ABI of libminipath_temporal.so: temporal reprojection of [h, w, 4] float images across camera moves,
 * the temporal stage of an SVGF-style reconstruction (spatiotemporal variance-guided filtering).  It carries colour and the two
 * luminance moments of a pixel from the previous frame to the current one through the world-space hit point of the "position"
 * plane of mp_render_aov_pass_device (include/minipath_hip.h), and hands mpd_atrous (include/minipath_denoise.h) a temporal
 * variance.  Scenes are static: the hit point is its own correspondence, there are no motion vectors.
 *
 * A library of its own: it knows images and views, no mp_ctx, no scene, no mp_camera.  libminipath_hip.so does not know of it.
 *
 * Conventions (those of minipath_hip.h and minipath_denoise.h)
 *   - plain C types, pointers and sizes only;
 *   - every function that can fail returns an int status, MP_OK == 0, with the values of minipath_hip.h; no exception or abort
 *     crosses the ABI (every body runs inside a catch-all: std::bad_alloc -> MP_ERR_NOMEM, anything else -> MP_ERR_INVALID); the
 *     message of the last failure on the calling thread is mpt_last_error();
 *   - "d_" pointers are device (HBM) pointers on the GPU `device_id`, 16-byte aligned: a pointer that is
 *     not is refused (MP_ERR_INVALID) before the first HIP call;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call is asynchronous on it;
 *   - every plane is image-major [height][width][4], 16 bytes per pixel, as mp_untile writes it (FrameRenderer.untile_plane): pixel
 *     (x, y) is at element index (y * width + x) * 4.
 *
 * Planes.  Of the CURRENT frame:
 *     color     f32 {r, g, b, a}           the image to accumulate (any max_depth); .w is passed through
 *     position  f32 {p.x, p.y, p.z, alpha} the untiled MEAN of the hit points: xyz is weighted by coverage, alpha = the fraction of
 *                                          the samples that hit; alpha == 0 marks a MISS pixel, anything else (NaN too) is a hit
 *     normal    f32 {n.x, n.y, n.z, t}     the "normal" plane, coverage-weighted means like position: .w is the mean hit distance
 *     ids       u32 {prim, instance, material, hit}   the record of sample 0
 *     variance_in  f32 {v, -, -, -}        nullable: the caller's variance of the pixel's mean for pixels with a young history (e.g.
 *                                          mpd_variance_from_moments); only .x is read
 *   Of the PREVIOUS frame: prev_position, prev_normal, prev_ids (its guide planes as they were given then), hist_color (its `out`)
 *   and hist_moments (its `moments_out`): f32 {m1, m2, N, 0}, the accumulated first and second moment of the luminance and the
 *   history length.
 *
 * View.  mpt_view is the pinhole through the lens centre of a CameraSampler: `center`, and the unit vectors `forward`, `right`, `up`
 *   of the camera; k = focal_length / pixel_scale; cx = (float)(width - 1) * 0.5f, cy = (float)(height - 1) * 0.5f.  The ray through
 *   the lens centre and the film point of pixel coordinates (u, v) has the direction
 *   forward * focal_length + right * (u * pixel_scale - ou) + up * (ov - v * pixel_scale),  ou = cx * pixel_scale, ov = cy * pixel_scale,
 *   so a point with camera coordinates (a, b, c) along (forward, right, up) is seen at u = cx + b * k / a, v = cy - c * k / a.
 *
 * ---- mpt_reproject, operation by operation ---------------------------------------------------------------------------------------
 * All arithmetic is IEEE-754 binary32, round to nearest even, every operation written below rounded once (no contraction into
 * fma, no reciprocal-multiply in place of a divide, subnormals kept).  Only + - * /, floorf and compares occur, so a numpy float32
 * restatement gives the same bits (tests/temporal_model.py is one).
 *   dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z
 *   max(a, c) means  a > c ? a : c  and  min(a, c) means  a < c ? a : c  with c the constant (a setting or a literal): a NaN a
 *   gives c, and max(-0, 0) is +0 (the rule of minipath_denoise.h).
 * For the pixel p = (x, y), W = width, H = height:
 *   1. Miss.  position[p].w == 0:  out[p] = color[p] bit for bit, moments_out[p] = {0, 0, 0, 0}, variance_out[p] = {0, 0, 0, 0};
 *      nothing else is read or done.
 *   2. A = position[p].w;   P.c = position[p].c / A  (c = x, y, z);   tp = normal[p].w / A;   l = (color.x + color.y) + color.z
 *   3. Project P through the PREVIOUS view:
 *        w.c = P.c - center.c;   a = dot(w, forward);   b = dot(w, right);   c = dot(w, up)
 *        !(a > 0): no history
 *        s = k / a;   u = cx + b*s;   v = cy - c*s
 *        !(u > -1 && u < (float)W && v > -1 && v < (float)H): no history  (NaN fails this test)
 *        x0 = (int)floorf(u);  y0 = (int)floorf(v);   fx = u - (float)x0;  fy = v - (float)y0
 *   4. Taps, from sum_w = sum_c.x = sum_c.y = sum_c.z = sum_1 = sum_2 = sum_n = +0.0f, for j = 0, 1 (outer), i = 0, 1 (inner),
 *      q = (x0 + i, y0 + j).  The tap is SKIPPED, in this order of tests, when
 *        q is outside [0, W) x [0, H);
 *        prev_position[q].w == 0  (a miss then);
 *        prev_ids[q].y != ids[p].y  or  prev_ids[q].z != ids[p].z;  with MPT_FLAG_MATCH_PRIM also when prev_ids[q].x != ids[p].x;
 *        !(d2 <= r*r),  where  Q.c = prev_position[q].c / prev_position[q].w,  e.c = Q.c - P.c,  d2 = dot(e, e),
 *                              r = sigma_position * tp;
 *        !(dn >= normal_min * (A * prev_position[q].w)),  where  dn = dot(normal[p], prev_normal[q])  on the raw plane values (both
 *                              are coverage-weighted, hence the product of the alphas on the right);
 *        wt == 0,  where  wx = i ? fx : 1 - fx,   wy = j ? fy : 1 - fy,   wt = wx*wy.
 *      A kept tap adds, in this order:
 *        sum_w += wt;   sum_c.c += wt * hist_color[q].c  (c = x, y, z);
 *        sum_1 += wt * hist_moments[q].x;   sum_2 += wt * hist_moments[q].y;   sum_n += wt * hist_moments[q].z
 *      A skipped tap's hist_color and hist_moments are never read.
 *   5. !(sum_w > 0): no history.
 *      No history:  out[p] = color[p] bit for bit;  moments_out[p] = {l, l*l, 1, 0}.
 *      Otherwise:   h.c = sum_c.c / sum_w;   h1 = sum_1 / sum_w;   h2 = sum_2 / sum_w;   n = sum_n / sum_w
 *                   N  = min(n + 1, max_history)
 *                   ac = max(1 / N, alpha_color);   am = max(1 / N, alpha_moments)
 *                   out[p].c = h.c + ac * (color.c - h.c)  (c = x, y, z);   out[p].w = color.w
 *                   m1 = h1 + am * (l - h1);   m2 = h2 + am * (l*l - h2);   moments_out[p] = {m1, m2, N, 0}
 *   6. variance_out (nullable), with {m1', m2', N'} = moments_out[p] of step 5:
 *        N' >= min_variance_history, or no d_variance_in:  v = max(m2' - m1'*m1', 0)
 *        otherwise:                                        v = variance_in[p].x
 *      variance_out[p] = {v, 0, 0, 0}.
 *
 * mpt_reset is the first frame: step 1, and for every other pixel step 2's l and the "no history" branch of step 5.
 *
 * What follows from the text: a NaN or infinite position ends in "no history" (a NaN alpha is a hit whose P is NaN, so !(a > 0));
 * a NaN previous position fails !(d2 <= r*r) and a NaN normal fails the normal test, so neither is blended; a NaN colour passes
 * through at a no-history pixel and poisons the accumulated value elsewhere.  With alpha_color == alpha_moments == 0 and an
 * identical, integer-aligned previous frame the blend is the running mean and N counts 1, 2, 3, ... up to max_history.  The bits of
 * a NaN RESULT are unspecified.
 *
 * The implementation (minipath_amd/temporal/reproject.hip): one launch of reproject_kernel<VARIANCE_IN> per call, a 256-thread
 * block per 32 x 8 pixel tile, the four taps gathered straight from global memory; mpt_reset is one launch of
 * reset_kernel. */
#ifndef MINIPATH_TEMPORAL_H
#define MINIPATH_TEMPORAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef MP_OK /* the status values of minipath_hip.h */
#define MP_OK 0
#define MP_ERR_INVALID 1
#define MP_ERR_IO 2
#define MP_ERR_BUILD 3
#define MP_ERR_HIP 4
#define MP_ERR_UNSUPPORTED 5
#define MP_ERR_ABORTED 6
#define MP_ERR_NOMEM 7
#endif

#define MPT_FLAG_MATCH_PRIM 1u
#define MPT_MAX_DIM 1048576u /* width and height at most 2^20 each */

typedef struct {
    float center[3], forward[3], right[3], up[3];
    float k;      /* focal_length / pixel_scale */
    float cx, cy; /* (float)(width - 1) * 0.5f, (float)(height - 1) * 0.5f */
} mpt_view;

typedef struct {
    uint32_t struct_size;       /* sizeof(mpt_settings) of the caller; smaller than the struct as first published (through
                                   min_variance_history): MP_ERR_INVALID.  Members beyond it are not read. */
    uint32_t width, height;
    uint32_t flags;             /* MPT_FLAG_MATCH_PRIM; any other bit: MP_ERR_INVALID */
    float sigma_position;       /* > 0 (+inf allowed): a tap's hit point may lie sigma_position * tp from the pixel's */
    float normal_min;           /* finite: the least cosine between the two (mean) normals */
    float max_history;          /* >= 1 (+inf allowed): the history length N stops growing here */
    float alpha_color;          /* in [0, 1]: the least weight of the new colour; 0 = the running mean up to max_history */
    float alpha_moments;        /* in [0, 1]: the same for the luminance moments */
    float min_variance_history; /* >= 0: below this history length the variance is the caller's variance_in, when given */
} mpt_settings;

const char *mpt_last_error(void);
uint32_t mpt_settings_size(void);

/* MP_OK for settings mpt_reproject accepts, else MP_ERR_INVALID with the reason in mpt_last_error(); no HIP call. */
int mpt_check_settings(const mpt_settings *settings);

/* The operation above.  The inputs are only read.  A plane is width * height * 16 bytes; d_out, d_moments_out and d_variance_out
 * must not overlap any other plane of the call, in whole or in part: the operation gathers from the history, so in place is a race.
 *   d_variance_in   nullable
 *   d_variance_out  nullable; must be given with d_variance_in
 * MP_ERR_INVALID: a NULL settings / prev_view / plane other than the two nullable ones, width * height == 0, a width or height above
 * MPT_MAX_DIM, a sigma_position that is not > 0, a normal_min that is not finite, a max_history that is not >= 1, an alpha outside
 * [0, 1], a min_variance_history that is not >= 0 (NaN refused everywhere), a bad struct_size, an unknown flag, a negative
 * device_id, d_variance_in without d_variance_out, an output that overlaps another plane.  All of this is decided before the first
 * HIP call: a refused call launches nothing and writes nothing.  MP_ERR_HIP: the runtime refused the device or the launch. */
int mpt_reproject(int device_id, const mpt_settings *settings, const mpt_view *prev_view,
                  const float *d_color, const float *d_position, const float *d_normal, const uint32_t *d_ids,
                  const float *d_variance_in, /* nullable */
                  const float *d_prev_position, const float *d_prev_normal, const uint32_t *d_prev_ids,
                  const float *d_hist_color, const float *d_hist_moments,
                  float *d_out, float *d_moments_out,
                  float *d_variance_out, /* nullable */
                  void *stream);

/* The first frame of a history.  One launch of reset_kernel.
 * MP_ERR_INVALID: a NULL pointer, width * height == 0, a width or height above MPT_MAX_DIM, a negative device_id, an output that
 * overlaps another plane; decided before the first HIP call. */
int mpt_reset(int device_id, uint32_t width, uint32_t height, const float *d_color, const float *d_position, float *d_out,
              float *d_moments_out, void *stream);

/* As mpd_last_kernels: the kernels of the last call ON THE CALLING THREAD that launched any, by name with their template arguments
 * ("reproject_kernel<true>"), each distinct name once in launch order, separated by '\n'.  The record is made before the launch.
 * A call that launches nothing leaves it as it was.  Copies at most cap - 1 characters and a terminating 0 to buf (nullable when
 * cap is 0); *needed (nullable) = length of the whole text without the 0. */
int mpt_last_kernels(char *buf, size_t cap, size_t *needed);

#ifdef __cplusplus
}
#endif
#endif
