/* minipath_resample.h -- C ABI of libminipath_resample.so: guided half-resolution resampling.  mpr_downsample picks one real surface
 * point per f x f block of the full-resolution "position" and "normal" planes of mp_render_aov_pass_device (include/minipath_hip.h)
 * and copies the planes' words there to low-resolution planes, on which mps_generate (include/minipath_secondary.h) starts its rays;
 * mpr_upsample brings a low-resolution colour -- the visibility plane of mps_resolve -- back to full resolution with a 3 x 3 filter
 * over the low pixels that weighs each by the full-resolution geometry.  Its result passes through mpt_reproject
 * (include/minipath_temporal.h) and mpd_atrous (include/minipath_denoise.h) as a colour.
 *
 * A library of its own: it knows planes only, no mp_ctx, no scene, no mp_camera.  libminipath_hip.so does not know of it.
 *
 * Conventions (those of minipath_hip.h, minipath_denoise.h, minipath_temporal.h and minipath_secondary.h)
 *   - plain C types, pointers and sizes only;
 *   - every function that can fail returns an int status, MP_OK == 0, with the values of minipath_hip.h; no exception or abort
 *     crosses the ABI (every body runs inside a catch-all: std::bad_alloc -> MP_ERR_NOMEM, anything else -> MP_ERR_INVALID); the
 *     message of the last failure on the calling thread is mpr_last_error();
 *   - "d_" pointers are device (HBM) pointers on the GPU `device_id`; planes are 16-byte aligned, `picks` 4-byte aligned:
 *     a pointer that is not is refused (MP_ERR_INVALID) before the first HIP call;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call is asynchronous on it;
 *   - every plane is image-major [height][width][4], 16 bytes per pixel, as mp_untile writes it (FrameRenderer.untile_plane): pixel
 *     p = (x, y) is at element index (y * width + x) * 4.
 *
 * Sizes.  W = width, H = height (the full resolution), f = factor; the low resolution is w = ceil(W / f), h = ceil(H / f)
 * (mpr_low_size).  Low pixel (X, Y) owns the block x' in [f X, min(f X + f, W)), y' in [f Y, min(f Y + f, H)): never empty.
 *
 * Planes read:  position f32 {p.x, p.y, p.z, alpha}  and  normal f32 {n.x, n.y, n.z, t}, the untiled coverage-weighted means of the
 * first hits as minipath_temporal.h describes them (every member carries the factor alpha).
 *
 * All arithmetic is IEEE-754 binary32, round to nearest even, every operation written below rounded once (no contraction into fma,
 * no reciprocal-multiply in place of a divide, subnormals kept).  Only + - * /, sqrtf, fabsf and compares occur, so a numpy float32
 * restatement gives the same bits (tests/resample_model.py is one).
 *   max(a, 0) means  a > 0 ? a : 0  (the denoiser's: a NaN a gives 0, and max(-0, 0) is +0)
 *   dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z
 *
 * ---- mpr_downsample, operation by operation ----------------------------------------------------------------------------------------
 * Pixel q = (x', y') of the full-resolution planes is VALID when  A = position[q].w  has  A > 0  and  dot(N, N) > 0  for
 * N = normal[q].xyz: the two NONE rules of mps_generate, so a picked pixel is exactly one that generates live rays.
 * For the low pixel (X, Y):
 *   MPR_PICK_PHASE.    The candidate is (f X + phase % f, f Y + phase / f).  Inside the image and valid: it is picked.  Otherwise the
 *                      first valid pixel of the block in row-major scan order (y' outer, x' inner) is picked.
 *   MPR_PICK_NEAREST.  d = normal[q].w / A.  Scanning the block in row-major order, a valid pixel replaces the pick when there is
 *                      none yet, or when d < d_best (then d_best = d).  Equal depths: the first wins.  A NaN depth never replaces and,
 *                      once picked (as the first valid pixel), is never replaced.  `phase` is not used (and still checked).
 *   No valid pixel:    picks[Y * w + X] = MPR_PICK_NONE and every destination plane gets 16 zero bytes at (X, Y).
 *   Otherwise:         picks[Y * w + X] = y' * W + x'  and every destination plane gets the four words of its source plane at
 *                      (x', y'), bit for bit (words are copied, not computed with: an int32 "ids" plane, NaN payloads and -0 survive).
 * Every word of picks and of every destination is written.  The position and normal planes are guides only; to have them at low
 * resolution pass them as source planes as well (minipath_amd.GuidedResampler does).
 *
 * ---- mpr_upsample, operation by operation -------------------------------------------------------------------------------------------
 * Reads the full-resolution position and normal, and at low resolution position_lo, normal_lo, picks -- as mpr_downsample wrote
 * them, but taken as caller data: nothing is assumed of them, no address depends on their contents -- and color_lo {r, g, b, alpha}.
 * For the full pixel p = (x, y):
 *   1. A = position[p].w.  !(A > 0): out[p] = {0, 0, 0, 0}.
 *   2. P.c = position[p].c / A  (c = x, y, z);   N = normal[p].xyz;   l2 = dot(N, N).   !(l2 > 0): out[p] = {0, 0, 0, 0}.
 *      n.c = N.c / sqrtf(l2);   tp = normal[p].w / A;   sd = sigma_plane * tp.
 *   3. sum_w = sum_c.x = sum_c.y = sum_c.z = +0.0f, the nearest-tap record empty.  For dY = -1..1 (outer), dX = -1..1 (inner):
 *      q = (x / f + dX, y / f + dY)  (integer division).  The tap is SKIPPED when
 *        q is outside [0, w) x [0, h),  or  picks[q] == MPR_PICK_NONE or picks[q] >= W * H,  or  color_lo[q].w == 0,  or
 *        !(position_lo[q].w > 0),  or  !(dot(Nq, Nq) > 0)  for Nq = normal_lo[q].xyz.
 *      Otherwise
 *        (xq, yq) = (picks[q] % W, picks[q] / W);   ddx = (float)(x - xq);   ddy = (float)(y - yq);   d2 = ddx*ddx + ddy*ddy
 *            (integers below 2^24 and so exact whenever the pick lies within 2^11 pixels, as every pick of mpr_downsample does)
 *        ws = 1 / (1 + d2 / (float)(f*f))
 *        Pq.c = position_lo[q].c / position_lo[q].w;   nq.c = Nq.c / sqrtf(dot(Nq, Nq))
 *        wn = max(dot(n, nq), 0);  then  wn = wn * wn  repeated k = sigma_normal_pow2 times
 *        e  = dot(n, Pq - P)  (the difference componentwise);   a = fabsf(e) / sd;   wp = 1 / (1 + a*a)
 *        w  = (ws * wn) * wp;   if w is NaN: w = +0.0f
 *      The first non-skipped tap with the smallest d2 (a later tap replaces the record only with d2 < d2_nearest; a NaN d2 cannot
 *      occur) is remembered as the nearest tap, whatever its w.  If w == 0 the tap adds nothing.  Otherwise, in this order:
 *        sum_w = sum_w + w;   sum_c.c = sum_c.c + w * color_lo[q].c  (c = x, y, z)
 *   4. sum_w > 0:                     out[p] = {sum_c.x / sum_w, sum_c.y / sum_w, sum_c.z / sum_w, 1.0f}
 *      else, a nearest tap q exists:  out[p] = {color_lo[q].x, .y, .z (the colour's bits), 1.0f}
 *      else:                          out[p] = {0, 0, 0, 0}: a hole; the caller's filters see a miss there.
 * Every word of out is written.
 *
 * What follows from the text.  The picked pixel of a block sees its own tap with ws = 1 and with the same point and normal: e = +-0,
 * wp = 1, wn = dot(n, n) squared k times, which is 1 to within a few 2^k ulp.  A NaN in position[p].xyz makes e and so every w a NaN,
 * that is +0: the pixel takes the nearest tap's colour.  A NaN alpha or a NaN in normal[p].xyz fails the compares of 1. and 2.: a
 * zero pixel.  A NaN in normal[p].w, or tp == 0 (sd == 0: a = x / 0 is +inf or NaN), makes every w +0 as well: the nearest tap.  A
 * negative tp gives the weights of -tp (a enters squared).  sigma_plane = +inf with tp > 0 makes a = 0 and wp = 1 for every finite e:
 * the plane weight is switched off.  A NaN in position_lo[q].xyz or normal_lo[q].xyz makes that tap's w +0; the tap can still be the
 * nearest.  A NaN or infinite colour behind a zero weight does not leak; behind a non-zero weight, or as the nearest tap's colour, it
 * is passed on, and the bits of a NaN that arithmetic produced (sum_c / sum_w) are unspecified.  Both normals are normalised here,
 * so ws, wn and wp are at most 1 to within rounding and sum_w stays below 10: no weight overflows, as the denoiser's can.
 *
 * The implementation (minipath_amd/resample/resample.hip): mpr_downsample is one launch of downsample_kernel<PICK>, a thread per low
 * pixel; mpr_upsample one of upsample_kernel, a 256-thread block per 16 x 16 full-resolution tile, which first stages what depends
 * on a low pixel alone -- the skip test, Pq, nq, (xq, yq), the colour -- once per low pixel in LDS. */
#ifndef MINIPATH_RESAMPLE_H
#define MINIPATH_RESAMPLE_H

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

#define MPR_PICK_PHASE 0u
#define MPR_PICK_NEAREST 1u
#define MPR_PICK_NONE 0xFFFFFFFFu  /* the word of `picks` for a block without a valid pixel */
#define MPR_MAX_PLANES 4u          /* (source, destination) pairs of one mpr_downsample call */
#define MPR_MIN_FACTOR 2u
#define MPR_MAX_FACTOR 4u
#define MPR_MAX_DIM 1048576u       /* width and height at most 2^20 each */
#define MPR_MAX_PIXELS 4294967294ull /* width * height at most 2^32 - 2: a pick y' * W + x' is a word below MPR_PICK_NONE */

typedef struct {
    uint32_t struct_size;     /* sizeof(mpr_settings) of the caller; smaller than the struct as first published (through sigma_plane):
                                 MP_ERR_INVALID.  Members beyond it are not read. */
    uint32_t width, height;   /* W, H: the full resolution */
    uint32_t factor;          /* f in MPR_MIN_FACTOR .. MPR_MAX_FACTOR */
    uint32_t pick_mode;       /* MPR_PICK_PHASE or MPR_PICK_NEAREST; read by mpr_downsample, checked by both */
    uint32_t phase;           /* < f * f; read by mpr_downsample in MPR_PICK_PHASE, checked by both in both modes */
    float sigma_normal_pow2;  /* k, a whole number in 0..8; read by mpr_upsample, checked by both */
    float sigma_plane;        /* > 0, +inf allowed: the distance from the pixel's tangent plane, as a fraction of the pixel's hit
                                 distance, at which wp = 1/2; read by mpr_upsample, checked by both */
} mpr_settings;

const char *mpr_last_error(void);
uint32_t mpr_settings_size(void);

/* MP_OK for settings mpr_downsample and mpr_upsample accept, else MP_ERR_INVALID with the reason in mpr_last_error(); no HIP call. */
int mpr_check_settings(const mpr_settings *settings);

/* *low_width = ceil(W / f), *low_height = ceil(H / f).  MP_ERR_INVALID: refused settings, a NULL pointer.  No HIP call. */
int mpr_low_size(const mpr_settings *settings, uint32_t *low_width, uint32_t *low_height);

/* The picks above.  d_position and d_normal are full-resolution planes and only read.  d_sources and d_destinations are HOST arrays
 * of n_planes device pointers each (both may be NULL when n_planes == 0): d_sources[i] is a full-resolution plane, only read (it may
 * be d_position or d_normal), d_destinations[i] a low-resolution plane.  d_picks holds w * h words.
 * MP_ERR_INVALID: a NULL pointer, W * H == 0, a width or height above MPR_MAX_DIM, W * H above MPR_MAX_PIXELS, a factor outside
 * 2..4, an unknown pick mode, phase >= f * f, sigma_normal_pow2 not a whole number in 0..8, a sigma_plane that is not > 0 (NaN
 * included), a bad struct_size, a negative device_id, n_planes > MPR_MAX_PLANES, a NULL member of a pair, d_picks or a destination
 * overlapping another buffer of the call (byte ranges from the sizes above).  All of this is decided before the first HIP call: a
 * refused call launches nothing and writes nothing.  MP_ERR_HIP: the runtime refused the device or the launch. */
int mpr_downsample(int device_id, const mpr_settings *settings, const float *d_position, const float *d_normal, uint32_t n_planes,
                   const void *const *d_sources, void *const *d_destinations, uint32_t *d_picks, void *stream);

/* The filter above.  d_position, d_normal: full resolution; d_position_lo, d_normal_lo, d_color_lo (planes) and d_picks (w * h
 * words): low resolution; all six are only read.  d_out is a full-resolution plane.
 * MP_ERR_INVALID: as mpr_downsample for the settings and device_id, a NULL pointer, d_out overlapping another buffer of the call;
 * decided before the first HIP call. */
int mpr_upsample(int device_id, const mpr_settings *settings, const float *d_position, const float *d_normal,
                 const float *d_position_lo, const float *d_normal_lo, const uint32_t *d_picks, const float *d_color_lo, float *d_out,
                 void *stream);

/* As mps_last_kernels: the kernel of the last call ON THE CALLING THREAD that launched any, by name with its template arguments
 * ("downsample_kernel<0>", "downsample_kernel<1>", "upsample_kernel").  The record is made before the launch.  A call that launches
 * nothing leaves it as it was.  Copies at most cap - 1 characters and a terminating 0 to buf (nullable when cap is 0); *needed
 * (nullable) = length of the whole text without the 0. */
int mpr_last_kernels(char *buf, size_t cap, size_t *needed);

#ifdef __cplusplus
}
#endif
#endif
