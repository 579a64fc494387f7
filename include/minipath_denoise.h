/* minipath_denoise.h -- C ABI of libminipath_denoise.so: an edge-avoiding a-trous wavelet filter for [h, w, 4] float images,
 * guided by the feature planes of mp_render_aov_device / mp_render_aov_pass_device (include/minipath_hip.h).
 *
 * A library of its own: it filters images, not scenes, and needs no mp_ctx.  libminipath_hip.so does not know of it.
 *
 * Conventions (those of minipath_hip.h)
 *   - plain C types, pointers and sizes only;
 *   - every function that can fail returns an int status, MP_OK == 0, with the values of minipath_hip.h; no exception or abort
 *     crosses the ABI (every body runs inside a catch-all: std::bad_alloc -> MP_ERR_NOMEM, anything else -> MP_ERR_INVALID); the
 *     message of the last failure on the calling thread is mpd_last_error();
 *   - "d_" pointers are device (HBM) pointers on the GPU `device_id`;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call is asynchronous on it;
 *   - images are image-major [height][width][4] f32, 16 bytes per pixel, as mp_untile writes them (FrameRenderer.untile /
 *     untile_plane): pixel (x, y) is at float index (y * width + x) * 4.
 *
 * ---- THE FILTER, operation by operation ---------------------------------------------------------------------------------------
 * All arithmetic is IEEE-754 binary32, round to nearest even, every operation written below rounded once (no contraction into
 * fma, no reciprocal-multiply in place of a divide, subnormals kept).  Only + - * /, sqrtf, fabsf and max occur, so a numpy
 * float32 restatement gives the same bits (tests/denoise_model.py is one).
 *   max(a, b) means  a > b ? a : b  with b the constant: a NaN a gives b, and max(-0, 0) is +0.  (This is fmaxf with the two cases
 *   fmaxf leaves open pinned.)
 *
 * Inputs.   color   {r, g, b, alpha}     alpha == 0 marks a MISS pixel; anything else (NaN too) is a hit
 *           normal  {n.x, n.y, n.z, t}   the "normal" plane: shading normal and hit distance
 *           albedo  {r, g, b, -}         read only with MPD_FLAG_DEMODULATE_ALBEDO
 *           var     {v, -, -, -}         .x = variance of the pixel's mean, in the units of C_0 below; only .x is read
 *
 * C_0.  Without MPD_FLAG_DEMODULATE_ALBEDO C_0 = color.  With it, at every hit pixel and per channel c of x, y, z:
 *           f.c = max(albedo.c, 1e-3f),   C_0.c = color.c / f.c
 *       C_0.w = color.w; a miss pixel keeps color's bits.  V_0 = var: the variance is NOT divided by anything, the caller gives it in
 *       the units of C_0.
 *
 * Pass i = 0 .. iterations-1 reads C_i (and V_i) and writes C_{i+1} (and V_{i+1}); s = 2^i (an integer, (float)s exact).
 *   For the pixel p = (x, y):
 *   - C_i[p].w == 0 (a miss): C_{i+1}[p] = C_i[p] and V_{i+1}[p].x = V_i[p].x, bit for bit.
 *   - otherwise, with  sum_w = sum_c.x = sum_c.y = sum_c.z = sum_v = +0.0f,  for dy = -2..2 (outer), dx = -2..2 (inner):
 *       q = (x + s*dx, y + s*dy)
 *       q outside [0, width) x [0, height): the tap is skipped.   C_i[q].w == 0 (q is a miss): the tap is skipped.
 *       h = {1/16, 1/4, 3/8, 1/4, 1/16};  hw = h[dx+2] * h[dy+2]                                     (exact)
 *       if q == p:  w = hw                                            (the centre tap always has wn = wz = wl = 1)
 *       else
 *         d  = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z
 *         wn = max(d, 0);  then  wn = wn * wn  repeated k = sigma_normal_pow2 times
 *         a  = fabsf(t_p - t_q) / sd,        sd = sigma_depth * (float)s        (one product per pass)
 *         wz = 1 / (1 + a*a)
 *         l(c) = (c.x + c.y) + c.z
 *         b  = fabsf(l(C_i[p]) - l(C_i[q])) / den
 *              den = sigma_luminance * sqrtf(max(V_i[p].x, 0)) + 1e-6f     with a variance plane (one product, one sum)
 *              den = sigma_luminance                                       without
 *         wl = 1 / (1 + b*b)
 *         w  = ((hw * wn) * wz) * wl
 *         if w is NaN: w = +0.0f
 *       if w == 0 the tap adds nothing (for finite colours that is what adding w*C would do; a NaN or infinite colour behind a
 *       zero weight does not leak).  Otherwise, in this order:
 *         sum_w = sum_w + w;   sum_c.c = sum_c.c + w * C_i[q].c  (c = x, y, z);   sum_v = sum_v + (w*w) * V_i[q].x
 *     then  C_{i+1}[p].c = sum_c.c / sum_w,   C_{i+1}[p].w = C_i[p].w,   V_{i+1}[p].x = sum_v / (sum_w * sum_w).
 *     sum_w >= 9/64 > 0 by the centre tap.
 *   V_{i+1}[p].yzw = 0 in every case.
 *
 * Output.  out = C_iterations; with MPD_FLAG_DEMODULATE_ALBEDO, at every hit pixel, out.c = C_iterations.c * f.c (the same f).
 *          variance_out = V_iterations ({v, 0, 0, 0}).
 *
 * What follows from the text: NaN normals or depths make every weight to and from that pixel +0, so such a hit pixel comes out as
 * hw*C / hw of itself; a weight that overflows to +inf (normals far from unit length with k > 0) is used as it is.  The bits of a
 * NaN RESULT (a NaN colour at a hit pixel, inf/inf) are unspecified.
 *
 * The implementation (minipath_amd/denoise/atrous.hip): one launch of atrous_kernel<VARIANCE> per pass, ping-ponging between the
 * halves of d_scratch; pass 0 reads the inputs (and demodulates as it loads), the last pass writes d_out (and re-modulates as it
 * stores).  Each 256-thread block filters a 16 x 16 tile of ONE residue class of the step-s lattice, so its 25 taps are a dense
 * 5 x 5 stencil over a 20 x 20 tile in LDS. */
#ifndef MINIPATH_DENOISE_H
#define MINIPATH_DENOISE_H

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

#define MPD_FLAG_DEMODULATE_ALBEDO 1u
#define MPD_MAX_ITERATIONS 8u
#define MPD_MAX_DIM 1048576u /* width and height at most 2^20 each */

typedef struct {
    uint32_t struct_size;       /* sizeof(mpd_settings) of the caller; smaller than the struct as first published (through flags):
                                   MP_ERR_INVALID.  Members beyond it are not read.  mpd_settings_size() is the library's own. */
    uint32_t width, height;
    uint32_t iterations;        /* 1..8; pass i uses tap spacing 2^i */
    float sigma_normal_pow2;    /* k, a whole number in 0..8: the normal weight is max(0, n_p.n_q) squared k times */
    float sigma_depth;          /* > 0 (+inf allowed: no depth weight) */
    float sigma_luminance;      /* > 0 (+inf allowed: no luminance weight) */
    uint32_t flags;             /* MPD_FLAG_DEMODULATE_ALBEDO; any other bit: MP_ERR_INVALID */
} mpd_settings;

const char *mpd_last_error(void);
uint32_t mpd_settings_size(void);

/* Floats of d_scratch mpd_atrous needs: 2*h*w*4, plus 2*h*w*4 with a variance plane (whatever `iterations` is).  0 for settings
 * mpd_atrous would refuse. */
size_t mpd_scratch_floats(const mpd_settings *settings, int with_variance);

/* The filter above.  The inputs are only read; d_out (and d_variance_out) must not overlap anything else passed.
 *   d_albedo       nullable unless MPD_FLAG_DEMODULATE_ALBEDO
 *   d_variance     nullable: without it the luminance weight uses sigma_luminance alone and no variance is propagated
 *   d_scratch      mpd_scratch_floats(settings, d_variance != NULL) floats, 16-byte aligned like every plane: a misaligned plane
 *                  is refused (MP_ERR_INVALID) before the first HIP call
 *   d_variance_out nullable; must be NULL when d_variance is
 * MP_ERR_INVALID: a NULL settings / d_color / d_normal_depth / d_scratch / d_out, width * height == 0, a width or height above
 * MPD_MAX_DIM, iterations outside 1..8, sigma_normal_pow2 not a whole number in 0..8, a sigma that is not > 0 (NaN included), a
 * bad struct_size, an unknown flag, DEMODULATE without d_albedo, d_variance_out without d_variance, a negative device_id, d_out or
 * d_variance_out equal to another pointer of the call.  All of this is decided before the first HIP call: a refused call launches
 * nothing and writes nothing.  MP_ERR_HIP: the runtime refused the device or a launch. */
int mpd_atrous(int device_id, const mpd_settings *settings,
               const float *d_color,        /* [h,w,4] image-major {r,g,b,alpha} */
               const float *d_normal_depth, /* [h,w,4] {n.x,n.y,n.z,t}: the "normal" plane */
               const float *d_albedo,       /* nullable unless DEMODULATE */
               const float *d_variance,     /* nullable; [h,w,4], .x = variance of the pixel's mean */
               float *d_scratch,            /* 2*h*w*4 floats (+ 2*h*w*4 when d_variance is given) */
               float *d_out,                /* [h,w,4] */
               float *d_variance_out,       /* nullable */
               void *stream);

/* Variance of the pixel's mean from the first and second moment planes of mp_render_aov_pass_device ("shade", "shade_sq":
 * coverage-weighted means over sample_count samples, .w = alpha = the fraction of samples that hit).  Per pixel:
 *     alpha = shade.w;   alpha == 0:  v = +0.0f
 *     else  m = shade.x / alpha;   q = shade_sq.x / alpha;   v = max(q - m*m, 0) / ((float)sample_count * alpha)
 * d_variance[p] = {v, 0, 0, 0}.  One launch of moments_kernel.
 * MP_ERR_INVALID: a NULL pointer, width * height == 0, a width or height above MPD_MAX_DIM, sample_count == 0, a negative
 * device_id, d_variance equal to an input; decided before the first HIP call. */
int mpd_variance_from_moments(int device_id, uint32_t width, uint32_t height, uint32_t sample_count,
                              const float *d_shade, const float *d_shade_sq, float *d_variance, void *stream);

/* As mp_ctx_last_kernels, without a context: the kernels of the last call ON THE CALLING THREAD that launched any, by name with
 * their template arguments ("atrous_kernel<true>"), each distinct name once in launch order, separated by '\n'.  The record is
 * made before the launch.  A call that launches nothing leaves it as it was.  Copies at most cap - 1 characters and a
 * terminating 0 to buf (nullable when cap is 0); *needed (nullable) = length of the whole text without the 0. */
int mpd_last_kernels(char *buf, size_t cap, size_t *needed);

#ifdef __cplusplus
}
#endif
#endif
