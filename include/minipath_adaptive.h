/* minipath_adaptive.h -- C ABI of libminipath_adaptive.so: the three device operations of adaptive sampling over the tile-major
 * first-hit planes of mp_render_aov_pass_device (include/minipath_hip.h): a per-tile convergence test on the two moment planes,
 * a whole-slot move between plane buffers (gather, scatter, permutation), and the scaling of stopped tiles to their means.
 *
 * A library of its own: it works on planes, not scenes, and needs no mp_ctx.  libminipath_hip.so does not know of it.  The driver
 * over it is minipath_amd.adaptive.AdaptiveSampler.
 *
 * Conventions (those of minipath_hip.h and minipath_denoise.h)
 *   - plain C types, pointers and sizes only;
 *   - every function that can fail returns an int status, MP_OK == 0, with the values of minipath_hip.h; no exception or abort
 *     crosses the ABI (every body runs inside a catch-all: std::bad_alloc -> MP_ERR_NOMEM, anything else -> MP_ERR_INVALID); the
 *     message of the last failure on the calling thread is mpa_last_error();
 *   - "d_" pointers are device (HBM) pointers on the GPU `device_id`;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call is asynchronous on it, and no host memory
 *     is read after a call returns;
 *   - every refusal is decided before the first HIP call: a refused call launches nothing and writes nothing.
 *
 * Planes are TILE-MAJOR, as the render writes them: with ts = tile_size, slot i starts at float index i * ts * ts * 4, and pixel
 * (x, y) of a slot sits at (y * ts + x) * 4 from there (16 bytes per pixel).  A plane buffer (d_shade, d_shade_sq, d_src, d_dst, d_plane) is
 * 16-byte aligned: one that is not is refused (MP_ERR_INVALID) before the first HIP call.  The extent (w, h) of slot i is d_tile_wh[i] = {w, h}
 * (u32[n][2]; a value above ts counts as ts): the slot OWNS the pixels x < w, y < h.  The rest of the slot is neither read nor
 * written by mpa_tile_error and mpa_finish_tiles; mpa_move_tiles moves whole slots. */
#ifndef MINIPATH_ADAPTIVE_H
#define MINIPATH_ADAPTIVE_H

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

#define MPA_MAX_TILE_SIZE 65535u /* a slot's pixel count fits 32 bits */

const char *mpa_last_error(void);

/* The convergence test.  d_shade and d_shade_sq hold the state of the "shade" and "shade_sq" planes after k = samples_done
 * samples of an unfinished pass sequence: {sum, sum, sum, hits}.  Only .x is read: s = the sum of the pixel's shade values c,
 * q = the sum of fl(c * c), over its k samples (a miss adds +0).
 *
 * Per owned pixel, every operation IEEE-754 binary32, round to nearest even, rounded once (no contraction, a true divide and
 * sqrtf, subnormals kept); max(a, b) means  a > b ? a : b  (as in minipath_denoise.h: b for a NaN a, +0 for max(-0, 0)):
 *     r  = 1.0f / (float)k
 *     m  = s * r
 *     m2 = q * r
 *     d  = m2 - m * m
 *     v  = max(d, 0) * r
 *     e  = sqrtf(v) / (m + floor)
 * e is the standard error of the pixel's value over ALL k samples, misses included (so the coverage noise of a silhouette counts;
 * mpd_variance_from_moments conditions on the hits and does not count it), relative to the value itself with a floor.  An all-miss
 * pixel gives exactly +0.
 *   A pixel is OPEN iff !(e <= threshold): a NaN e is open, and a negative threshold leaves every pixel open (e of a pixel the
 *   render wrote is never negative).
 *   d_open[i]    = the number of open owned pixels of slot i.
 *   d_max_err[i] = the maximum of e' over the owned pixels of slot i, where e' = +inf for a NaN e and e otherwise, in the order
 *                  -inf < ... < -0 < +0 < ... < +inf.  That order is total on the operands, so the result does not depend on
 *                  the order of the reduction.  (Moments a render wrote give e >= +0; a negative e needs m + floor < 0.)
 *                  A slot that owns no pixel (w == 0 or h == 0) gives open 0 and max_err +0.
 * What follows from the text: a NaN s gives a NaN e (open, +inf); a NaN q alone gives d = NaN, which max() clamps to 0 as it does
 * a negative difference, so e = +0 (the render cannot write a NaN q without a NaN s); an infinite s gives e = +0.
 * Every slot's two outputs are written by the call: nothing needs zeroing first and no atomics are used.
 *
 * MP_ERR_INVALID: a NULL pointer, n_slots == 0, tile_size == 0, samples_done == 0, a NaN threshold, a floor that is not finite
 * and > 0, a negative device_id, an output equal to an input or to the other output.  MP_ERR_UNSUPPORTED: a tile_size above
 * MPA_MAX_TILE_SIZE, more than 2^31 - 1 slots.  MP_ERR_HIP: the runtime refused the device or the launch.
 * One launch of tile_error_kernel, one 256-thread block per slot. */
int mpa_tile_error(int device_id, uint32_t tile_size, uint32_t n_slots, uint32_t samples_done, float threshold, float floor,
                   const float *d_shade,      /* [n_slots][ts][ts][4] */
                   const float *d_shade_sq,   /* [n_slots][ts][ts][4] */
                   const uint32_t *d_tile_wh, /* [n_slots][2] */
                   uint32_t *d_open,          /* [n_slots] */
                   float *d_max_err,          /* [n_slots] */
                   void *stream);

/* For j < n: copies the whole slot src_slot[j] of d_src to slot dst_slot[j] of d_dst -- ts * ts pixels of 16 bytes, bit patterns
 * untouched, so the int32 "ids" plane travels the same way.  A NULL index array means the identity (j).  d_src holds src_slots
 * slots and d_dst dst_slots: an index >= its buffer's slot count makes the kernel skip that j (its neighbours still move; nothing
 * is accessed out of bounds).  Distinct destination slots and buffers that do not overlap are the caller's contract.  This one
 * primitive is the gather (d_src_slot = the active tiles, d_dst_slot = NULL), the scatter back (the other way round) and a
 * permutation.
 *
 * MP_ERR_INVALID: a NULL d_src or d_dst, d_src == d_dst, tile_size == 0, src_slots == 0 or dst_slots == 0, a negative device_id.
 * n == 0 is MP_OK and launches nothing.  MP_ERR_UNSUPPORTED: a tile_size above MPA_MAX_TILE_SIZE, or more blocks (n * ceil(ts^2 / 1024))
 * than one launch takes (2^31 - 1).  One launch of move_tiles_kernel. */
int mpa_move_tiles(int device_id, uint32_t tile_size, uint32_t n,
                   const void *d_src, uint32_t src_slots, const uint32_t *d_src_slot, /* u32[n] or NULL */
                   void *d_dst, uint32_t dst_slots, const uint32_t *d_dst_slot,       /* u32[n] or NULL */
                   void *stream);

/* Turns the running sums of stopped tiles into means, in place.  d_samples[i] = k_i, the samples slot i holds.
 *   0 < k_i < sample_count:  every float of every owned pixel becomes  value * (1.0f / (float)k_i)  -- the operation of
 *                            mp_untile_preview, so a stopped tile gets exactly the bits its preview after k_i samples has;
 *   k_i == sample_count:     untouched (the render's last pass already left the means);
 *   k_i == 0:                untouched;       k_i > sample_count: skipped.
 *
 * MP_ERR_INVALID: a NULL pointer, n_slots == 0, tile_size == 0, sample_count == 0, a negative device_id, d_plane equal to
 * d_samples or d_tile_wh.  MP_ERR_UNSUPPORTED as for mpa_move_tiles.  One launch of finish_tiles_kernel. */
int mpa_finish_tiles(int device_id, uint32_t tile_size, uint32_t n_slots, uint32_t sample_count,
                     float *d_plane,            /* [n_slots][ts][ts][4] */
                     const uint32_t *d_samples, /* [n_slots] */
                     const uint32_t *d_tile_wh, /* [n_slots][2] */
                     void *stream);

/* As mpd_last_kernels: the kernels of the last call ON THE CALLING THREAD that launched any, by name, each distinct name once in
 * launch order, separated by '\n'.  The record is made before the launch.  A call that launches nothing leaves it as it was.
 * Copies at most cap - 1 characters and a terminating 0 to buf (nullable when cap is 0); *needed (nullable) = length of the whole
 * text without the 0. */
int mpa_last_kernels(char *buf, size_t cap, size_t *needed);

#ifdef __cplusplus
}
#endif
#endif
