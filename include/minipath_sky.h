/* minipath_sky.h -- C ABI of libminipath_sky.so: sky lighting.  The cosine-distributed rays mps_generate (MPS_MODE_AO,
 * include/minipath_secondary.h) starts on the surfaces of the "position" and "normal" planes are traced once by mp_occluded_rays
 * (include/minipath_hip.h); mps_resolve reduces the answers to a scalar visibility and throws the directions away.  mpe_resolve
 * reduces the same answers once more, with the directions: every ray that escapes looks its direction up in an environment map, and
 * the mean over a pixel's counted samples is the incoming sky radiance under cosine sampling, that is the irradiance / pi, as a plane
 * {E.r, E.g, E.b, alpha} that mpt_reproject (include/minipath_temporal.h) and mpd_atrous (include/minipath_denoise.h) take as a
 * colour.  No ray is traced for it: visibility and sky light come from one mp_occluded_rays call.
 *
 * A library of its own, the seventh over minipath_amd/post/post_abi.h: it knows planes, ray buffers and one environment map, no
 * mp_ctx, no scene, no mp_camera.  libminipath_hip.so and libminipath_secondary.so do not know of it; the caller runs mps_generate and
 * mp_occluded_rays before mpe_resolve (minipath_amd.SkyLight does).
 *
 * Conventions (those of minipath_lights.h)
 *   - plain C types, pointers and sizes only;
 *   - every function that can fail returns an int status, MP_OK == 0, with the values of minipath_hip.h; no exception or abort
 *     crosses the ABI (every body runs inside a catch-all: std::bad_alloc -> MP_ERR_NOMEM, anything else -> MP_ERR_INVALID); the
 *     message of the last failure on the calling thread is mpe_last_error();
 *   - "d_" pointers are device (HBM) pointers on the GPU `device_id`; planes (the map is one) are 16-byte aligned, ray arrays 4-byte
 *     aligned (`occluded` is bytes and has no rule): a pointer that is not is refused (MP_ERR_INVALID) before the first HIP call;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call is asynchronous on it;
 *   - every image plane is image-major [height][width][4], 16 bytes per pixel: pixel p = (x, y) is at element index (y * width + x) * 4.
 *
 * The environment map.  An octahedral map: a device plane `env` of N x N texels, [N][N][4] f32 {r, g, b, unused}, 1 <= N <=
 * MPE_MAX_MAP; texel (x, y) = T[y][x] is at element index (y * N + x) * 4 and its .w is never read.  The unit octahedron
 * |x| + |y| + |z| = 1 is laid flat: the upper half (z >= 0) is the diamond |px| + |py| <= 1 of the square [-1, 1]^2, the four
 * faces of the lower half are folded outwards into the square's corners.  Octahedral and not latitude-longitude on purpose: from a
 * direction to a texel takes + - * /, abs, copysign, floor and compares, all of them exact or correctly rounded in binary32, so a
 * numpy restatement gives the same bits, as for every other library here; atan2 and acos would not.
 * settings.pole is the world axis that is the map's +z (the zenith of a sky map); m is the direction in the map's frame:
 *     pole = 2:  m = (d.x, d.y, d.z)       pole = 1:  m = (d.z, d.x, d.y)       pole = 0:  m = (d.y, d.z, d.x)
 *
 * Ray buffers.  Those of minipath_secondary.h: the ray of pixel p = y * W + x and batch sample b is r = b * (W * H) + p, n = W * H * B
 * elements per array for a batch of B = settings.batch samples, n < 2^31.  mpe_resolve reads dx dy dz tmax (f32) and occluded (u8);
 * the origins are not arguments.  Directions are used as they are (any length: the lookup divides by their l1 norm).
 *
 * ---- mpe_resolve, operation by operation -----------------------------------------------------------------------------------------
 * All arithmetic is IEEE-754 binary32, round to nearest even, every operation written below rounded once (no contraction into fma,
 * no reciprocal-multiply in place of a divide, correctly rounded divide, subnormals kept).  A numpy float32 restatement gives the
 * same bits (tests/sky_model.py is one).  Nf = (float)N.
 * For the pixel p, from E = {+0, +0, +0} and C = +0, or from E = sums[p].xyz and C = sums[p].w with MPE_FLAG_ACCUMULATE, for
 * b = 0 .. B-1 in this order, r = b * (W * H) + p:
 *   1. t = tmax[r].    t > 0:     C = C + 1, and the ray is looked up (steps 2 and 3) if occluded[r] == 0
 *                      t == -1:   C = C + 1, nothing else                          (an unlit sample: counted, never open)
 *                      otherwise (0, -0, any other negative, NaN): nothing         (the rule of mps_resolve)
 *   2. The lookup L(d), d = {dx[r], dy[r], dz[r]}:   m from d by `pole`;   l1 = (|m.x| + |m.y|) + |m.z|
 *        !(l1 > 0) or !(l1 < +inf):  L = {+0, +0, +0}; the sample stays counted and no texel is read (a zero direction, a NaN or an
 *                                    infinite component, an l1 that overflows)
 *        otherwise   px = m.x / l1;   py = m.y / l1
 *                    m.z < 0:   (px, py) = (copysign(1 - |py|, px), copysign(1 - |px|, py)), both from the old values   (the fold;
 *                               m.z == -0 is not folded)
 *                    u = px * 0.5 + 0.5;          v = py * 0.5 + 0.5
 *                    fx = u * Nf - 0.5;           fx = fx > 0 ? fx : 0;        fx = fx < Nf - 1 ? fx : Nf - 1;     fy from v likewise
 *                    x0 = (int)floor(fx);         x1 = min(x0 + 1, N - 1);     wx = fx - (float)x0;                y0, y1, wy likewise
 *                    top.c = T[y0][x0].c * (1 - wx) + T[y0][x1].c * wx;        bot.c likewise on the row y1        (c = r, g, b)
 *                    L.c   = top.c * (1 - wy) + bot.c * wy
 *      The two clamps in the form written send a NaN to 0 and every other value into [0, N - 1], so no index leaves the map for any
 *      input bits.  Borders clamp: the bilinear taps do NOT follow the octahedral wrap across the map's edge, where the lower
 *      hemisphere's faces meet each other.  Only directions within half a texel of that edge are affected: those just below the
 *      horizon (m.z < 0, small), which see the edge texels alone instead of a blend with the texels across the seam.
 *   3. E.c = E.c + L.c   (also for L = {0, 0, 0})
 * Then  sums[p] = {E.r, E.g, E.b, C},  and with a non-null out:
 *     C > 0:  out[p] = {E.r / C, E.g / C, E.b / C, 1};   otherwise  out[p] = {0, 0, 0, 0}.
 * The sum is carried in order through sums, so any split of the samples into batches gives the same bits.  A pixel without a
 * counted sample has alpha 0 and passes through mpt_reproject and mpd_atrous as their misses do.  sample_count <= 65536 keeps C an
 * exactly represented integer.  The texels are used as they are: a NaN or an infinity in the map reaches the sums.
 *
 * ---- mpe_fill_gradient ---------------------------------------------------------------------------------------------------------
 * A sky without an HDR file: writes an N x N octahedral map from three finite colours.  For the texel (i, j) = T[j][i], in binary32:
 *     px = ((i + 0.5) / Nf) * 2 - 1;   py = ((j + 0.5) / Nf) * 2 - 1;   z = (1 - |px|) - |py|
 *     z < 0:  (px, py) = (copysign(1 - |py|, px), copysign(1 - |px|, py)), both from the old values
 *     len = sqrt((px * px + py * py) + z * z);   h = z / len                       (the sine of the elevation above the horizon)
 *     h >= 0:  c = horizon.c + (zenith.c - horizon.c) * h;   otherwise  c = ground.c;       T[j][i] = {c.r, c.g, c.b, 1}
 * (correctly rounded sqrt).  (px, py, z) is the direction, in the map's frame, that the lookup sends to the texel's centre.
 *
 * The implementation (minipath_amd/sky/sky.hip): mpe_resolve is one launch of sky_resolve_kernel<WRITE_OUT>, a thread per pixel in
 * 256-thread blocks over the image in row-major order, mpe_fill_gradient one of sky_gradient_kernel, a thread per texel
 * (DESIGN.md 4.15). */
#ifndef MINIPATH_SKY_H
#define MINIPATH_SKY_H

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

#define MPE_FLAG_ACCUMULATE 1u      /* mpe_resolve continues the sums already in d_sums */
#define MPE_MAX_MAP 8192u           /* map_size at most 8192: a map of at most 1 GiB */
#define MPE_MAX_DIM 1048576u        /* width and height at most 2^20 each */
#define MPE_MAX_SAMPLES 65536u      /* sample_count at most 2^16 */
#define MPE_MAX_RAYS 2147483648ull  /* width * height * batch below 2^31 */

typedef struct {
    uint32_t struct_size;   /* sizeof(mpe_settings) of the caller; smaller than the struct as first published (through pole):
                               MP_ERR_INVALID.  Members beyond it are not read. */
    uint32_t width, height;
    uint32_t flags;         /* MPE_FLAG_ACCUMULATE; any other bit: MP_ERR_INVALID */
    uint32_t sample_count;  /* 1 .. MPE_MAX_SAMPLES: the samples of the whole pass, as given to mps_generate */
    uint32_t sample_begin;  /* the batch holds the samples [sample_begin, sample_begin + batch) of sample_count */
    uint32_t batch;         /* B > 0 */
    uint32_t map_size;      /* N: 1 .. MPE_MAX_MAP */
    uint32_t pole;          /* 0, 1 or 2: the world axis (x, y, z) that is the map's +z */
} mpe_settings;

const char *mpe_last_error(void);
uint32_t mpe_settings_size(void);

/* MP_OK for settings mpe_resolve accepts, else MP_ERR_INVALID with the reason in mpe_last_error(); no HIP call. */
int mpe_check_settings(const mpe_settings *settings);

/* The reduction above.  d_env (map_size * map_size texels), d_dx, d_dy, d_dz, d_tmax (width * height * batch floats each) and
 * d_occluded (as many bytes) are only read; d_sums is a plane, read as well with MPE_FLAG_ACCUMULATE; d_out is a plane or NULL.
 * MP_ERR_INVALID: a NULL pointer other than d_out, width * height == 0, a width or height above MPE_MAX_DIM, batch == 0, width *
 * height * batch >= MPE_MAX_RAYS, sample_count == 0 or above MPE_MAX_SAMPLES, sample_begin + batch > sample_count, map_size == 0 or
 * above MPE_MAX_MAP, pole > 2, an unknown flag, a bad struct_size, a negative device_id, d_env, d_sums or d_out not 16-byte aligned,
 * a ray array not 4-byte aligned, d_sums or d_out overlapping each other, the map or a ray array.  All of this is decided before the
 * first HIP call: a refused call launches nothing and writes nothing.  MP_ERR_HIP: the runtime refused the device or the launch. */
int mpe_resolve(int device_id, const mpe_settings *settings, const float *d_env, const float *d_dx, const float *d_dy,
                const float *d_dz, const float *d_tmax, const uint8_t *d_occluded, float *d_sums, float *d_out /* nullable */,
                void *stream);

/* Writes the map_size x map_size gradient map above to d_env; zenith, horizon and ground are host arrays of three floats, read
 * during the call.  MP_ERR_INVALID: a NULL pointer, map_size == 0 or above MPE_MAX_MAP, a colour component that is not finite, a
 * negative device_id, d_env not 16-byte aligned; decided before the first HIP call. */
int mpe_fill_gradient(int device_id, uint32_t map_size, const float *zenith, const float *horizon, const float *ground,
                      float *d_env, void *stream);

/* As mpl_last_kernels: the kernel of the last call ON THE CALLING THREAD that launched any, by name with its template arguments
 * ("sky_resolve_kernel<false>", "sky_resolve_kernel<true>", "sky_gradient_kernel").  The record is made before the launch.  A call
 * that launches nothing leaves it as it was.  Copies at most cap - 1 characters and a terminating 0 to buf (nullable when cap is
 * 0); *needed (nullable) = length of the whole text without the 0. */
int mpe_last_kernels(char *buf, size_t cap, size_t *needed);

#ifdef __cplusplus
}
#endif
#endif
