/* minipath_secondary.h -- C ABI of libminipath_secondary.so: deferred secondary visibility.  Rays are started on the surfaces the
 * "position" and "normal" planes of mp_render_aov_pass_device describe (include/minipath_hip.h) -- cosine-distributed about the
 * normal for ambient occlusion, or towards a directional light for a sun shadow --, written as the SoA device buffers
 * mp_occluded_rays takes, and the query's answers are reduced to a per-pixel visibility plane that mpt_reproject
 * (include/minipath_temporal.h) and mpd_atrous (include/minipath_denoise.h) take as it is.
 *
 * A library of its own: it knows planes and ray buffers, no mp_ctx, no scene, no mp_camera.  libminipath_hip.so does not know of it;
 * the caller runs mp_occluded_rays between mps_generate and mps_resolve (minipath_amd.SecondaryVisibility does).
 *
 * Conventions (those of minipath_hip.h, minipath_denoise.h and minipath_temporal.h)
 *   - plain C types, pointers and sizes only;
 *   - every function that can fail returns an int status, MP_OK == 0, with the values of minipath_hip.h; no exception or abort
 *     crosses the ABI (every body runs inside a catch-all: std::bad_alloc -> MP_ERR_NOMEM, anything else -> MP_ERR_INVALID); the
 *     message of the last failure on the calling thread is mps_last_error();
 *   - "d_" pointers are device (HBM) pointers on the GPU `device_id`; planes are 16-byte aligned, ray arrays 4-byte aligned
 *     (`occluded` is bytes and has no rule): a pointer that is not is refused (MP_ERR_INVALID) before the first HIP call;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call is asynchronous on it;
 *   - every plane is image-major [height][width][4], 16 bytes per pixel, as mp_untile writes it (FrameRenderer.untile_plane): pixel
 *     p = (x, y) is at element index (y * width + x) * 4.
 *
 * Planes read:  position f32 {p.x, p.y, p.z, alpha}  and  normal f32 {n.x, n.y, n.z, t}, the untiled coverage-weighted means of the
 * first hits as minipath_temporal.h describes them.
 *
 * Ray buffers.  Seven f32 arrays ox oy oz dx dy dz tmax and one u8 array occluded, each of n = W * H * B elements for a batch of
 * B = settings.batch samples (W = width, H = height).  The ray of pixel (x, y) and batch sample b is
 *     r = b * (W * H) + (y * W + x)                                                                   (sample-major)
 * so neighbouring pixels are neighbouring rays.
 *
 * ---- mps_generate, operation by operation ----------------------------------------------------------------------------------------
 * All arithmetic is IEEE-754 binary32, round to nearest even, every operation written below rounded once (no contraction into fma,
 * no reciprocal-multiply in place of a divide, subnormals kept).  Only + - * /, sqrt, copysign and compares occur, so a numpy
 * float32 restatement gives the same bits (tests/secondary_model.py is one).
 *   dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z
 *   basis(m) -- the orthonormal basis of Duff et al. 2017 about m, as the path extension writes it (minipath_oracle.c,
 *   render_sample_paths_impl; the device's path_vertex):
 *       sg = copysign(1, m.z);   a = -1 / (sg + m.z);   bb = (m.x * m.y) * a
 *       t  = { 1 + ((sg * m.x) * m.x) * a,   sg * bb,                -sg * m.x }
 *       bt = { bb,                           sg + (m.y * m.y) * a,   -m.y      }
 * For the pixel p = (x, y) and the sample s = sample_begin + b, b < B:
 *   1. A = position[p].w.  !(A > 0): the ray is NONE: o = d = {0, 0, 0}, tmax = 0 (a miss, a negative or a NaN alpha).
 *   2. P.c = position[p].c / A  (c = x, y, z);   N = normal[p].xyz;   l2 = dot(N, N).   !(l2 > 0): the ray is NONE.
 *      n.c = N.c / sqrt(l2);   w.c = P.c - eye.c;   dot(w, n) > 0: n = -n   (the normal turned against the pinhole ray from `eye`)
 *   3. key = mix(seed) + ((y * W + x) * sample_count + s)  in u64, wrapping: the rule of "Seeded mode" in minipath_hip.h (mix = the
 *      first SplitMix64 output for the state `seed`);  the Xoshiro256++ stream is seeded from key (four SplitMix64 outputs);
 *      (u, v) = one rand_distr::UnitDisc rejection sample from it, as the path extension draws it.
 *   4. MPS_MODE_AO:   z = sqrt(1 - (u*u + v*v));   (t, bt) = basis(n);
 *                     d.c = (t.c*u + bt.c*v) + n.c*z;   o.c = P.c + n.c*bias;   tmax = radius
 *   5. MPS_MODE_SUN:  L = light, as given (the caller normalises it).
 *                     !(dot(n, L) > 0): the ray is UNLIT: o = d = {0, 0, 0}, tmax = -1.
 *                     otherwise  (t, bt) = basis(L);   us = u*spread;   vs = v*spread;
 *                     d.c = (t.c*us + bt.c*vs) + L.c;   o.c = P.c + n.c*bias;   tmax = radius
 *   6. Every word of the seven arrays is written for every ray of the batch; `occluded` is not an argument.
 * Whether a ray is NONE or UNLIT depends on the pixel alone; only (u, v) depends on the sample.
 *
 * The trace in the middle.  mp_occluded_rays is given the buffers as they are.  By its own contract it does not walk a ray with
 * tmax <= 0 and reports 0 for it, and it clamps tmax to f32::MAX: that is what the two codes (0 and -1) and radius = +inf rely on.
 *
 * ---- mps_resolve -----------------------------------------------------------------------------------------------------------------
 * For the pixel p, from V = C = +0.0f, for b = 0 .. B-1 in this order, r = b * (W * H) + p:
 *     tmax[r] > 0:          C = C + 1;   occluded[r] == 0: V = V + 1
 *     else tmax[r] == -1:   C = C + 1                                           (an unlit sample: counted, never visible)
 *     otherwise (0, -0, any other negative, NaN): nothing
 * With MPS_FLAG_ACCUMULATE:  V = counts[p].x + V;  C = counts[p].y + C  (the counts already there; .z and .w are not read).
 *     counts[p] = {V, C, 0, 0}
 * With a non-null out:  a = C > 0 ? V / C : 1.0f;   out[p] = {a, a, a, C > 0 ? 1.0f : 0.0f}.
 * A pixel without a counted sample has alpha 0 and so passes through mpt_reproject and mpd_atrous as their misses do.
 * sample_count <= 65536 keeps every count an exactly represented integer.
 *
 * The implementation (minipath_amd/secondary/secondary.hip): mps_generate is one launch of secondary_rays_kernel<MODE>, mps_resolve
 * one of resolve_kernel<WRITE_OUT>, a thread per pixel in 256-thread blocks over the image in row-major order. */
#ifndef MINIPATH_SECONDARY_H
#define MINIPATH_SECONDARY_H

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

#define MPS_MODE_AO 0u
#define MPS_MODE_SUN 1u
#define MPS_FLAG_ACCUMULATE 1u      /* mps_resolve adds to the counts already in d_counts */
#define MPS_MAX_DIM 1048576u        /* width and height at most 2^20 each */
#define MPS_MAX_SAMPLES 65536u      /* sample_count at most 2^16 */
#define MPS_MAX_RAYS 2147483648ull  /* width * height * batch below 2^31 */

typedef struct {
    uint32_t struct_size;   /* sizeof(mps_settings) of the caller; smaller than the struct as first published (through spread):
                               MP_ERR_INVALID.  Members beyond it are not read. */
    uint32_t width, height;
    uint32_t mode;          /* MPS_MODE_AO or MPS_MODE_SUN; read by mps_generate */
    uint32_t flags;         /* MPS_FLAG_ACCUMULATE; any other bit: MP_ERR_INVALID; read by mps_resolve */
    uint32_t sample_count;  /* 1 .. MPS_MAX_SAMPLES: the samples of the whole pass, the `spp` of the key */
    uint32_t sample_begin;  /* the batch holds the samples [sample_begin, sample_begin + batch) of sample_count */
    uint32_t batch;         /* B > 0 */
    uint64_t seed;
    float eye[3];           /* finite: the point the surfaces were seen from (the lens centre) */
    float light[3];         /* finite: the direction TOWARDS the light, used as given; MPS_MODE_SUN only, checked in both modes */
    float radius;           /* > 0, +inf allowed: the tmax of every generated ray */
    float bias;             /* >= 0, finite: the origin's offset along the normal; the path extension uses 1e-4 */
    float spread;           /* >= 0, finite: the radius of the light's disc at distance 1 (0 = hard shadows); MPS_MODE_SUN only */
} mps_settings;

const char *mps_last_error(void);
uint32_t mps_settings_size(void);

/* MP_OK for settings mps_generate and mps_resolve accept, else MP_ERR_INVALID with the reason in mps_last_error(); no HIP call. */
int mps_check_settings(const mps_settings *settings);

/* Steps 1 to 6 above: writes the seven ray arrays, width * height * batch floats each, from the two planes, which are only read.
 * MP_ERR_INVALID: a NULL pointer, width * height == 0, a width or height above MPS_MAX_DIM, batch == 0, width * height * batch >=
 * MPS_MAX_RAYS, sample_count == 0 or above MPS_MAX_SAMPLES, sample_begin + batch > sample_count, an unknown mode or flag, a NaN
 * anywhere in the settings, a non-finite eye, light, bias or spread, a radius that is not > 0, a negative bias or spread, a bad
 * struct_size, a negative device_id, a ray array that overlaps a plane or another ray array of the call.  All of this is decided
 * before the first HIP call: a refused call launches nothing and writes nothing.  MP_ERR_HIP: the runtime refused the device or
 * the launch. */
int mps_generate(int device_id, const mps_settings *settings, const float *d_position, const float *d_normal,
                 float *d_ox, float *d_oy, float *d_oz, float *d_dx, float *d_dy, float *d_dz, float *d_tmax, void *stream);

/* The reduction above.  d_tmax (width * height * batch floats) and d_occluded (as many bytes) are only read; d_counts is a plane,
 * read as well with MPS_FLAG_ACCUMULATE; d_out is a plane or NULL.
 * MP_ERR_INVALID: as mps_generate for the settings and device_id, a NULL pointer other than d_out, d_counts or d_out overlapping
 * another buffer of the call; decided before the first HIP call. */
int mps_resolve(int device_id, const mps_settings *settings, const float *d_tmax, const uint8_t *d_occluded, float *d_counts,
                float *d_out /* nullable */, void *stream);

/* As mpt_last_kernels: the kernel of the last call ON THE CALLING THREAD that launched any, by name with its template arguments
 * ("secondary_rays_kernel<0>", "secondary_rays_kernel<1>", "resolve_kernel<false>", "resolve_kernel<true>").  The record is made
 * before the launch.  A call that launches nothing leaves it as it was.  Copies at most cap - 1 characters and a terminating 0 to
 * buf (nullable when cap is 0); *needed (nullable) = length of the whole text without the 0. */
int mps_last_kernels(char *buf, size_t cap, size_t *needed);

#ifdef __cplusplus
}
#endif
#endif
