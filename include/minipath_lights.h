/* minipath_lights.h -- C ABI of libminipath_lights.so: point and sphere lights.  Bounded shadow rays are started on the surfaces the
 * "position" and "normal" planes of mp_render_aov_pass_device describe (include/minipath_hip.h), one per light and sample, each
 * ending at the light (its centre, or a point of the disc a sphere light shows to the surface), written as the SoA device buffers
 * mp_occluded_rays takes; the query's answers are reduced to a per-pixel irradiance plane (the cosine over the squared distance,
 * times the light's radiant intensity, summed over the lights that are seen) that mpt_reproject (include/minipath_temporal.h) and
 * mpd_atrous (include/minipath_denoise.h) take as a colour.
 *
 * A library of its own, the sixth over minipath_amd/post/post_abi.h: it knows planes, ray buffers and a light table, no mp_ctx, no
 * scene, no mp_camera.  libminipath_hip.so and libminipath_secondary.so do not know of it; the caller runs mp_occluded_rays between
 * mpl_generate and mpl_resolve (minipath_amd.LocalLights does).
 *
 * Conventions (those of minipath_secondary.h)
 *   - plain C types, pointers and sizes only;
 *   - every function that can fail returns an int status, MP_OK == 0, with the values of minipath_hip.h; no exception or abort
 *     crosses the ABI; the message of the last failure on the calling thread is mpl_last_error();
 *   - "d_" pointers are device (HBM) pointers on the GPU `device_id`; planes are 16-byte aligned, ray arrays 4-byte aligned
 *     (`occluded` is bytes and has no rule): a pointer that is not is refused (MP_ERR_INVALID) before the first HIP call;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call is asynchronous on it;
 *   - every plane is image-major [height][width][4], 16 bytes per pixel: pixel p = (x, y) is at element index (y * width + x) * 4.
 *
 * Planes read:  position f32 {p.x, p.y, p.z, alpha}  and  normal f32 {n.x, n.y, n.z, t}, as minipath_secondary.h reads them.
 *
 * The light table.  `lights` is a HOST array of L = settings.light_count records, 1 <= L <= MPL_MAX_LIGHTS, read during the call
 * and not kept: the table travels to the kernels by value in the kernel arguments (it is the same for every thread, so it is read
 * through the scalar unit), and lights need no device allocation.  radius == 0 is a point light, radius > 0 a sphere light;
 * intensity is the rgb radiant intensity (power per solid angle), finite and >= 0; reserved must be 0.
 *
 * Ray buffers.  Eight f32 arrays ox oy oz dx dy dz tmax weight and one u8 array occluded, each of n = W * H * B * L elements for a
 * batch of B = settings.batch samples (W = width, H = height), n < 2^31.  The ray of pixel p = y * W + x, batch sample b and light l is
 *     r = (b * L + l) * (W * H) + p                                                          (sample-major, then light-major)
 * so neighbouring pixels are neighbouring rays of every (sample, light) slab.
 *
 * ---- mpl_generate, operation by operation ----------------------------------------------------------------------------------------
 * All arithmetic is IEEE-754 binary32, round to nearest even, every operation written below rounded once (no contraction into fma,
 * no reciprocal-multiply in place of a divide, correctly rounded divide and sqrt, subnormals kept).  dot(a, b) and basis(m) are
 * exactly those of minipath_secondary.h.  A numpy float32 restatement gives the same bits (tests/lights_model.py is one).
 * For the pixel p = (x, y), the sample s = sample_begin + b, b < B, and the light l < L:
 *   1. A = position[p].w.  !(A > 0): the pixel is NONE: every ray of the pixel gets o = d = {0, 0, 0}, tmax = 0, weight = 0, and no
 *      random number is drawn (a miss, a negative or a NaN alpha).
 *   2. P.c = position[p].c / A  (c = x, y, z);   N = normal[p].xyz;   l2 = dot(N, N).   !(l2 > 0): the pixel is NONE.
 *      n.c = N.c / sqrt(l2);   w.c = P.c - eye.c;   dot(w, n) > 0: n = -n   (steps 1 and 2 of mps_generate);   o.c = P.c + n.c*bias
 *   3. key = mix(seed) + ((y * W + x) * sample_count + s)  in u64, wrapping ("Seeded mode" of minipath_hip.h); the Xoshiro256++
 *      stream is seeded from key.  For l = 0 .. L-1 in this order one rand_distr::UnitDisc rejection sample (u, v) is drawn from it
 *      if and only if radius_l > 0.  The draws depend on the table and on (p, s) alone, never on what a light's ray turns out to be.
 *   4. For the light l, with c = position_l, R = radius_l:
 *        w.c = c.c - o.c;   q2 = dot(w, w)
 *        R > 0 (sphere):  !(q2 > R*R): the ray is UNLIT (the point is inside the light).  Otherwise
 *                         m.c = w.c / sqrt(q2);   (t, bt) = basis(m);   ur = u*R;   vr = v*R;   g.c = c.c + (t.c*ur + bt.c*vr)
 *        R == 0 (point):  g = c
 *        d.c = g.c - o.c;   dd = dot(d, d);   len = sqrt(dd);   nd = dot(n, d)
 *        !(nd > 0), !(dd > 0) or !(len - margin > 0): the ray is UNLIT.
 *        otherwise  tmax = len - margin;   weight = nd / (dd * len)      (the cosine over the squared distance)
 *      d is stored as computed, not normalised: Ray::new normalises it inside the query, so tmax is a distance.
 *      An UNLIT ray gets o = d = {0, 0, 0}, tmax = -1, weight = 0.
 *   5. Every word of the eight arrays is written for every ray of the batch; `occluded` is not an argument.
 *
 * The trace in the middle.  mp_occluded_rays is given the first seven arrays as they are, with their per-ray tmax.  By its own
 * contract it does not walk a ray with tmax <= 0 and reports 0 for it.
 *
 * ---- mpl_resolve -----------------------------------------------------------------------------------------------------------------
 * For the pixel p, from E = {+0, +0, +0} and C = +0, or from E = sums[p].xyz and C = sums[p].w with MPL_FLAG_ACCUMULATE, for
 * b = 0 .. B-1 in this order:
 *     t0 = tmax of the ray (b, 0):   t0 > 0 or t0 == -1:   C = C + 1                (the sample of a hit pixel: counted once)
 *     for l = 0 .. L-1 in this order, r = (b * L + l) * (W * H) + p:
 *         tmax[r] > 0 and occluded[r] == 0:   E.c = E.c + intensity_l.c * weight[r]   (c = r, g, b; product and sum rounded once each)
 * Then  sums[p] = {E.r, E.g, E.b, C},  and with a non-null out:
 *     C > 0:  out[p] = {E.r / C, E.g / C, E.b / C, 1};   otherwise  out[p] = {0, 0, 0, 0}.
 * The sum is carried in order through sums, so any split of the samples into batches gives the same bits.  A pixel without a
 * counted sample has alpha 0 and passes through mpt_reproject and mpd_atrous as their misses do.  sample_count <= 65536 keeps C an
 * exactly represented integer.
 *
 * The same seed as a pass of minipath_secondary.h gives the same key and so the same first disc sample: a caller that runs both
 * offsets the seed of one of them.
 *
 * The implementation (minipath_amd/lights/lights.hip): mpl_generate is one launch of light_rays_kernel<SPHERES> (SPHERES = false
 * when every radius is 0: no random number is drawn at all), mpl_resolve one of irradiance_kernel<WRITE_OUT>, a thread per pixel in
 * 256-thread blocks over the image in row-major order. */
#ifndef MINIPATH_LIGHTS_H
#define MINIPATH_LIGHTS_H

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

#define MPL_FLAG_ACCUMULATE 1u      /* mpl_resolve continues the sums already in d_sums */
#define MPL_MAX_LIGHTS 8u           /* light_count at most 8 */
#define MPL_MAX_DIM 1048576u        /* width and height at most 2^20 each */
#define MPL_MAX_SAMPLES 65536u      /* sample_count at most 2^16 */
#define MPL_MAX_RAYS 2147483648ull  /* width * height * batch * light_count below 2^31 */

typedef struct {
    float position[3];  /* finite: the centre */
    float radius;       /* >= 0, finite; 0 = a point light */
    float intensity[3]; /* >= 0, finite: rgb radiant intensity */
    float reserved;     /* must be 0 */
} mpl_light;            /* 32 bytes */

typedef struct {
    uint32_t struct_size;   /* sizeof(mpl_settings) of the caller; smaller than the struct as first published (through margin):
                               MP_ERR_INVALID.  Members beyond it are not read. */
    uint32_t width, height;
    uint32_t flags;         /* MPL_FLAG_ACCUMULATE; any other bit: MP_ERR_INVALID; read by mpl_resolve */
    uint32_t sample_count;  /* 1 .. MPL_MAX_SAMPLES: the samples of the whole pass, the `spp` of the key */
    uint32_t sample_begin;  /* the batch holds the samples [sample_begin, sample_begin + batch) of sample_count */
    uint32_t batch;         /* B > 0 */
    uint32_t light_count;   /* L: 1 .. MPL_MAX_LIGHTS */
    uint64_t seed;
    float eye[3];           /* finite: the point the surfaces were seen from (the lens centre) */
    float bias;             /* >= 0, finite: the origin's offset along the normal */
    float margin;           /* >= 0, finite: the length taken off each shadow ray at the light's end, so that a lamp mesh around
                               the light does not shadow it */
} mpl_settings;

const char *mpl_last_error(void);
uint32_t mpl_settings_size(void);

/* MP_OK for settings and a light table mpl_generate and mpl_resolve accept, else MP_ERR_INVALID with the reason in
 * mpl_last_error(); no HIP call.  `lights` is a host array of settings->light_count records. */
int mpl_check_settings(const mpl_settings *settings, const mpl_light *lights);

/* Steps 1 to 5 above: writes the eight ray arrays, width * height * batch * light_count floats each, from the two planes, which
 * are only read.
 * MP_ERR_INVALID: a NULL pointer, width * height == 0, a width or height above MPL_MAX_DIM, batch == 0, light_count == 0 or above
 * MPL_MAX_LIGHTS, width * height * batch * light_count >= MPL_MAX_RAYS, sample_count == 0 or above MPL_MAX_SAMPLES, sample_begin +
 * batch > sample_count, an unknown flag, a NaN or a non-finite value anywhere in the settings or the lights, a negative radius,
 * intensity, bias or margin, reserved != 0, a bad struct_size, a negative device_id, a ray array that overlaps a plane or another
 * ray array of the call.  All of this is decided before the first HIP call: a refused call launches nothing and writes nothing.
 * MP_ERR_HIP: the runtime refused the device or the launch. */
int mpl_generate(int device_id, const mpl_settings *settings, const mpl_light *lights, const float *d_position, const float *d_normal,
                 float *d_ox, float *d_oy, float *d_oz, float *d_dx, float *d_dy, float *d_dz, float *d_tmax, float *d_weight,
                 void *stream);

/* The reduction above.  d_tmax, d_weight (width * height * batch * light_count floats each) and d_occluded (as many bytes) are
 * only read; d_sums is a plane, read as well with MPL_FLAG_ACCUMULATE; d_out is a plane or NULL.
 * MP_ERR_INVALID: as mpl_generate for the settings, the lights and device_id, a NULL pointer other than d_out, d_sums or d_out
 * overlapping another buffer of the call; decided before the first HIP call. */
int mpl_resolve(int device_id, const mpl_settings *settings, const mpl_light *lights, const float *d_tmax, const float *d_weight,
                const uint8_t *d_occluded, float *d_sums, float *d_out /* nullable */, void *stream);

/* As mps_last_kernels: the kernel of the last call ON THE CALLING THREAD that launched any, by name with its template arguments
 * ("light_rays_kernel<false>", "light_rays_kernel<true>", "irradiance_kernel<false>", "irradiance_kernel<true>").  The record is
 * made before the launch.  A call that launches nothing leaves it as it was.  Copies at most cap - 1 characters and a terminating
 * 0 to buf (nullable when cap is 0); *needed (nullable) = length of the whole text without the 0. */
int mpl_last_kernels(char *buf, size_t cap, size_t *needed);

#ifdef __cplusplus
}
#endif
#endif
