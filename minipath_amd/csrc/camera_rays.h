// A camera ray from its film point and lens point: the arithmetic of CameraSampler::sample_ray (camera.rs:178-191) after its random
// draws, and Ray::new.  A header of its own because two callers must compute the very same f32 values: sample_ray_rng (wave_common.h),
// which feeds it the sample's draws, and the mask cache's corner rays (mask_cache_begin_unit, mask_cache.h), which feed it the
// corners of a work unit's footprint.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/minipath_hip.h"
#include "ray_math.h"

namespace mp {
namespace mc {

// (Ray = a struct of the nine floats ox, oy, oz, dx, dy, dz, ix, iy, iz: the walk's mc::Ray, mask_cache.h)
// geometry/mod.rs:45-54 (the short division / sqrt sequences where they are exact: ray_math.h)
template <class Ray>
__device__ __forceinline__ void ray_new(float ox, float oy, float oz, float dx, float dy, float dz, Ray& r) {
    r.ox = ox; r.oy = oy; r.oz = oz;
    rm::ray_dir(dx, dy, dz, r.dx, r.dy, r.dz, r.ix, r.iy, r.iz);
}
// CameraSampler::sample_ray camera.rs:178-191 from the film point (film_u, film_v) and the lens point lens_radius * (x1, x2) on, in
// the two halves that sample_ray_rng (wave_common.h) puts around its lens draw
__device__ __forceinline__ void camera_film(const mp_camera_sampler& s, float film_u, float film_v, float (&f)[3]) {
    float fv = film_v * s.pixel_scale, fu = film_u * s.pixel_scale;
    f[0] = s.film_origin_offset[0] + s.up[0] * fv - s.right[0] * fu;
    f[1] = s.film_origin_offset[1] + s.up[1] * fv - s.right[1] * fu;
    f[2] = s.film_origin_offset[2] + s.up[2] * fv - s.right[2] * fu;
}
template <class Ray>
__device__ __forceinline__ void camera_lens_ray(const mp_camera_sampler& s, const float (&f)[3], float x1, float x2, Ray& r) {
    float a = s.lens_radius * x1, b = s.lens_radius * x2;
    float lx = s.right[0] * a + s.up[0] * b;
    float ly = s.right[1] * a + s.up[1] * b;
    float lz = s.right[2] * a + s.up[2] * b;
    ray_new(s.center[0] + lx, s.center[1] + ly, s.center[2] + lz, lx * s.lens_weight - f[0], ly * s.lens_weight - f[1],
            lz * s.lens_weight - f[2], r);
}

}  // namespace mc
}  // namespace mp
