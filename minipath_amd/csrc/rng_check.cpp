// libmp_rm_host.so: ray_math.h's RNG (v_alignbit_b32 emulated) and its per-pass form of the sample key compiled for the host, for
// tests/test_ray_math_cpu.py and tests/test_sample_key_cpu.py.
#include <cstdint>

#include "ray_math.h"

using namespace mp::rm;

extern "C" {
// n streams seeded with keys[i]; out[i * draws + j] = draw j (Xoshiro256++ high word)
void mp_rm_draws(const uint64_t* keys, int64_t n, int draws, uint32_t* out) {
    for (int64_t i = 0; i < n; i++) {
        Rng r;
        rng_seed(r, keys[i]);
        for (int j = 0; j < draws; j++) out[i * draws + j] = rng_next_u32(r);
    }
}
// The sample key on n tuples, both ways: formula[i] = sample_key_u64(..., s[i]), the 64-bit formula; stepped[i] = the key at sample 0
// plus s[i] on 32-bit halves (key_add_sample), as the cached packet kernels form it per pass.
void mp_rm_sample_keys(const uint64_t* seed, const uint32_t* width, const uint32_t* spp, const uint32_t* x, const uint32_t* y,
                       const uint32_t* s, int64_t n, uint64_t* formula, uint64_t* stepped) {
    for (int64_t i = 0; i < n; i++) {
        formula[i] = sample_key_u64(seed[i], width[i], spp[i], x[i], y[i], s[i]);
        stepped[i] = key_add_sample(sample_key_u64(seed[i], width[i], spp[i], x[i], y[i], 0u), s[i]);
    }
}
// UnitDisc on n streams, both forms: xy[4 i .. 4 i + 3] = (x1, x2) of unit_disc<true>, then of unit_disc<false>; next[2 i] = the draw
// after unit_disc<true>, next[2 i + 1] = the draw after unit_disc<false> and one rng_advance
void mp_rm_unit_disc(const uint64_t* keys, int64_t n, float* xy, uint32_t* next) {
    for (int64_t i = 0; i < n; i++) {
        Rng a, b;
        rng_seed(a, keys[i]);
        b = a;
        unit_disc<true>(a, xy[4 * i + 0], xy[4 * i + 1]);
        next[2 * i] = rng_next_u32(a);
        unit_disc<false>(b, xy[4 * i + 2], xy[4 * i + 3]);
        rng_advance(b);
        next[2 * i + 1] = rng_next_u32(b);
    }
}
}
