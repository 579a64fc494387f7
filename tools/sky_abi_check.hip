// Host check of the argument checking of libminipath_sky.so, a program of its own (nothing of it is loaded into Python; it makes no
// HIP call and opens no GPU): the library's unit is compiled into this program and every refusal of include/minipath_sky.h is walked
// under the sanitizers, with buffers of exactly the sizes the calls state, so a read beyond a settings struct of struct_size bytes or
// beyond a colour of three floats would be reported.
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined tools/sky_abi_check.hip -o sky_abi_check
//   ./sky_abi_check          prints "sky_abi_check: ok" and exits 0, or names the first line that does not hold
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>

#include "../minipath_amd/sky/sky.hip"

#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("sky_abi_check: line %d: %s\n", __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

namespace {

constexpr uint32_t W = 6, H = 5, B = 3, N = 4;
constexpr size_t PLANE = size_t(W) * H * 4, RAYS = size_t(W) * H * B, MAP = size_t(N) * N * 4;  // floats
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

mpe_settings good_settings() {
    mpe_settings st{};
    st.struct_size = sizeof(mpe_settings);
    st.width = W; st.height = H; st.sample_count = 8; st.sample_begin = 2; st.batch = B; st.map_size = N; st.pole = 1;
    return st;
}

struct Buffers {
    std::unique_ptr<float[]> env{new float[MAP]()}, sums{new float[PLANE]()}, out{new float[PLANE]()};
    std::unique_ptr<float[]> ray[4];  // dx dy dz tmax
    std::unique_ptr<uint8_t[]> occluded{new uint8_t[RAYS]()};
    Buffers() {
        for (auto& r : ray) r.reset(new float[RAYS]());
    }
};

// never a real device: a call accepted by mistake would be refused by the runtime, not launched
constexpr int DEV = 1 << 20;

// the call with nothing wrong but argument `at` (in the order of the arguments: env dx dy dz tmax occluded sums out) NULL, or moved
// by `by` bytes, or replaced
int resolve(const mpe_settings* st, Buffers& b, int dev = DEV, int null_at = -1, int move_at = -1, int by = 0, int put_at = -1,
            void* put = nullptr) {
    void* p[8] = {b.env.get(), b.ray[0].get(), b.ray[1].get(), b.ray[2].get(), b.ray[3].get(), b.occluded.get(), b.sums.get(), b.out.get()};
    if (null_at >= 0) p[null_at] = nullptr;
    if (move_at >= 0) p[move_at] = static_cast<char*>(p[move_at]) + by;
    if (put_at >= 0) p[put_at] = put;
    return mpe_resolve(dev, st, static_cast<float*>(p[0]), static_cast<float*>(p[1]), static_cast<float*>(p[2]), static_cast<float*>(p[3]),
                       static_cast<float*>(p[4]), static_cast<uint8_t*>(p[5]), static_cast<float*>(p[6]), static_cast<float*>(p[7]), nullptr);
}

}  // namespace

int main() {
    Buffers b;
    const mpe_settings good = good_settings();
    EXPECT(mpe_settings_size() == 36);
    EXPECT(mpe_check_settings(&good) == MP_OK);

    // every refusal by the settings alone, through both entry points that read them
    int n_bad = 0;
    auto refused = [&](mpe_settings st, const char* why) -> bool {
        ++n_bad;
        return mpe_check_settings(&st) == MP_ERR_INVALID && g_last_error == why && resolve(&st, b) == MP_ERR_INVALID && g_last_error == why;
    };
#define BAD(why, ...)             \
    do {                          \
        mpe_settings st = good;   \
        __VA_ARGS__;              \
        EXPECT(refused(st, why)); \
    } while (0)
    BAD("bad struct_size", st.struct_size = 0);
    BAD("bad struct_size", st.struct_size = 35);
    BAD("width * height == 0", st.width = 0);
    BAD("width * height == 0", st.height = 0);
    BAD("width or height above MPE_MAX_DIM", st.width = MPE_MAX_DIM + 1);
    BAD("width or height above MPE_MAX_DIM", st.height = 0xFFFFFFFFu);
    BAD("batch == 0", st.batch = 0);
    BAD("width * height * batch >= 2^31", st.width = 1u << 20; st.height = 1u << 20);
    BAD("width * height * batch >= 2^31", st.width = 1u << 16; st.height = 1u << 15; st.batch = 1);
    BAD("width * height * batch >= 2^31", st.width = 1u << 10; st.height = 1u << 10; st.batch = 0xFFFFFFFFu);
    BAD("width * height * batch >= 2^31", st.width = 1u << 10; st.height = 1u << 10; st.batch = 2048; st.sample_count = 65536);
    BAD("sample_count outside 1 .. MPE_MAX_SAMPLES", st.sample_count = 0; st.sample_begin = 0);
    BAD("sample_count outside 1 .. MPE_MAX_SAMPLES", st.sample_count = MPE_MAX_SAMPLES + 1);
    BAD("sample_begin + batch > sample_count", st.sample_begin = 6);
    BAD("sample_begin + batch > sample_count", st.sample_begin = 0xFFFFFFFEu);
    BAD("map_size outside 1 .. MPE_MAX_MAP", st.map_size = 0);
    BAD("map_size outside 1 .. MPE_MAX_MAP", st.map_size = MPE_MAX_MAP + 1);
    BAD("map_size outside 1 .. MPE_MAX_MAP", st.map_size = 0xFFFFFFFFu);
    BAD("pole above 2", st.pole = 3);
    BAD("pole above 2", st.pole = 0xFFFFFFFFu);
    BAD("unknown flag", st.flags = 2);
    BAD("unknown flag", st.flags = 0x80000001u);
#undef BAD
    // a caller's struct of exactly the published size on the heap: nothing beyond struct_size is read
    {
        const size_t published = offsetof(mpe_settings, pole) + sizeof(uint32_t);
        std::unique_ptr<unsigned char[]> raw(new unsigned char[published]);
        mpe_settings st = good;
        st.struct_size = uint32_t(published);
        std::memcpy(raw.get(), &st, published);
        EXPECT(published == 36 && mpe_check_settings(reinterpret_cast<const mpe_settings*>(raw.get())) == MP_OK);
    }

    // NULL pointers, a negative device, overlaps
    EXPECT(mpe_check_settings(nullptr) == MP_ERR_INVALID && g_last_error == "settings is NULL");
    EXPECT(resolve(nullptr, b) == MP_ERR_INVALID && g_last_error == "settings is NULL");
    EXPECT(resolve(&good, b, -1) == MP_ERR_INVALID && g_last_error == "negative device_id");
    for (int i = 0; i < 7; ++i) EXPECT(resolve(&good, b, DEV, i) == MP_ERR_INVALID && g_last_error == "NULL argument");
    EXPECT(resolve(&good, b, DEV, 7) == MP_ERR_HIP);  // out may be NULL: the call gets as far as the device, which does not exist
    EXPECT(resolve(&good, b) == MP_ERR_HIP);
    for (int i = 0; i < 6; ++i) {  // sums or out on the map, a ray array or the answers
        void* p[6] = {b.env.get(), b.ray[0].get(), b.ray[1].get(), b.ray[2].get(), b.ray[3].get(), b.occluded.get()};
        for (int o : {6, 7}) EXPECT(resolve(&good, b, DEV, -1, -1, 0, o, p[i]) == MP_ERR_INVALID && g_last_error == "an output overlaps another buffer of the call");
    }
    EXPECT(resolve(&good, b, DEV, -1, -1, 0, 7, b.sums.get()) == MP_ERR_INVALID);                    // out == sums
    EXPECT(resolve(&good, b, DEV, -1, -1, 0, 7, b.sums.get() + PLANE - 4) == MP_ERR_INVALID);        // out on the last pixel of sums
    EXPECT(resolve(&good, b, DEV, -1, -1, 0, 6, b.env.get() + MAP - 4) == MP_ERR_INVALID);           // sums on the last texel of the map
    EXPECT(resolve(&good, b, DEV, -1, -1, 0, 7, b.ray[3].get() + RAYS - 2) == MP_ERR_INVALID);       // out on the last words of tmax
    EXPECT(g_last_error == "an output overlaps another buffer of the call");

    // alignment, after the NULL and overlap checks: a plane or the map 4, 8 or 12 bytes off, a ray array 1, 2 or 3 bytes off (a
    // refused call reads and writes none of its buffers)
    for (void* p : {static_cast<void*>(b.env.get()), static_cast<void*>(b.sums.get()), static_cast<void*>(b.out.get())})
        EXPECT(reinterpret_cast<uintptr_t>(p) % 16 == 0);
    for (int by : {4, 8, 12})
        for (int at : {0, 6, 7}) EXPECT(resolve(&good, b, DEV, -1, at, by) == MP_ERR_INVALID && g_last_error == "a plane is not 16-byte aligned");
    for (int by : {1, 2, 3}) {
        for (int at : {1, 2, 3, 4}) EXPECT(resolve(&good, b, DEV, -1, at, by) == MP_ERR_INVALID && g_last_error == "a ray array is not 4-byte aligned");
        EXPECT(resolve(&good, b, DEV, -1, 5, by) == MP_ERR_HIP);  // occluded is bytes and has no rule (one byte fewer is read: never, here)
    }

    // mpe_fill_gradient: colours of exactly three floats on the heap
    {
        auto colour = [](float r, float g, float bl) {
            std::unique_ptr<float[]> c(new float[3]);
            c[0] = r; c[1] = g; c[2] = bl;
            return c;
        };
        auto z = colour(1, 2, 3), hz = colour(4, 5, 6), g = colour(7, 8, 9);
        float* env = b.env.get();
        EXPECT(mpe_fill_gradient(DEV, N, z.get(), hz.get(), g.get(), env, nullptr) == MP_ERR_HIP);
        EXPECT(mpe_fill_gradient(DEV, 0, z.get(), hz.get(), g.get(), env, nullptr) == MP_ERR_INVALID && g_last_error == "map_size outside 1 .. MPE_MAX_MAP");
        EXPECT(mpe_fill_gradient(DEV, MPE_MAX_MAP + 1, z.get(), hz.get(), g.get(), env, nullptr) == MP_ERR_INVALID);
        EXPECT(mpe_fill_gradient(-1, N, z.get(), hz.get(), g.get(), env, nullptr) == MP_ERR_INVALID && g_last_error == "negative device_id");
        EXPECT(mpe_fill_gradient(DEV, N, nullptr, hz.get(), g.get(), env, nullptr) == MP_ERR_INVALID && g_last_error == "NULL argument");
        EXPECT(mpe_fill_gradient(DEV, N, z.get(), nullptr, g.get(), env, nullptr) == MP_ERR_INVALID);
        EXPECT(mpe_fill_gradient(DEV, N, z.get(), hz.get(), nullptr, env, nullptr) == MP_ERR_INVALID);
        EXPECT(mpe_fill_gradient(DEV, N, z.get(), hz.get(), g.get(), nullptr, nullptr) == MP_ERR_INVALID);
        for (int by : {1, 2, 3}) EXPECT(mpe_fill_gradient(DEV, N, z.get(), hz.get(), g.get(), env + by, nullptr) == MP_ERR_INVALID && g_last_error == "a plane is not 16-byte aligned");
        for (int c = 0; c < 3; ++c)
            for (float v : {kNaN, kInf, -kInf}) {
                for (int which = 0; which < 3; ++which) {
                    auto bad = colour(1, 1, 1);
                    bad[c] = v;
                    const float* k[3] = {z.get(), hz.get(), g.get()};
                    k[which] = bad.get();
                    ++n_bad;
                    EXPECT(mpe_fill_gradient(DEV, N, k[0], k[1], k[2], env, nullptr) == MP_ERR_INVALID && g_last_error == "a gradient colour is not finite");
                }
            }
    }

    // nothing above launched anything or wrote a word
    size_t need = 99;
    EXPECT(mpe_last_kernels(nullptr, 0, &need) == MP_OK && need == 0);
    EXPECT(mpe_last_kernels(nullptr, 4, nullptr) == MP_ERR_INVALID && g_last_error == "NULL argument");
    for (size_t i = 0; i < PLANE; ++i) EXPECT(b.sums[i] == 0.0f && b.out[i] == 0.0f);
    for (size_t i = 0; i < MAP; ++i) EXPECT(b.env[i] == 0.0f);
    std::printf("sky_abi_check: ok (%d refusals of settings and colours)\n", n_bad);
    return 0;
}
