// Host check of the argument checking of libminipath_lights.so, a program of its own (nothing of it is loaded into Python; it makes
// no HIP call and opens no GPU): the library's unit is compiled into this program and every refusal of include/minipath_lights.h is
// walked under the sanitizers, with buffers of exactly the sizes the calls state, so a read beyond a table of light_count lights or
// beyond a settings struct of struct_size bytes would be reported.
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined tools/lights_abi_check.hip -o lights_abi_check
//   ./lights_abi_check          prints "lights_abi_check: ok" and exits 0, or names the first line that does not hold
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>

#include "../minipath_amd/lights/lights.hip"

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("lights_abi_check: line %d: %s\n", __LINE__, #cond); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

namespace {

constexpr uint32_t W = 6, H = 5, B = 3, L = 2;
constexpr size_t PLANE = size_t(W) * H * 4, RAYS = size_t(W) * H * B * L;  // floats
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

mpl_settings good_settings() {
    mpl_settings st{};
    st.struct_size = sizeof(mpl_settings);
    st.width = W; st.height = H; st.sample_count = 8; st.sample_begin = 2; st.batch = B; st.light_count = L; st.seed = 1;
    st.eye[2] = 5.0f; st.bias = 1e-4f; st.margin = 0.0f;
    return st;
}

// a table of exactly n lights on the heap: the sanitizer sees a read of light n
std::unique_ptr<mpl_light[]> good_lights(uint32_t n = L) {
    std::unique_ptr<mpl_light[]> t(new mpl_light[n]());
    for (uint32_t i = 0; i < n; ++i) {
        t[i].position[0] = float(i); t[i].position[1] = 1.0f; t[i].position[2] = 2.0f;
        t[i].radius = (i & 1) ? 0.25f : 0.0f;
        t[i].intensity[0] = 1.0f; t[i].intensity[1] = 0.0f; t[i].intensity[2] = 2.0f;
    }
    return t;
}

struct Buffers {
    std::unique_ptr<float[]> position{new float[PLANE]()}, normal{new float[PLANE]()}, sums{new float[PLANE]()}, out{new float[PLANE]()};
    std::unique_ptr<float[]> ray[8];
    std::unique_ptr<uint8_t[]> occluded{new uint8_t[RAYS]()};
    Buffers() {
        for (auto& r : ray) r.reset(new float[RAYS]());
    }
};

// never a real device: a call accepted by mistake would be refused by the runtime, not launched
constexpr int DEV = 1 << 20;

int generate(const mpl_settings* st, const mpl_light* lt, Buffers& b, int dev = DEV, int null_at = -1, float* ox = nullptr) {
    float* p[10] = {b.position.get(), b.normal.get(), b.ray[0].get(), b.ray[1].get(), b.ray[2].get(), b.ray[3].get(), b.ray[4].get(),
                    b.ray[5].get(), b.ray[6].get(), b.ray[7].get()};
    if (ox) p[2] = ox;
    if (null_at >= 0) p[null_at] = nullptr;
    return mpl_generate(dev, st, lt, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], nullptr);
}

int resolve(const mpl_settings* st, const mpl_light* lt, Buffers& b, int dev = DEV, int null_at = -1, float* out = nullptr) {
    void* p[4] = {b.ray[6].get(), b.ray[7].get(), b.occluded.get(), b.sums.get()};
    if (null_at >= 0) p[null_at] = nullptr;
    return mpl_resolve(dev, st, lt, static_cast<float*>(p[0]), static_cast<float*>(p[1]), static_cast<uint8_t*>(p[2]), static_cast<float*>(p[3]),
                       out ? out : b.out.get(), nullptr);
}

// the calls with nothing wrong but buffer `at` (in the order of the arguments) moved by `by` bytes
char* moved(void* p, int by) { return static_cast<char*>(p) + by; }
int generate_moved(const mpl_settings* st, const mpl_light* lt, Buffers& b, int at, int by) {
    void* p[10] = {b.position.get(), b.normal.get(), b.ray[0].get(), b.ray[1].get(), b.ray[2].get(), b.ray[3].get(), b.ray[4].get(),
                   b.ray[5].get(), b.ray[6].get(), b.ray[7].get()};
    p[at] = moved(p[at], by);
    float* f[10];
    for (int i = 0; i < 10; ++i) f[i] = static_cast<float*>(p[i]);
    return mpl_generate(DEV, st, lt, f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], f[9], nullptr);
}
int resolve_moved(const mpl_settings* st, const mpl_light* lt, Buffers& b, int at, int by) {
    void* p[5] = {b.ray[6].get(), b.ray[7].get(), b.occluded.get(), b.sums.get(), b.out.get()};
    p[at] = moved(p[at], by);
    return mpl_resolve(DEV, st, lt, static_cast<float*>(p[0]), static_cast<float*>(p[1]), static_cast<uint8_t*>(p[2]), static_cast<float*>(p[3]),
                       static_cast<float*>(p[4]), nullptr);
}

}  // namespace

int main() {
    Buffers b;
    auto lights = good_lights();
    const mpl_settings good = good_settings();
    EXPECT(mpl_settings_size() == 64 && sizeof(mpl_light) == 32);
    EXPECT(mpl_check_settings(&good, lights.get()) == MP_OK);

    // every refusal by the settings alone, through all three entry points
    int n_bad = 0;
    auto refused = [&](mpl_settings st, const char* why) -> bool {
        ++n_bad;
        auto table = good_lights(st.light_count >= 1 && st.light_count <= MPL_MAX_LIGHTS ? st.light_count : L);
        return mpl_check_settings(&st, table.get()) == MP_ERR_INVALID && g_last_error == why && generate(&st, table.get(), b) == MP_ERR_INVALID &&
               g_last_error == why && resolve(&st, table.get(), b) == MP_ERR_INVALID && g_last_error == why;
    };
#define BAD(why, ...)                \
    do {                             \
        mpl_settings st = good;      \
        __VA_ARGS__;                 \
        EXPECT(refused(st, why));    \
    } while (0)
    BAD("bad struct_size", st.struct_size = 0);
    BAD("bad struct_size", st.struct_size = 59);
    BAD("width * height == 0", st.width = 0);
    BAD("width * height == 0", st.height = 0);
    BAD("width or height above MPL_MAX_DIM", st.width = MPL_MAX_DIM + 1);
    BAD("width or height above MPL_MAX_DIM", st.height = 0xFFFFFFFFu);
    BAD("batch == 0", st.batch = 0);
    BAD("light_count outside 1 .. MPL_MAX_LIGHTS", st.light_count = 0);
    BAD("light_count outside 1 .. MPL_MAX_LIGHTS", st.light_count = 9);
    BAD("light_count outside 1 .. MPL_MAX_LIGHTS", st.light_count = 0xFFFFFFFFu);
    BAD("width * height * batch * light_count >= 2^31", st.width = 1u << 20; st.height = 1u << 20);
    BAD("width * height * batch * light_count >= 2^31", st.width = 1u << 16; st.height = 1u << 15; st.batch = 1; st.light_count = 1);
    BAD("width * height * batch * light_count >= 2^31", st.width = 1u << 10; st.height = 1u << 10; st.batch = 0xFFFFFFFFu);
    BAD("width * height * batch * light_count >= 2^31", st.width = 1u << 10; st.height = 1u << 10; st.batch = 256; st.sample_count = 65536;
        st.light_count = 8);
    BAD("sample_count outside 1 .. MPL_MAX_SAMPLES", st.sample_count = 0; st.sample_begin = 0);
    BAD("sample_count outside 1 .. MPL_MAX_SAMPLES", st.sample_count = MPL_MAX_SAMPLES + 1);
    BAD("sample_begin + batch > sample_count", st.sample_begin = 6);
    BAD("sample_begin + batch > sample_count", st.sample_begin = 0xFFFFFFFEu);
    BAD("unknown flag", st.flags = 2);
    BAD("unknown flag", st.flags = 0x80000001u);
    BAD("eye is not finite", st.eye[0] = kNaN);
    BAD("eye is not finite", st.eye[1] = kInf);
    BAD("eye is not finite", st.eye[2] = -kInf);
    BAD("bias is not finite and >= 0", st.bias = -1e-4f);
    BAD("bias is not finite and >= 0", st.bias = kNaN);
    BAD("bias is not finite and >= 0", st.bias = kInf);
    BAD("margin is not finite and >= 0", st.margin = -0.1f);
    BAD("margin is not finite and >= 0", st.margin = kNaN);
    BAD("margin is not finite and >= 0", st.margin = kInf);
#undef BAD

    // every refusal by the light table, in the first and in the last light
    auto bad_light = [&](uint32_t i, void (*spoil)(mpl_light&), const char* why) -> bool {
        ++n_bad;
        auto table = good_lights();
        spoil(table[i]);
        return mpl_check_settings(&good, table.get()) == MP_ERR_INVALID && g_last_error == why && generate(&good, table.get(), b) == MP_ERR_INVALID &&
               g_last_error == why && resolve(&good, table.get(), b) == MP_ERR_INVALID && g_last_error == why;
    };
    for (uint32_t i = 0; i < L; ++i) {
        EXPECT(bad_light(i, [](mpl_light& t) { t.position[0] = std::numeric_limits<float>::quiet_NaN(); }, "a light's position is not finite"));
        EXPECT(bad_light(i, [](mpl_light& t) { t.position[2] = -std::numeric_limits<float>::infinity(); }, "a light's position is not finite"));
        EXPECT(bad_light(i, [](mpl_light& t) { t.intensity[1] = -1.0f; }, "a light's intensity is not finite and >= 0"));
        EXPECT(bad_light(i, [](mpl_light& t) { t.intensity[2] = std::numeric_limits<float>::infinity(); }, "a light's intensity is not finite and >= 0"));
        EXPECT(bad_light(i, [](mpl_light& t) { t.intensity[0] = std::numeric_limits<float>::quiet_NaN(); }, "a light's intensity is not finite and >= 0"));
        EXPECT(bad_light(i, [](mpl_light& t) { t.radius = -0.5f; }, "a light's radius is not finite and >= 0"));
        EXPECT(bad_light(i, [](mpl_light& t) { t.radius = std::numeric_limits<float>::infinity(); }, "a light's radius is not finite and >= 0"));
        EXPECT(bad_light(i, [](mpl_light& t) { t.radius = std::numeric_limits<float>::quiet_NaN(); }, "a light's radius is not finite and >= 0"));
        EXPECT(bad_light(i, [](mpl_light& t) { t.reserved = 1.0f; }, "a light's reserved is not 0"));
        EXPECT(bad_light(i, [](mpl_light& t) { t.reserved = std::numeric_limits<float>::quiet_NaN(); }, "a light's reserved is not 0"));
    }
    // one light of a table of one: nothing beyond it is read
    {
        mpl_settings st = good;
        st.light_count = 1;
        auto one = good_lights(1);
        EXPECT(mpl_check_settings(&st, one.get()) == MP_OK);
    }
    // a caller's struct of exactly the published size on the heap: nothing beyond struct_size is read
    {
        const size_t published = offsetof(mpl_settings, margin) + sizeof(float);
        std::unique_ptr<unsigned char[]> raw(new unsigned char[published]);
        mpl_settings st = good;
        st.struct_size = uint32_t(published);
        std::memcpy(raw.get(), &st, published);
        EXPECT(published == 60 && mpl_check_settings(reinterpret_cast<const mpl_settings*>(raw.get()), lights.get()) == MP_OK);
    }

    // NULL pointers, a negative device, overlaps
    EXPECT(mpl_check_settings(nullptr, lights.get()) == MP_ERR_INVALID && g_last_error == "settings is NULL");
    EXPECT(mpl_check_settings(&good, nullptr) == MP_ERR_INVALID && g_last_error == "lights is NULL");
    EXPECT(generate(nullptr, lights.get(), b) == MP_ERR_INVALID && resolve(nullptr, lights.get(), b) == MP_ERR_INVALID);
    EXPECT(generate(&good, nullptr, b) == MP_ERR_INVALID && resolve(&good, nullptr, b) == MP_ERR_INVALID);
    EXPECT(generate(&good, lights.get(), b, -1) == MP_ERR_INVALID && g_last_error == "negative device_id");
    EXPECT(resolve(&good, lights.get(), b, -1) == MP_ERR_INVALID && g_last_error == "negative device_id");
    for (int i = 0; i < 10; ++i) EXPECT(generate(&good, lights.get(), b, DEV, i) == MP_ERR_INVALID && g_last_error == "NULL argument");
    for (int i = 0; i < 4; ++i) EXPECT(resolve(&good, lights.get(), b, DEV, i) == MP_ERR_INVALID && g_last_error == "NULL argument");
    EXPECT(generate(&good, lights.get(), b, DEV, -1, b.ray[3].get()) == MP_ERR_INVALID);                // ox == dx
    EXPECT(generate(&good, lights.get(), b, DEV, -1, b.ray[7].get() + RAYS - 1) == MP_ERR_INVALID);     // ox on weight's last word
    EXPECT(generate(&good, lights.get(), b, DEV, -1, b.position.get() + 4) == MP_ERR_INVALID);          // ox inside a plane
    EXPECT(g_last_error == "a ray array overlaps another buffer of the call");
    EXPECT(resolve(&good, lights.get(), b, DEV, -1, b.sums.get()) == MP_ERR_INVALID);                   // out == sums
    EXPECT(resolve(&good, lights.get(), b, DEV, -1, b.ray[7].get() + 8) == MP_ERR_INVALID);             // out inside weight
    EXPECT(g_last_error == "an output overlaps another buffer of the call");

    // alignment, after the NULL and overlap checks: a plane 4, 8 or 12 bytes off, a ray array 1, 2 or 3 bytes off (a refused
    // call reads and writes none of its buffers)
    for (void* p : {static_cast<void*>(b.position.get()), static_cast<void*>(b.normal.get()), static_cast<void*>(b.sums.get()), static_cast<void*>(b.out.get())})
        EXPECT(reinterpret_cast<uintptr_t>(p) % 16 == 0);
    for (int by : {4, 8, 12}) {
        for (int at : {0, 1}) EXPECT(generate_moved(&good, lights.get(), b, at, by) == MP_ERR_INVALID && g_last_error == "a plane is not 16-byte aligned");
        for (int at : {3, 4}) EXPECT(resolve_moved(&good, lights.get(), b, at, by) == MP_ERR_INVALID && g_last_error == "a plane is not 16-byte aligned");
    }
    for (int by : {1, 2, 3}) {
        for (int at = 2; at < 10; ++at)
            EXPECT(generate_moved(&good, lights.get(), b, at, by) == MP_ERR_INVALID && g_last_error == "a ray array is not 4-byte aligned");
        for (int at : {0, 1}) EXPECT(resolve_moved(&good, lights.get(), b, at, by) == MP_ERR_INVALID && g_last_error == "a ray array is not 4-byte aligned");
    }

    // nothing above launched anything or wrote a word
    size_t need = 99;
    EXPECT(mpl_last_kernels(nullptr, 0, &need) == MP_OK && need == 0);
    EXPECT(mpl_last_kernels(nullptr, 4, nullptr) == MP_ERR_INVALID && g_last_error == "NULL argument");
    for (auto& r : b.ray)
        for (size_t i = 0; i < RAYS; ++i) EXPECT(r[i] == 0.0f);
    for (size_t i = 0; i < PLANE; ++i) EXPECT(b.sums[i] == 0.0f && b.out[i] == 0.0f);
    std::printf("lights_abi_check: ok (%d refusals of settings and lights, each through three entry points)\n", n_bad);
    return 0;
}
