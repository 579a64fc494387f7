// Host check of minipath_amd/post/post_abi.h, a program of its own (nothing of it is loaded into Python; it opens no GPU):
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined tools/post_abi_check.hip -o post_abi_check
//   ./post_abi_check            prints "post_abi_check: ok" and exits 0, or names the first line that does not hold
// It throws through guarded(), fills and reads the kernel record, runs the overlap check on adjacent, nested, partly
// overlapping and NULL spans and the alignment check on every offset of a 16-byte block and at the top of the address space, and
// walks the alignment refusals of one library built on it: the unit of libminipath_denoise.so is compiled into this program
// (tools/lights_abi_check.hip does the same for the lights).  launch() and DeviceScope need a device and are left to the GPU tests.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "../minipath_amd/denoise/atrous.hip"

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("post_abi_check: line %d: %s\n", __LINE__, #cond); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static std::string record() {
    size_t need = 99;
    if (copy_last_kernels(nullptr, 0, &need) != MP_OK) return "?";
    std::string s(need + 1, '\xff');
    if (copy_last_kernels(&s[0], need + 1, nullptr) != MP_OK) return "?";
    s.resize(need);
    return s;
}

int main() {
    // guarded: the three catches, and a body's own status
    EXPECT(guarded([]() -> int { throw std::bad_alloc(); }) == MP_ERR_NOMEM);
    EXPECT(g_last_error == "out of host memory (std::bad_alloc)");
    EXPECT(guarded([]() -> int { throw std::runtime_error("boom"); }) == MP_ERR_INVALID);
    EXPECT(g_last_error == "unexpected exception: boom");
    EXPECT(guarded([]() -> int { throw 7; }) == MP_ERR_INVALID);
    EXPECT(g_last_error == "unexpected exception");
    EXPECT(guarded([]() -> int { return fail(MP_ERR_UNSUPPORTED, "why"); }) == MP_ERR_UNSUPPORTED && g_last_error == "why");
    EXPECT(guarded([]() -> int { return MP_OK; }) == MP_OK && g_last_error == "why");  // success leaves the message

    // the kernel record: empty at first; distinct names in launch order; a call that launched nothing leaves it
    EXPECT(record().empty());
    { LaunchLog log; }
    EXPECT(record().empty());
    {
        LaunchLog log;
        log.note("a_kernel<true>");
        log.note("b_kernel");
        const char again[] = "a_kernel<true>";  // the same name at another address
        log.note(again);
        EXPECT(record().empty());  // the record is the call's when it returns
    }
    EXPECT(record() == "a_kernel<true>\nb_kernel");
    { LaunchLog log; }
    EXPECT(record() == "a_kernel<true>\nb_kernel");
    {
        LaunchLog log;
        log.note("c_kernel");
    }
    EXPECT(record() == "c_kernel");

    // copy_last_kernels: the size alone; a NULL buffer with room asked for; the terminating 0 alone; a short buffer
    size_t need = 0;
    EXPECT(copy_last_kernels(nullptr, 0, &need) == MP_OK && need == 8);
    EXPECT(copy_last_kernels(nullptr, 4, nullptr) == MP_ERR_INVALID && g_last_error == "NULL argument");
    char buf[16];
    std::memset(buf, 0x7f, sizeof buf);
    EXPECT(copy_last_kernels(buf, 1, nullptr) == MP_OK && buf[0] == 0 && buf[1] == 0x7f);
    EXPECT(copy_last_kernels(buf, 4, &need) == MP_OK && std::strcmp(buf, "c_k") == 0 && buf[4] == 0x7f && need == 8);
    EXPECT(copy_last_kernels(buf, 9, nullptr) == MP_OK && std::strcmp(buf, "c_kernel") == 0 && buf[9] == 0x7f);

    // outputs_overlap: the first n_outs spans against every later one
    alignas(16) static char m[256];
    {
        const Span adjacent[] = {{m, 64}, {m + 64, 64}, {m + 128, 128}};
        EXPECT(!outputs_overlap(adjacent, 3, 1) && !outputs_overlap(adjacent, 3, 3));
        const Span nested[] = {{m, 128}, {m + 32, 16}};
        const Span nested_rev[] = {{m + 32, 16}, {m, 128}};
        EXPECT(outputs_overlap(nested, 2, 1) && outputs_overlap(nested_rev, 2, 1));
        const Span partial[] = {{m + 32, 64}, {m, 33}};
        const Span touching[] = {{m + 32, 64}, {m, 32}};
        EXPECT(outputs_overlap(partial, 2, 1) && !outputs_overlap(touching, 2, 1));
        const Span last_byte[] = {{m, 64}, {m + 63, 1}};
        EXPECT(outputs_overlap(last_byte, 2, 1));
        const Span same[] = {{m, 16}, {m, 16}};
        EXPECT(outputs_overlap(same, 2, 1));
        // two inputs may share bytes: only outputs are compared
        const Span inputs[] = {{m, 16}, {m + 64, 32}, {m + 64, 32}};
        EXPECT(!outputs_overlap(inputs, 3, 1) && outputs_overlap(inputs, 3, 2));
        // NULL spans are absent, as an output and as an input, whatever their size
        const Span null_out[] = {{nullptr, 256}, {m, 64}, {m + 64, 64}};
        EXPECT(!outputs_overlap(null_out, 3, 2));
        const Span null_in[] = {{m, 64}, {nullptr, ~size_t(0)}, {m + 32, 8}};
        EXPECT(!outputs_overlap(null_in, 2, 1) && outputs_overlap(null_in, 3, 1));
        EXPECT(!outputs_overlap(null_in, 0, 0));
    }

    // all_aligned: every pointer of the list against the alignment; NULL pointers are absent; an empty list is aligned
    {
        EXPECT(all_aligned({}, kPlaneAlign) && all_aligned({nullptr}, kPlaneAlign) && all_aligned({m, m + 16, m + 240}, kPlaneAlign));
        for (int off = 1; off < 16; ++off) {
            EXPECT(!all_aligned({m + off}, kPlaneAlign));
            // the misaligned pointer is found wherever it stands in the list
            EXPECT(!all_aligned({m + off, m, nullptr}, kPlaneAlign) && !all_aligned({m, m + off, nullptr}, kPlaneAlign));
            EXPECT(!all_aligned({nullptr, m, m + 32 + off}, kPlaneAlign));
            EXPECT(all_aligned({m + off}, kWordAlign) == (off % 4 == 0));
            EXPECT(all_aligned({m, nullptr, m + off}, kWordAlign) == (off % 4 == 0));
        }
        EXPECT(all_aligned({m + 1, m + 2, m + 3}, 1));  // bytes (an `occluded` array) have no rule
        // the top of the address space: no arithmetic on the pointer overflows
        const void* top = reinterpret_cast<const void*>(~uintptr_t(0));
        const void* top16 = reinterpret_cast<const void*>(~uintptr_t(15));
        EXPECT(!all_aligned({top}, kPlaneAlign) && !all_aligned({top}, kWordAlign) && all_aligned({top16}, kPlaneAlign));
        // a refusal as the libraries make it: status, message, and the kernel record left alone
        const std::string before = record();
        EXPECT(guarded([&]() -> int {
                   if (!all_aligned({m, m + 4}, kPlaneAlign)) return fail(MP_ERR_INVALID, "a plane is not 16-byte aligned");
                   return MP_OK;
               }) == MP_ERR_INVALID);
        EXPECT(g_last_error == "a plane is not 16-byte aligned" && record() == before);
    }

    // the refusals built on it, through mpd_atrous and mpd_variance_from_moments: every plane argument 4, 8 and 12 bytes off, with
    // nothing else wrong, on heap buffers of exactly the sizes the calls state (a refused call reads and writes none of them)
    {
        constexpr uint32_t W = 6, H = 5;
        constexpr size_t PLANE = size_t(W) * H * 16;  // bytes
        const size_t sizes[7] = {PLANE, PLANE, PLANE, PLANE, 4 * PLANE, PLANE, PLANE};  // color, normal_depth, albedo, variance, scratch, out, variance_out
        float* p[7];
        for (int i = 0; i < 7; ++i) {
            p[i] = static_cast<float*>(std::aligned_alloc(16, sizes[i]));
            EXPECT(p[i] && reinterpret_cast<uintptr_t>(p[i]) % 16 == 0);
        }
        mpd_settings st{};
        st.struct_size = sizeof st;
        st.width = W; st.height = H; st.iterations = 3;
        st.sigma_normal_pow2 = 7.0f; st.sigma_depth = 0.5f; st.sigma_luminance = 1.0f;
        st.flags = MPD_FLAG_DEMODULATE_ALBEDO;
        EXPECT(mpd_scratch_floats(&st, 1) * 4 == sizes[4]);
        const int no_device = 1 << 20;
        const std::string before = record();
        for (int at = 0; at < 7; ++at)
            for (int by : {4, 8, 12}) {
                float* q[7];
                for (int i = 0; i < 7; ++i) q[i] = i == at ? reinterpret_cast<float*>(reinterpret_cast<char*>(p[i]) + by) : p[i];
                EXPECT(mpd_atrous(no_device, &st, q[0], q[1], q[2], q[3], q[4], q[5], q[6], nullptr) == MP_ERR_INVALID);
                EXPECT(g_last_error == "a plane is not 16-byte aligned");
            }
        for (int at = 0; at < 3; ++at)
            for (int by : {4, 8, 12}) {
                float* q[3];
                for (int i = 0; i < 3; ++i) q[i] = i == at ? reinterpret_cast<float*>(reinterpret_cast<char*>(p[i]) + by) : p[i];
                EXPECT(mpd_variance_from_moments(no_device, W, H, 8, q[0], q[1], q[2], nullptr) == MP_ERR_INVALID);
                EXPECT(g_last_error == "a plane is not 16-byte aligned");
            }
        // the earlier refusals keep their messages when a plane is misaligned too
        EXPECT(mpd_atrous(no_device, &st, p[0] + 1, p[1], p[2], p[3], p[4], p[0] + 1, p[6], nullptr) == MP_ERR_INVALID);
        EXPECT(g_last_error == "an output aliases another argument");
        EXPECT(mpd_variance_from_moments(no_device, W, H, 8, p[0] + 1, nullptr, p[2], nullptr) == MP_ERR_INVALID && g_last_error == "NULL argument");
        EXPECT(record() == before);
        for (float* q : p) std::free(q);
    }
    std::printf("post_abi_check: ok\n");
    return 0;
}
