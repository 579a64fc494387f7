// Host check of minipath_amd/post/post_abi.h, a program of its own (nothing of it is loaded into Python; it opens no GPU):
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/post_abi_check.hip -o post_abi_check
//   ./post_abi_check            prints "post_abi_check: ok" and exits 0, or names the first line that does not hold
// It throws through guarded(), fills and reads the kernel record, and runs the overlap check on adjacent, nested, partly
// overlapping and NULL spans.  launch() and DeviceScope need a device and are left to the GPU tests.
#include <cstdio>
#include <stdexcept>

#include "../include/minipath_denoise.h"
#include "../minipath_amd/post/post_abi.h"

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
    std::printf("post_abi_check: ok\n");
    return 0;
}
