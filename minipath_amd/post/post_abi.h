// The host side each of the seven post-process libraries (denoise, adaptive, temporal, secondary, resample, lights, sky) puts
// between its C ABI and its kernels: the last-error and last-kernels records, the catch-all of an extern "C" body, the device scope, the launch and the
// overlap and alignment checks of a call's buffers.  Include it after the library's own header under include/ (the MP_* status values).
// Everything here has internal linkage: each shared object that includes this keeps thread-local records of its own, and two
// libraries loaded into one process share nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

namespace {

thread_local std::string g_last_error;
thread_local std::string g_last_kernels;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
int hip_fail(hipError_t e, const std::string& what) { return fail(MP_ERR_HIP, what + ": " + hipGetErrorString(e)); }

// No exception crosses the C ABI: every extern "C" body runs inside guarded().
template <class F>
int guarded(F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        try { g_last_error = "out of host memory (std::bad_alloc)"; } catch (...) {}
        return MP_ERR_NOMEM;
    } catch (const std::exception& ex) {
        try { g_last_error = std::string("unexpected exception: ") + ex.what(); } catch (...) {}
        return MP_ERR_INVALID;
    } catch (...) {
        try { g_last_error = "unexpected exception"; } catch (...) {}
        return MP_ERR_INVALID;
    }
}

// The body of mpX_last_kernels (called inside guarded()).
int copy_last_kernels(char* buf, size_t cap, size_t* needed) {
    if (cap && !buf) return fail(MP_ERR_INVALID, "NULL argument");
    if (needed) *needed = g_last_kernels.size();
    if (cap) {
        const size_t n = std::min(cap - 1, g_last_kernels.size());
        std::memcpy(buf, g_last_kernels.data(), n);
        buf[n] = 0;
    }
    return MP_OK;
}

// The record of mpX_last_kernels: a call notes each kernel before it launches it, distinct names in launch order, and the record
// is theirs, joined by '\n', when the call returns.  A call that launched nothing leaves the record as it was.
struct LaunchLog {
    std::vector<const char*> names;
    void note(const char* n) {
        for (const char* m : names)
            if (std::strcmp(m, n) == 0) return;
        names.push_back(n);
    }
    ~LaunchLog() {
        if (names.empty()) return;
        try {
            std::string t;
            for (const char* n : names) {
                if (!t.empty()) t += '\n';
                t += n;
            }
            g_last_kernels.swap(t);
        } catch (...) {}
    }
};

// One launch: `name` ("kernel" or "kernel<args>") goes into the log, and a failure reads "kernel launch: <HIP's text>".  HIP's
// last-error state is per thread and sticky: an error that earlier work of the process left there (any library, any call whose
// status nobody read) is not this launch's, so it is cleared first and what hipGetLastError() says after the launch is the
// launch's own.
template <class... Params, class... Args>
int launch(LaunchLog& log, const char* name, void (*kernel)(Params...), dim3 grid, dim3 block, void* stream, Args&&... args) {
    log.note(name);
    (void)hipGetLastError();
    hipLaunchKernelGGL(kernel, grid, block, 0, static_cast<hipStream_t>(stream), static_cast<Args&&>(args)...);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return hip_fail(e, std::string(name, std::strcspn(name, "<")) + " launch");
    return MP_OK;
}

// The calling thread's device is put back when the call returns.
struct DeviceScope {
    int prev = -1;
    hipError_t enter(int device) {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess) { prev = -1; return e; }
        return hipSetDevice(device);
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

struct Span {
    const void* p;
    size_t bytes;
};
// Does one of the first n_outs buffers share a byte with another buffer of the list?  NULL buffers are absent.
bool outputs_overlap(const Span* s, size_t n, size_t n_outs) {
    for (size_t o = 0; o < n_outs; ++o) {
        if (!s[o].p) continue;
        const uintptr_t ob = reinterpret_cast<uintptr_t>(s[o].p);
        for (size_t i = o + 1; i < n; ++i) {
            if (!s[i].p) continue;
            const uintptr_t ib = reinterpret_cast<uintptr_t>(s[i].p);
            if (ob < ib ? ib - ob < s[o].bytes : ob - ib < s[i].bytes) return true;
        }
    }
    return false;
}

// The alignment a header states is refused where it is missing, not left to the device: a plane is read and written as 16-byte
// pixels (kPlaneAlign), a ray array or a pick array as 32-bit words (kWordAlign).  Is every pointer of the list a multiple of
// `align` (a power of two)?  NULL pointers are absent.
constexpr uintptr_t kPlaneAlign = 16, kWordAlign = 4;
bool all_aligned(std::initializer_list<const void*> ptrs, uintptr_t align) {
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & (align - 1)) return false;
    return true;
}

}  // namespace
