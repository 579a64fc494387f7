// Move-only owners of the HIP resources the host code holds: a device buffer, a pinned host buffer, a stream and an event.
// Each remembers the device it was made on; its destructor switches to that device and back.  No other host unit frees or
// destroys a HIP resource.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace mp {

// Makes `dev` the current device of the calling thread for its lifetime.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// What the four owners share: one handle made on the current device, given back on that device by Traits::release.
template <class T, class Traits>
class Owned {
public:
    Owned() = default;
    Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, T{})), device_(o.device_), bytes_(std::exchange(o.bytes_, 0)) {}
    Owned& operator=(Owned&& o) noexcept {  // (what this one held goes with `o`)
        std::swap(h_, o.h_);
        std::swap(device_, o.device_);
        std::swap(bytes_, o.bytes_);
        return *this;
    }
    ~Owned() { reset(); }
    void reset() {  // (hipFree waits for the device: the caller waits first where the order matters)
        if (!h_) return;
        DeviceGuard g(device_);
        Traits::release(h_);
        h_ = T{};
        bytes_ = 0;
    }
    T get() const { return h_; }

protected:
    hipError_t adopt(hipError_t e, size_t bytes) {
        if (e != hipSuccess) h_ = T{};
        bytes_ = h_ ? bytes : 0;
        if (hipGetDevice(&device_) != hipSuccess) device_ = 0;
        return e;
    }
    T h_{};
    int device_ = 0;
    size_t bytes_ = 0;
};

struct DeviceFree { static void release(void* p) { (void)hipFree(p); } };
struct PinnedFree { static void release(void* p) { (void)hipHostFree(p); } };
struct StreamFree { static void release(hipStream_t s) { (void)hipStreamDestroy(s); } };
struct EventFree { static void release(hipEvent_t e) { (void)hipEventDestroy(e); } };

// Device and pinned buffers know their capacity.  grow(): nothing if the buffer is large enough already; otherwise it frees
// before it allocates, and an allocation that fails leaves an empty buffer of capacity 0.
template <class Traits>
class Buffer : public Owned<void*, Traits> {
public:
    size_t bytes() const { return this->bytes_; }
    template <class U> U* as() const { return static_cast<U*>(this->h_); }
    hipError_t grow(size_t bytes) {
        if (this->h_ && this->bytes_ >= bytes) return hipSuccess;
        this->reset();
        return this->adopt(alloc(&this->h_, bytes, Traits{}), bytes);
    }

private:
    static hipError_t alloc(void** p, size_t n, DeviceFree) { return hipMalloc(p, n); }
    static hipError_t alloc(void** p, size_t n, PinnedFree) { return hipHostMalloc(p, n, hipHostMallocDefault); }
};
using DeviceBuffer = Buffer<DeviceFree>;
using PinnedBuffer = Buffer<PinnedFree>;

struct Stream : Owned<hipStream_t, StreamFree> {
    hipError_t ensure() { return h_ ? hipSuccess : adopt(hipStreamCreateWithFlags(&h_, hipStreamNonBlocking), 0); }
    void sync() const { if (h_) (void)hipStreamSynchronize(h_); }
};
struct Event : Owned<hipEvent_t, EventFree> {
    hipError_t ensure() { return h_ ? hipSuccess : adopt(hipEventCreateWithFlags(&h_, hipEventDisableTiming), 0); }
};

}  // namespace mp
