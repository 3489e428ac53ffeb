// y2_mem.hpp -- who owns device and pinned memory in libyolo2_hip.so: two move-only handles.  A buffer is freed when its owner goes
// out of scope, is reset or is assigned to; everything else (kernel arguments, launch tables, a lane's weights) is a plain T* view
// that frees nothing.  Not for static storage: a destructor that runs at process exit may find the HIP runtime gone.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>

#include "../../include/yolo2_hip.h"

int y2_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));   // yolo2_hip.hip (y2_internal.hpp)

// live bytes held by owners, [0] device, [1] pinned (yolo2_hip_debug_live_bytes); nothing on a launch path allocates
extern std::atomic<size_t> y2_live_bytes[2];

template <typename T, bool kPinned>
class Y2Owner {
public:
    Y2Owner() = default;
    Y2Owner(const Y2Owner &) = delete;
    Y2Owner &operator=(const Y2Owner &) = delete;
    Y2Owner(Y2Owner &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    Y2Owner &operator=(Y2Owner &&o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~Y2Owner() { reset(); }
    // frees what it holds, then allocates `count` elements (0: stays empty); on failure it is empty and the error is set
    int alloc(size_t count, const char *file = __builtin_FILE(), int line = __builtin_LINE())
    {
        reset();
        if (!count) return YOLO2_SUCCESS;
        const size_t bytes = count * sizeof(T);
        const hipError_t e = kPinned ? hipHostMalloc((void **)&p_, bytes, hipHostMallocDefault) : hipMalloc((void **)&p_, bytes);
        if (e != hipSuccess) {
            p_ = nullptr;
            return y2_fail(YOLO2_MMAP_ERROR, "%s(%zu bytes) failed: %s (%s:%d)", kPinned ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e), file, line);
        }
        bytes_ = bytes;
        y2_live_bytes[kPinned] += bytes;
        return YOLO2_SUCCESS;
    }
    void reset()
    {
        if (!p_) return;
        (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
        y2_live_bytes[kPinned] -= bytes_;
        p_ = nullptr;
        bytes_ = 0;
    }
    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    T *p_ = nullptr;
    size_t bytes_ = 0;
};
template <typename T> using Y2DevBuf = Y2Owner<T, false>;   // hipMalloc
template <typename T> using Y2PinBuf = Y2Owner<T, true>;    // hipHostMalloc
