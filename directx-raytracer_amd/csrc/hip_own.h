// Ownership of HIP resources for the host side of the geometry code (bvh_gpu.hip, bvh_ploc.hip, refit_kernels.hip and what
// the C-ABI layer takes over from them): one way to turn a hipError_t into an exception, one buffer in HBM that frees itself, one
// pair of timing events.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <stdexcept>
#include <string>

#define HIP_THROW(expr)                                                                                        \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) throw std::runtime_error(std::string(#expr " failed: ") + hipGetErrorString(e_)); \
    } while (0)

namespace crt {

// hipMalloc'ed memory, freed with its owner unless release() handed it on; move-only.  An empty buffer holds NULL.
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    explicit DeviceBuffer(size_t bytes) { HIP_THROW(hipMalloc(&p_, bytes ? bytes : 16)); } // (never NULL: "no bytes" is still a buffer)
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.release()) {}
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept
    {
        if (this != &o) {
            if (p_) (void)hipFree(p_);
            p_ = o.release();
        }
        return *this;
    }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { if (p_) (void)hipFree(p_); }

    template <class T = void> T* as() const { return static_cast<T*>(p_); }
    explicit operator bool() const { return p_ != nullptr; }
    void* release() // ownership leaves
    {
        void* q = p_;
        p_ = nullptr;
        return q;
    }

private:
    void* p_ = nullptr;
};

// start .. stop on a stream, in milliseconds; the events are created at the first start
class EventPair {
public:
    EventPair() = default;
    EventPair(const EventPair&) = delete;
    EventPair& operator=(const EventPair&) = delete;
    ~EventPair()
    {
        if (e0_) (void)hipEventDestroy(e0_);
        if (e1_) (void)hipEventDestroy(e1_);
    }
    void start(hipStream_t stream)
    {
        if (!e0_) HIP_THROW(hipEventCreate(&e0_));
        if (!e1_) HIP_THROW(hipEventCreate(&e1_));
        HIP_THROW(hipEventRecord(e0_, stream));
    }
    // records the stop, waits for the stream and returns the time since start
    double stopAndWait(hipStream_t stream)
    {
        HIP_THROW(hipEventRecord(e1_, stream));
        HIP_THROW(hipStreamSynchronize(stream));
        float ms = 0.f;
        HIP_THROW(hipEventElapsedTime(&ms, e0_, e1_));
        return ms;
    }

private:
    hipEvent_t e0_ = nullptr, e1_ = nullptr;
};

} // namespace crt
