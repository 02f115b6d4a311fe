// Owners of what the library takes from the HIP runtime: device memory, pinned host memory, events, streams.  Each is a
// member of the struct that uses it and is released with that struct -- members go in reverse order of declaration --
// so that no teardown keeps a list of them and none can be forgotten.  They cannot be copied or moved, and hold nothing
// but the raw handle, which is read as .p / .e / .s wherever it is used.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#define PB_LOCAL __attribute__((visibility("hidden")))      // shared between the library's files, not exported

struct pb_handle;
struct PB_LOCAL Unique { Unique() = default; Unique(Unique &&) = delete; };      // neither copied nor moved

template <class T>
struct PB_LOCAL DevBuf : Unique {
    T *p = nullptr;
    size_t cap = 0;      // elements
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t alloc(size_t n)      // n elements in place of what it held; counted nowhere
    {
        release();
        hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
    hipError_t grow(pb_handle *h, size_t n);      // at least n elements, on demand; h->device_bytes follows (pb_internal.h)
    hipError_t from_host(const T *src, size_t n, hipStream_t st) { return hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, st); }
    // (dst = nullptr: an output the caller left out)
    hipError_t to_host(void *dst, size_t n, hipStream_t st) const { return dst ? hipMemcpyAsync(dst, p, n * sizeof(T), hipMemcpyDeviceToHost, st) : hipSuccess; }
};

// page-locked host memory: a copy to or from it is a DMA transfer that does not wait for the host
template <class T>
struct PB_LOCAL PinBuf : Unique {
    T *p = nullptr;
    size_t cap = 0;      // elements
    ~PinBuf() { release(); }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    hipError_t grow(size_t n)      // at least n elements; what it held is gone when it had to grow
    {
        if (n <= cap) return hipSuccess;
        release();
        hipError_t e = hipHostMalloc((void **)&p, n * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) cap = n;
        return e;
    }
};

struct PB_LOCAL Event : Unique {
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDisableTiming) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }      // once
};

// (made where it is used, with hipStreamCreateWithFlags / WithPriority / hipExtStreamCreateWithCUMask on .s)
struct PB_LOCAL Stream : Unique {
    hipStream_t s = nullptr;
    ~Stream() { (void)destroy(); }
    hipError_t destroy() { hipError_t r = s ? hipStreamDestroy(s) : hipSuccess; s = nullptr; return r; }
};

// events that wait to be used again (the stage timers')
struct PB_LOCAL EventPool : Unique {
    std::vector<hipEvent_t> free;
    ~EventPool() { for (hipEvent_t e : free) (void)hipEventDestroy(e); }
};
