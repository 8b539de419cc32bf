// devres.hpp -- move-only owners of a cr_ctx's device handles.  Each frees in its destructor on the current device
// (cr_destroy sets it before `delete c`): no list of what to free, no virtuals, reference counts or allocator.
#pragma once
#include "chiaro_hip.h"
#include "kernels.hpp" // (hip_runtime.h)

namespace crx {

struct DevBuf {
    void *ptr = nullptr;
    size_t cap = 0; // the bytes asked for when ptr was allocated

    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : ptr(o.ptr), cap(o.cap) { o.ptr = nullptr, o.cap = 0; }
    ~DevBuf() { release(); }
    void release() {
        if (ptr) hipFree(ptr);
        ptr = nullptr, cap = 0;
    }
    template <class T> T *as() const { return (T *)ptr; }
    template <class T> size_t count() const { return cap / sizeof(T); }
    // Grow-only work buffer: reallocated (contents lost) when `need` exceeds the capacity; CR_OK or CR_E_OOM.
    int grow(size_t need) {
        if (need <= cap && ptr) return CR_OK;
        release();
        if (hipMalloc(&ptr, need ? need : 16) != hipSuccess) return ptr = nullptr, CR_E_OOM;
        cap = need;
        return CR_OK;
    }
    // Exactly `bytes`: nothing when the size is unchanged; else freed, allocated and -- only then, when asked --
    // zeroed.  CR_OK, CR_E_OOM, or CR_E_HIP with the memset's error in *e.
    int resize_exact(size_t bytes, bool zero, hipError_t *e = nullptr) {
        if (bytes == cap) return CR_OK;
        release();
        if (hipMalloc(&ptr, bytes) != hipSuccess) return ptr = nullptr, CR_E_OOM;
        cap = bytes;
        const hipError_t m = zero ? hipMemset(ptr, 0, bytes) : hipSuccess;
        if (e) *e = m;
        return m == hipSuccess ? CR_OK : CR_E_HIP;
    }
};

// One raw handle H, created by the owner's create() and released by Free in the destructor.
template <class H, hipError_t (*Free)(H)> struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(const Handle &) = delete;
    Handle &operator=(const Handle &) = delete;
    ~Handle() {
        if (h) Free(h);
    }
    operator H() const { return h; }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
    hipError_t create() { return hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
    hipError_t create(int priority) { return hipStreamCreateWithPriority(&h, hipStreamNonBlocking, priority); }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    hipError_t create(bool timing) {
        return timing ? hipEventCreate(&h) : hipEventCreateWithFlags(&h, hipEventDisableTiming);
    }
};
struct PinnedWords : Handle<void *, hipHostFree> { // (the lanes' queue lengths)
    hipError_t create(size_t n) { return hipHostMalloc(&h, n * sizeof(uint32_t), hipHostMallocDefault); }
    uint32_t *words() const { return (uint32_t *)h; }
};
// cr::TraceEvents (kernels.hpp) as the launchers see and grow it, with its arrays freed here
struct TraceEventsOwner : cr::TraceEvents {
    ~TraceEventsOwner() {
        for (int i = 0; i < 2 * cap; i++) hipEventDestroy(ev[i]);
        delete[] ev;
        delete[] kind;
    }
};

} // namespace crx
