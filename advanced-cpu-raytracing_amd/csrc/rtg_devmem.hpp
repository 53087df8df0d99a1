// The owners of device memory and of pinned host words: every hipMalloc / hipFree and
// hipHostMalloc / hipHostFree of the library is in this header (rtg_host_alloc / rtg_host_free,
// the public pinned-memory API, apart).  Host-only; needs the HIP runtime header alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

namespace rtg {

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;      // entries in use
    size_t cap = 0;    // entries allocated (>= n: update() keeps an allocation that is large enough)
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n), cap(o.cap) { o.p = nullptr; o.n = o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p; n = o.n; cap = o.cap;
            o.p = nullptr; o.n = o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);   // hipFree waits for the device
        p = nullptr;
        n = cap = 0;
    }
    // what the kernels are handed: null for an empty table, as after upload()
    T* ptr() const { return n ? p : nullptr; }
    hipError_t alloc(size_t count) {
        release();
        n = cap = count;
        return count ? hipMalloc(&p, count * sizeof(T)) : hipSuccess;
    }
    // Grow-only: nothing when `count` entries fit; otherwise the old allocation is freed first and
    // count + slack(count) entries are allocated.  The growth policies differ between the callers
    // and are theirs; so is any wait for a stream that may still use the old allocation.
    template <typename Slack>
    hipError_t reserve(size_t count, Slack slack) {
        if (count <= cap) return hipSuccess;
        release();
        const size_t want = count + slack(count);
        hipError_t e = hipMalloc(&p, want * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return e; }
        n = cap = want;
        return hipSuccess;
    }
    hipError_t reserve(size_t count) { return reserve(count, [](size_t) { return (size_t)0; }); }
    hipError_t upload(const std::vector<T>& v) {
        release();
        n = cap = v.size();
        if (n == 0) return hipSuccess;
        hipError_t e = hipMalloc(&p, n * sizeof(T));
        if (e != hipSuccess) { n = cap = 0; return e; }
        return hipMemcpy(p, v.data(), n * sizeof(T), hipMemcpyHostToDevice);
    }
    // In place on `st` where `v` fits the allocation: work enqueued on `st` before sees the old
    // entries, work after it the new ones; `v` must outlive the copy.  A table that outgrows its
    // capacity is reallocated: hipFree waits for the device (every stream's work), and p changes.
    hipError_t update(const std::vector<T>& v, hipStream_t st) {
        if (v.size() > cap) {
            release();
            hipError_t e = hipMalloc(&p, v.size() * sizeof(T));
            if (e != hipSuccess) return e;
            cap = v.size();
        }
        n = v.size();
        return n ? hipMemcpyAsync(p, v.data(), n * sizeof(T), hipMemcpyHostToDevice, st) : hipSuccess;
    }
};

// Page-locked host words the device copies into (a level's size, an overflow flag).
template <typename T>
struct PinnedBuf {
    T* p = nullptr;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t count) {
        if (p) { (void)hipHostFree(p); p = nullptr; }
        return hipHostMalloc(&p, count * sizeof(T));
    }
    T& operator[](size_t i) const { return p[i]; }
};

}  // namespace rtg
