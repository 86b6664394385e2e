// devbuf.h -- the one owner of a device buffer that only grows (host only).  Every growable buffer of the engine and of
// a live group is a DevBuf: it frees itself, so no teardown names it, and it regrows by the one rule of devbuf_rule.h.
#pragma once
#include <hip/hip_runtime.h>

#include "devbuf_rule.h"

// what the DevBufs that report here have done (mlggd_debug_buffers): device allocations ever made, bytes held now
struct DevBufStats {
    long long allocs = 0, bytes = 0;
};

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;                // elements of T
    DevBufStats *stats = nullptr;  // where the last allocation was counted; it outlives the buffer

    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap), stats(o.stats) { o.p = nullptr, o.cap = 0; }
    ~DevBuf() { release(); }

    // the caller has made sure that nothing on the device still uses the buffer
    void release() {
        if (p) {
            hipFree(p);
            stats->bytes -= (long long)(cap * sizeof(T));
        }
        p = nullptr;
        cap = 0;
    }

    // At least `need` elements: nothing happens while the buffer holds them.  Otherwise `drain` (if given) is
    // synchronised, the old allocation freed -- its contents are dropped -- and `alloc` elements allocated, zero-filled
    // on `zero` (if given).  A failure leaves the buffer empty (p == nullptr, cap == 0).
    hipError_t grow(size_t need, size_t alloc, DevBufStats &s, const hipStream_t *zero, const hipStream_t *drain) {
        if (!devbuf_rule::regrows(need, cap)) return hipSuccess;
        hipError_t rc = drain ? hipStreamSynchronize(*drain) : hipSuccess;
        if (rc != hipSuccess) return rc;
        release();
        rc = hipMalloc((void **)&p, alloc * sizeof(T));
        if (rc != hipSuccess) {
            p = nullptr;
            return rc;
        }
        cap = alloc;
        stats = &s;
        s.allocs++;
        s.bytes += (long long)(alloc * sizeof(T));
        if (zero && (rc = hipMemsetAsync(p, 0, alloc * sizeof(T), *zero)) != hipSuccess) release();
        return rc;
    }
};
