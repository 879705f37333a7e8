// mn_host.hpp — host-side idioms the modules share: the HIP status check, the formatter behind every module's
// thread-local error string, a scope-bound arena of device buffers, and an owned device array for what a handle keeps.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

// A failed HIP call becomes the module's error string and the function's -1.  SETERR is the module's printf-like setter.
#define MN_HIPCHK(SETERR, expr)                                                                  \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess) {                                                                 \
            SETERR("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return -1;                                                                           \
        }                                                                                        \
    } while (0)

// what every *set_err does between va_start and va_end
inline void mn_vformat(std::string &dst, const char *fmt, va_list ap) {
    char buf[512];
    vsnprintf(buf, sizeof(buf), fmt, ap);
    dst = buf;
}

// Device buffers of one call, freed on scope exit.  alloc returns null when the device has no room; the vector's own
// growth can throw std::bad_alloc, which the entry point's MN_GUARD_END turns into its error value.
struct DevArena {
    std::vector<void *> p;
    template <typename T> T *alloc(size_t n) {
        p.push_back(nullptr); // the slot first: a growth that throws then leaves no buffer behind
        if (hipMalloc(&p.back(), (n ? n : 1) * sizeof(T)) != hipSuccess) {
            p.pop_back();
            return nullptr;
        }
        return static_cast<T *>(p.back());
    }
    ~DevArena() {
        for (void *q : p)
            (void)hipFree(q);
    }
};

// One device array that outlives the call: a handle's work struct holds it and frees it by being deleted.  It knows its
// capacity, so a group of them needs no bookkeeping beside it.  Both ways to a size return 0, or -1 after `seterr` (the
// module's printf-like setter) has the message under the entry point's name `who`; a failure leaves the buffer as it was
// or empty, never dangling.
template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0; // elements
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    operator T *() const { return p; }
    void release() {
        if (p)
            (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }

    // exactly `n` elements unless it holds that many already; what it held is not kept.  (hipFree waits for the device,
    // so nothing in flight reads the old array; it goes first, and the two never stand side by side.)
    int fit(void (*seterr)(const char *, ...), const char *who, size_t n) {
        if (n <= cap)
            return 0;
        release();
        if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) {
            p = nullptr;
            seterr("%s: out of device memory (%zu bytes)", who, n * sizeof(T));
            return -1;
        }
        cap = n;
        return 0;
    }

    // the same with the first `keep` elements kept: copied on `st`, which is synchronised before the old array is freed
    int grow(void (*seterr)(const char *, ...), const char *who, size_t n, size_t keep, hipStream_t st) {
        if (n <= cap || keep == 0)
            return fit(seterr, who, n);
        T *q = nullptr;
        if (hipMalloc(&q, n * sizeof(T)) != hipSuccess) {
            seterr("%s: out of device memory (%zu bytes)", who, n * sizeof(T));
            return -1;
        }
        hipError_t e = hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            (void)hipFree(q);
            seterr("%s: growing a device array failed: %s", who, hipGetErrorString(e));
            return -1;
        }
        (void)hipFree(p);
        p = q;
        cap = n;
        return 0;
    }
};
