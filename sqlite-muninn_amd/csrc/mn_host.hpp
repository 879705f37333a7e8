// mn_host.hpp — host-side idioms the modules share: the HIP status check, the formatter behind every module's
// thread-local error string, and a scope-bound arena of device buffers.
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
