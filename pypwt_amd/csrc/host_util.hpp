// host_util.hpp -- small host-side helpers shared by the translation units of the C ABI (plan.cpp, volume.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include "plan.hpp"  // real_t, set_last_error, the status codes

namespace pdwt {

#define HIP_TRY(expr)                                                                                                   \
    do {                                                                                                                \
        hipError_t e_ = (expr);                                                                                         \
        if (e_ != hipSuccess)                                                                                           \
            return ::pdwt::set_last_error(PDWT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                                          __LINE__);                                                                    \
    } while (0)

#define PDWT_TRY(expr)                  \
    do {                                \
        const int rc_ = (expr);         \
        if (rc_ != PDWT_OK) return rc_; \
    } while (0)

static inline int div2(int n) { return (n + (n & 1)) / 2; }  // pdwt/src/utils.cu:24-27

static inline int ilog2(int i) {  // pdwt/src/utils.cu:14-20 (terminates for i <= 0 too)
    int l = 0;
    while (i > 1) {
        i >>= 1;
        ++l;
    }
    return l;
}

static inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// beta of the approximation band under `normalize`: beta / sqrt(2)^levels (pdwt/src/common.cu:229-236)
static inline real_t app_beta(real_t beta, int levels, int normalize) {
    if (normalize > 0) {
        const int n2 = levels / 2;
        beta /= (real_t)(1 << n2);
        if (n2 * 2 != levels) beta = (real_t)(beta / 1.4142135623730951);
    }
    return beta;
}

// selects a device for the lifetime of the object and puts the caller's back; `ok` is false where that failed
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

}  // namespace pdwt
