// Host-side plumbing of the C-ABI translation units (xvec_api, mfcc, score, plda_train, eval, augment): the error text behind a
// *_last_error() export, workspace carving, the CU count.  Host code only: nothing here is called from a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>

#include "../../include/xvec_hip.h"

namespace xvec {

// The message behind one *_last_error() export.  Every translation unit declares ITS OWN `thread_local ErrorChannel`: the
// channels stay independent of each other and per thread, as the headers promise.  fail / launch_ok return the code to return.
struct ErrorChannel {
    char text[512] = "";
    __attribute__((format(printf, 3, 4))) int fail(int code, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof(text), fmt, ap);
        va_end(ap);
        return code;
    }
    int launch_ok(const char* what) {      // right after a kernel launch
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? XVEC_OK : fail(XVEC_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
    }
    const char* c_str() const { return text; }
};

// The channel behind xvec_train_last_error(): defined in tdnn_train.hip, shared with train_tail.hip (one header, one channel).
ErrorChannel& train_error_channel();

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

inline int workspace_ok(size_t have, size_t need, ErrorChannel& err) {
    return have >= need ? XVEC_OK : err.fail(XVEC_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", have, need);
}

// Hands out consecutive 256-byte aligned buffers of one workspace.  A plan function is written once over a Carver: called
// with a null base it only sizes the workspace (every pointer comes back null), with the real base it names the buffers.
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* ws) : base(static_cast<char*>(ws)) {}
    template <typename T>
    T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += align256(count * sizeof(T));
        return p;
    }
    size_t total() const { return off; }
};

// Compute units of the current device (256 where the query fails), asked once per device.
inline int device_cu_count() {
    static int cache[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    const bool slot = dev >= 0 && dev < 64;
    if (slot && cache[dev]) return cache[dev];
    hipDeviceProp_t prop;
    const int n = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
    if (slot) cache[dev] = n;             // benign if raced (idempotent)
    return n;
}

}  // namespace xvec
