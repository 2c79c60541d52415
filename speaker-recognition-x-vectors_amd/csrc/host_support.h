// Host-side plumbing of every C-ABI translation unit (xvec_api, mfcc, score, plda_train, eval, snorm, ident, diar, lda,
// augment, resample, vad, tsne, calib, report, vbx, der, tdnn_train*, train_tail*): the error text behind a *_last_error() export, the workspace check,
// the upload of a small host array, the CU count, and through plan_support.h the alignment, the workspace carver, the typed
// pointer of a workspace part and a plan header's refusal (eval, calib and report share theirs: trial_plan.h; diar, vbx and der
// theirs: rec_plan.h).  Host code only: nothing here is called from a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/xvec_hip.h"
#include "plan_support.h"

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
    // a plan header's refusal, as "<call>: <reason>" where the unit's messages name the call
    int refused(int code, const Refusal& why, const char* call = nullptr) {
        return call ? fail(code, "%s: %s", call, why.text) : fail(code, "%s", why.text);
    }
    int launch_ok(const char* what) {      // right after a kernel launch
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? XVEC_OK : fail(XVEC_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
    }
    const char* c_str() const { return text; }
};

// The channel behind xvec_train_last_error(): defined in tdnn_train.hip, shared with train_tail.hip (one header, one channel).
ErrorChannel& train_error_channel();

inline int workspace_ok(size_t have, size_t need, ErrorChannel& err) {
    return have >= need ? XVEC_OK : err.fail(XVEC_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", have, need);
}

// "Workspace given, aligned and large enough".  What the entry points answer is part of the ABI (the headers' error
// conventions; tests/test_workspace_refusals.py holds every answer), so the differences between the units are parameters:
//   - a null workspace is XVEC_ERR_ARG "null pointer: workspace";
//   - t-SNE alone asks for alignment (xvec_tsne.h: 8-byte aligned device pointers; align = 8, 0 = not tested): XVEC_ERR_ARG
//     "workspace is not 8-byte aligned", and alone names the call in front of these two texts (call; null = no prefix);
//   - a workspace below `need` bytes is "workspace too small: <have> < <need> bytes", never prefixed, with XVEC_ERR_WORKSPACE;
//     the training units (xvec_train.h) alone answer XVEC_ERR_ARG for it (small_code).
// The units whose single "null pointer" test names the workspace among other arguments (score, plda_train, eval, lda, augment,
// xvec_model_mean) and xvec_resample, which checks its ratios between the two tests, call workspace_ok alone.
inline int workspace_arg_ok(const void* ws, size_t have, size_t need, ErrorChannel& err, int small_code = XVEC_ERR_WORKSPACE,
                            const char* call = nullptr, size_t align = 0) {
    const char* sep = call ? ": " : "";
    if (!call) call = "";
    if (!ws) return err.fail(XVEC_ERR_ARG, "%s%snull pointer: workspace", call, sep);
    if (align && reinterpret_cast<uintptr_t>(ws) % align != 0)
        return err.fail(XVEC_ERR_ARG, "%s%sworkspace is not %zu-byte aligned", call, sep, align);
    return have >= need ? XVEC_OK : err.fail(small_code, "workspace too small: %zu < %zu bytes", have, need);
}

// `count` elements of a small host array (rec_start, class_start, want) into device memory, in stream order.  XVEC_OK, or
// XVEC_ERR_HIP "<name> copy failed: <hip error>".
template <typename T>
inline int upload(T* dev, const T* host, size_t count, const char* name, hipStream_t s, ErrorChannel& err) {
    const hipError_t e = hipMemcpyAsync(dev, host, count * sizeof(T), hipMemcpyHostToDevice, s);
    return e == hipSuccess ? XVEC_OK : err.fail(XVEC_ERR_HIP, "%s copy failed: %s", name, hipGetErrorString(e));
}

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
