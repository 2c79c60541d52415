// What the host-only plan headers (diar_plan.h, vad_plan.h, tsne_plan.h, calib_plan.h, report_plan.h, vbx_plan.h, der_plan.h,
// trial_plan.h, rec_plan.h) and the C-ABI translation units (through host_support.h) both need: the 256-byte alignment, the
// workspace carver, the typed pointer of a recorded byte offset, the reason of a refused argument check.  No HIP header, so
// that the plan headers stay compilable by the host compiler alone (tests/abi/*_dump.cpp).
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdio>

namespace xvec {

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Hands out consecutive 256-byte aligned buffers of one workspace: as byte offsets (take_bytes; what a plan header's Layout
// records) or as pointers from a base (take<T>).  A plan function is written once over a Carver: called with a null base it
// only sizes the workspace (every pointer comes back null), with the real base it names the buffers.
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* ws = nullptr) : base(static_cast<char*>(ws)) {}
    size_t take_bytes(size_t bytes) {
        const size_t at = off;
        off += align256(bytes);
        return at;
    }
    template <typename T>
    T* take(size_t count) {
        const size_t at = take_bytes(count * sizeof(T));
        return base ? reinterpret_cast<T*>(base + at) : nullptr;
    }
    size_t total() const { return off; }
};

// The part of workspace `ws` that a plan header's Layout records at byte offset `off`, as a T*.
template <typename T>
inline T* part(void* ws, size_t off) {
    return reinterpret_cast<T*>(static_cast<char*>(ws) + off);
}

// Why a plan header's check refused its arguments.  A check returns 0, or `why.refuse(...)` = 1 with the reason in why.text;
// the translation unit forwards it with ErrorChannel::refused (host_support.h).
struct Refusal {
    char text[256] = "";
    __attribute__((format(printf, 2, 3))) int refuse(const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof(text), fmt, ap);
        va_end(ap);
        return 1;
    }
};

}  // namespace xvec
