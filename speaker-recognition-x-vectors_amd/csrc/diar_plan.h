// The host side of average-linkage clustering (csrc/diar.hip, include/xvec_diar.h): the checks of rec_start and want, the
// layout of the workspace, the block size a recording's block runs with and the grouping of a batch into launches.
// Host-compilable (no HIP header, like score_tiles.h and mfcc_tables.h), so that tests/test_diarize.py can ask it on the CPU
// (tests/abi/diar_plan_dump.cpp); mat_elems alone is also called from the kernel that lays the matrices out on the device.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/xvec_diar.h"
#include "rec_plan.h"

#if defined(__HIPCC__)
#define XVEC_DIAR_FN __host__ __device__ __forceinline__
#else
#define XVEC_DIAR_FN inline
#endif

namespace xvec {
namespace diar_plan {

// Doubles the working matrix of a recording of n segments takes: n rows of n cells, dense (row stride n), rounded up to a whole
// number of 256-byte lines so that the next matrix starts on one.
XVEC_DIAR_FN int64_t mat_elems(int64_t n) { return (n * n + 31) & ~(int64_t)31; }

// rec_start [n_rec + 1]: from 0, every recording with 1 .. XVEC_DIAR_MAX_SEGMENTS segments, fewer than 2^31 in all.
// 0, or 1 with the reason in why.
inline int check_rec_start(const int64_t* rs, int32_t n_rec, Refusal& why) {
    return rec_plan::check_rec_start(rs, n_rec, {"segment", XVEC_DIAR_MAX_SEGMENTS, "XVEC_DIAR_MAX_SEGMENTS"}, why);
}

// want [n_rec] (may be null: no recording asks for a count): no negative entry.
inline int check_want(const int32_t* want, int32_t n_rec, Refusal& why) {
    if (!want) return 0;
    for (int32_t r = 0; r < n_rec; ++r)
        if (want[r] < 0) return why.refuse("want[%d] = %d must not be negative (0 = stop by threshold)", r, want[r]);
    return 0;
}

// Byte offsets of the workspace's parts (each 256-byte aligned) for a checked rec_start.
struct Layout {
    size_t rec_start;      // int64 [n_rec + 1]: the copy of rec_start_host
    size_t want;           // int32 [n_rec]: the copy of want_host (unused when that is null)
    size_t mat_off;        // int64 [n_rec]: where each working matrix starts, in doubles from `mats` (written on the device)
    size_t best_v;         // double [N]: every row's first best score ...
    size_t best_i;         // int32 [N]: ... and partner, written with the working copy
    size_t mats;           // the working matrices, recording after recording, mat_elems(n_r) doubles each
    size_t total;
};

inline Layout make_layout(const int64_t* rs, int32_t n_rec) {
    Layout l{};
    const size_t N = (size_t)rs[n_rec];
    Carver c;
    l.rec_start = c.take_bytes(((size_t)n_rec + 1) * sizeof(int64_t));
    l.want = c.take_bytes((size_t)n_rec * sizeof(int32_t));
    l.mat_off = c.take_bytes((size_t)n_rec * sizeof(int64_t));
    l.best_v = c.take_bytes(N * sizeof(double));
    l.best_i = c.take_bytes(N * sizeof(int32_t));
    l.mats = l.total = c.total();
    for (int32_t r = 0; r < n_rec; ++r) l.total += (size_t)mat_elems(rs[r + 1] - rs[r]) * sizeof(double);
    return l;
}

// Byte offset of recording r's working matrix in the workspace.
inline size_t matrix_offset(const Layout& l, const int64_t* rs, int32_t r) {
    size_t off = l.mats;
    for (int32_t q = 0; q < r; ++q) off += (size_t)mat_elems(rs[q + 1] - rs[q]) * sizeof(double);
    return off;
}

// Threads of the block that clusters a recording of n segments: a single wave while a lane can own a row (no barrier then
// costs more than a wave's own ordering), else four waves, which walk a row of XVEC_DIAR_MAX_SEGMENTS cells in eight strides.
inline int block_threads(int64_t n) { return n <= XVEC_DIAR_THREADS_SMALL ? XVEC_DIAR_THREADS_SMALL : XVEC_DIAR_THREADS_LARGE; }

// One launch: a block per recording first .. first + count - 1; the blocks whose recording wants another block size leave at
// once.  A batch is at most two launches, the hull of the small recordings and the hull of the large ones.
struct Group {
    int32_t first, count, threads;
};

inline int plan_groups(const int64_t* rs, int32_t n_rec, Group out[2]) {
    int n = 0;
    for (int threads : {XVEC_DIAR_THREADS_SMALL, XVEC_DIAR_THREADS_LARGE}) {
        int32_t lo = -1, hi = -1;
        for (int32_t r = 0; r < n_rec; ++r) {
            if (block_threads(rs[r + 1] - rs[r]) != threads) continue;
            if (lo < 0) lo = r;
            hi = r;
        }
        if (lo >= 0) out[n++] = Group{lo, hi - lo + 1, threads};
    }
    return n;
}

}  // namespace diar_plan
}  // namespace xvec
