// Statistics pooling over row ranges of a row matrix (pool_segments.hip): declarations for the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xvec {

// y[rows][ldy] (elem 0: fp32, 1: bf16), C channels; segment i = rows [row0[i], row0[i] + n[i]) -> out[i][2C] = mean ‖ unbiased std.
// scale / shift: nullptr, or a per-channel affine map of the rows applied to the statistics instead
// (mean = shift + scale * mean_r, std = |scale| * std_r).  A segment with n <= 0, row0 < 0 or row0 + n > rows reads nothing
// and gets a NaN row.
struct PoolSegArgs {
    const void* y;
    int elem;
    int64_t rows;
    int ldy, C;
    const int64_t* row0;     // device [n_segments]
    const int32_t* n;        // device [n_segments]
    int64_t n_segments;
    const float* scale;
    const float* shift;
    float* out;              // [n_segments][2C]
};
// 16-byte loads when the base, the row stride and C rounded up to the vector allow (a vector may read the padding columns
// C..ldy of its row, never past the row); the element-wise variant of the same kernel otherwise.  pool_segments_vector is that choice (host only).
bool pool_segments_vector(const void* y, int elem, int ldy, int C);
hipError_t launch_pool_segments(const PoolSegArgs& a, hipStream_t s);

// (utt, start, len) in INPUT frames of a packed batch (offsets[n_utts + 1]) -> (row0, n) in layer 5's compact row layout:
// recording u keeps len_u - cum rows starting at offsets[u] - cum * u, so the segment's rows are
// [offsets[u] - cum * u + start, ... + len - cum).  A segment with utt outside [0, n_utts), start < 0, len <= cum or
// start + len past its recording gets n = 0 (a NaN row of launch_pool_segments).
hipError_t launch_segment_rows(const int32_t* utt, const int32_t* start, const int32_t* len, int64_t n_segments,
                               const int64_t* offsets, int n_utts, int cum, int64_t* row0, int32_t* n, hipStream_t s);

}  // namespace xvec
