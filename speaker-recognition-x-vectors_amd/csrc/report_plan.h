// The host side of the trial report (csrc/report.hip, include/xvec_report.h): the argument checks, the tiling of the image pass,
// the split of a row's piece of an output plane into its ragged head, its aligned 16-byte body and its ragged tail, the map from
// a wide image's column to its panel, the thinning rule of the DET curve and the workspace layout.  Host-compilable (no HIP
// header, like calib_plan.h), so that tests/test_report.py can ask it on the CPU (tests/abi/report_plan_dump.cpp).  The functions
// marked XVEC_HD are the ones the kernels call too (wide_cols, split_piece, det_step, det_keep); everything else runs on the host.
//
// The checks of the trial forms are trial_plan.h's, re-exported here; the key of a score (include/xvec_eval.h) and its inverse
// are trial_device.h's.  Both are shared with csrc/eval.hip and csrc/calib.hip.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/xvec_report.h"
#include "plan_support.h"
#include "trial_plan.h"

#ifdef __HIPCC__
#define XVEC_HD __host__ __device__
#else
#define XVEC_HD
#endif

namespace xvec {
namespace report_plan {

constexpr int kThreads = XVEC_REPORT_THREADS;
constexpr int kTile = XVEC_REPORT_TILE;                // cells a block of the image pass stages
constexpr int kRangeBlocks = XVEC_REPORT_RANGE_BLOCKS;
constexpr int kRangeTile = 4 * kThreads;               // consecutive columns of one row a block of the range pass takes at a time
constexpr int kDetItems = XVEC_REPORT_DET_ITEMS;
constexpr int kDetTile = XVEC_REPORT_DET_TILE;
constexpr int kGap = XVEC_REPORT_GAP;
constexpr int kChunk = 16;                             // bytes of a vector store
constexpr int kMaxPlanes = 25;                         // 1 + 3 + 3 narrow planes, 3 wide images x 3 channels x 2 panels
static_assert(kDetTile == kThreads * kDetItems, "a thread scans kDetItems consecutive trials");
static_assert(kTile % kThreads == 0 && kRangeBlocks % kThreads == 0, "whole rounds of the block");

// the trial forms and their checks are the family's (trial_plan.h)
using trial_plan::check_all_pairs;
using trial_plan::check_matrix;
using trial_plan::check_shape;
using trial_plan::check_trials;
using trial_plan::count_ok;

// ---------------------------------------------------------------- the image pass

// A tile is tile_rows(C) x tile_cols(C) cells: consecutive columns of one row, or whole rows of a matrix narrower than a tile.
inline int64_t tile_cols(int64_t n_cols) { return n_cols < kTile ? n_cols : kTile; }
inline int64_t tile_rows(int64_t n_cols) { return n_cols < kTile ? kTile / n_cols : 1; }
inline int64_t col_tiles(int64_t n_cols) { return (n_cols + tile_cols(n_cols) - 1) / tile_cols(n_cols); }
inline int64_t row_tiles(int64_t n_rows, int64_t n_cols) { return (n_rows + tile_rows(n_cols) - 1) / tile_rows(n_cols); }
inline int64_t image_tiles(int64_t n_rows, int64_t n_cols) { return row_tiles(n_rows, n_cols) * col_tiles(n_cols); }

XVEC_HD inline int64_t wide_cols(int64_t n_cols) { return 2 * n_cols + kGap; }

// The first wide column of a panel: 0 the EER threshold's (columns [0, C)), 1 the gap ([C, C + 5)), 2 the minDCF threshold's
// ([C + 5, 2C + 5)).  xvec_report_images places the panels' planes with it (the column offset of a plane); the kernel writes the
// gap at n_cols + k itself.
inline int64_t panel_first(int panel, int64_t n_cols) { return panel == 0 ? 0 : panel == 1 ? n_cols : n_cols + kGap; }
// The inverse, for the CPU check of the layout only (tests/test_report.py holds panel_first to it column by column; no kernel
// calls it -- what the kernel writes where is held by the GPU tests): the panel of wide column w and, in *cell, the matrix
// column behind it (the offset inside the gap for panel 1).
inline int wide_panel(int64_t w, int64_t n_cols, int64_t* cell) {
    if (w < n_cols) {
        *cell = w;
        return 0;
    }
    if (w < n_cols + kGap) {
        *cell = w - n_cols;
        return 1;
    }
    *cell = w - n_cols - kGap;
    return 2;
}

// The bytes [a, b) of an output plane (addresses), split for the stores: [a, body) byte by byte, [body, tail) in aligned
// 16-byte pieces, [tail, b) byte by byte.  body and tail are multiples of 16 unless the whole piece lies inside one.
struct Piece {
    uint64_t body, tail;
};
XVEC_HD inline Piece split_piece(uint64_t a, uint64_t b) {
    Piece p;
    const uint64_t up = (a + (kChunk - 1)) & ~(uint64_t)(kChunk - 1);
    p.body = up < b ? up : b;
    const uint64_t down = b & ~(uint64_t)(kChunk - 1);
    p.tail = down > p.body ? down : p.body;
    return p;
}

// ---------------------------------------------------------------- the DET curve

// floor(count * grid / total) in 64 bits (count <= total < 2^31, grid < 2^31); 0 for an empty class
XVEC_HD inline int64_t det_step(int64_t count, int64_t total, int64_t grid) { return total > 0 ? count * grid / total : 0; }

// Whether the thinned curve keeps a point: tp / nn its counts, tp_prev / nn_prev those of the distinct score before it.
XVEC_HD inline bool det_keep(int64_t tp, int64_t nn, int64_t tp_prev, int64_t nn_prev, int64_t P, int64_t N, int64_t grid,
                             bool first, bool last) {
    if (grid == 0 || first || last) return true;
    return det_step(tp, P, grid) != det_step(tp_prev, P, grid) || det_step(N - nn, N, grid) != det_step(N - nn_prev, N, grid);
}

inline int64_t det_blocks(int64_t n) { return (n + kDetTile - 1) / kDetTile; }

// Byte offsets of the workspace's parts (each 256-byte aligned).
struct Layout {
    size_t state;           // 256 bytes: the counters and totals of a call
    size_t eval;            // eval_bytes: the window xvec_eval_sorted_keys works in
    size_t keys;            // uint32 [n]: the sorted keys
    size_t bits;            // uint8 [n]: the bits carried with them
    size_t row;             // int32 [n]: all pairs, the row of every cell (-1: a skipped diagonal cell)
    size_t col;             // int32 [n]
    size_t tgt;             // uint8 [n]
    size_t sums;            // uint32 [3, blocks]: targets, kept trials and run ends of every block; then their scans
    size_t keep_sums;       // uint32 [blocks]: kept points of every block of the thinning pass
    size_t pt_thr;          // float [n]: the unthinned points
    size_t pt_tp;           // int32 [n]
    size_t pt_nn;           // int32 [n]
    size_t total;
    int64_t blocks;
};

// eval_bytes = xvec_eval_workspace_bytes(n) (the library asks eval.hip; the dump program is told).
inline Layout make_layout(int64_t n, size_t eval_bytes) {
    Layout l{};
    if (!count_ok(n) || eval_bytes == 0) return l;
    const size_t un = (size_t)n;
    l.blocks = det_blocks(n);
    Carver c;
    l.state = c.take_bytes(256);
    l.eval = c.take_bytes(eval_bytes);
    l.keys = c.take_bytes(un * sizeof(uint32_t));
    l.bits = c.take_bytes(un);
    l.row = c.take_bytes(un * sizeof(int32_t));
    l.col = c.take_bytes(un * sizeof(int32_t));
    l.tgt = c.take_bytes(un);
    l.sums = c.take_bytes((size_t)l.blocks * 3 * sizeof(uint32_t));
    l.keep_sums = c.take_bytes((size_t)l.blocks * sizeof(uint32_t));
    l.pt_thr = c.take_bytes(un * sizeof(float));
    l.pt_tp = c.take_bytes(un * sizeof(int32_t));
    l.pt_nn = c.take_bytes(un * sizeof(int32_t));
    l.total = c.total();
    return l;
}

inline size_t range_bytes() { return align256((size_t)kRangeBlocks * 3 * sizeof(double)); }

// Blocks of the range pass: a function of the shape alone, so that the order of the reduction is too.
inline int64_t range_col_tiles(int64_t n_cols) { return (n_cols + kRangeTile - 1) / kRangeTile; }
inline int64_t range_blocks(int64_t n_rows, int64_t n_cols) {
    const int64_t t = n_rows * range_col_tiles(n_cols);      // n_rows < 2^31, tiles of a row < 2^21
    return t < kRangeBlocks ? t : kRangeBlocks;
}

// ---------------------------------------------------------------- argument checks: 0, or 1 with the reason in why

inline int check_map(const void* map, int64_t ld_map, int64_t n_cols, Refusal& why) {
    if (!map) return why.refuse("null pointer: map");
    if (ld_map < n_cols) return why.refuse("ld_map = %lld is smaller than n_cols = %lld", (long long)ld_map, (long long)n_cols);
    if (ld_map % 4 != 0 || reinterpret_cast<uintptr_t>(map) % 4 != 0)
        return why.refuse("the map must be 4-byte aligned and ld_map = %lld a multiple of 4", (long long)ld_map);
    return 0;
}

// *too_large: the refusal is one of size (XVEC_ERR_TOO_LARGE), not of form
inline int check_trial_map(const void* row_idx, const void* col_idx, const void* is_target, int64_t n_trials, int64_t n_rows,
                           int64_t n_cols, const void* map, int64_t ld_map, Refusal& why, bool* too_large) {
    *too_large = false;
    if (n_trials < 0) return why.refuse("n_trials = %lld must not be negative", (long long)n_trials);
    if (n_trials > 0x7fffffff) {
        *too_large = true;
        return why.refuse("n_trials = %lld exceeds 2^31 - 1", (long long)n_trials);
    }
    if (check_shape(n_rows, n_cols, why) || check_map(map, ld_map, n_cols, why)) return 1;
    if (n_trials > 0 && (!row_idx || !col_idx || !is_target)) return why.refuse("null pointer: row_idx / col_idx / is_target");
    return 0;
}

inline int check_images(const void* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const void* map, int64_t ld_map,
                        const void* range, uint32_t which, int32_t dtype, void* const* images, Refusal& why, bool* too_large) {
    *too_large = false;
    if (check_matrix(scores, ld, n_rows, n_cols, why) || check_map(map, ld_map, n_cols, why)) return 1;
    if (!range) return why.refuse("null pointer: range");
    if (which == 0 || (which & ~(uint32_t)XVEC_REPORT_ALL)) return why.refuse("which = 0x%x: one to six of the bits 0x%x", which, XVEC_REPORT_ALL);
    if (dtype != XVEC_REPORT_U8 && dtype != XVEC_REPORT_F32) return why.refuse("dtype = %d is neither XVEC_REPORT_U8 nor XVEC_REPORT_F32", dtype);
    static const char* const names[6] = {"score_matrix", "ground_truth", "ground_truth_scores", "prediction",
                                         "correct_prediction", "false_prediction"};
    for (int i = 0; i < 6; ++i) {
        if (!(which >> i & 1u)) continue;
        if (!images[i]) return why.refuse("null pointer: %s is selected", names[i]);
        if (dtype == XVEC_REPORT_F32 && reinterpret_cast<uintptr_t>(images[i]) % 4 != 0)
            return why.refuse("%s: a float32 image must be 4-byte aligned", names[i]);
    }
    if (n_rows > ((int64_t)1 << 56) / wide_cols(n_cols)) {      // 3 channels x 4 bytes: every address offset stays below 2^62
        *too_large = true;
        return why.refuse("%lld x %lld cells: a wide image of more than 2^56 elements per channel", (long long)n_rows, (long long)n_cols);
    }
    if (image_tiles(n_rows, n_cols) > 0x7fffffff) {
        *too_large = true;
        return why.refuse("%lld x %lld cells are %lld tiles: more than 2^31 - 1", (long long)n_rows, (long long)n_cols,
                          (long long)image_tiles(n_rows, n_cols));
    }
    return 0;
}

inline int check_curve(int64_t grid, const void* header, const void* thr, const void* tp, const void* nn, int64_t capacity,
                       Refusal& why) {
    if (grid < 0 || grid > 0x7fffffff) return why.refuse("grid = %lld must lie in 0 .. 2^31 - 1", (long long)grid);
    if (!header) return why.refuse("null pointer: header");
    if (capacity < 0) return why.refuse("capacity = %lld must not be negative", (long long)capacity);
    if (capacity > 0 && (!thr || !tp || !nn)) return why.refuse("null pointer: thr / tp / nn with capacity = %lld", (long long)capacity);
    return 0;
}

}  // namespace report_plan
}  // namespace xvec
