// The host side of score calibration (csrc/calib.hip, include/xvec_calib.h): the argument checks, the block and partial
// counts of the multi-sum passes, the level plan of the hull reduction and the workspace layout.  Host-compilable (no HIP
// header, like vad_plan.h and tsne_plan.h), so that tests/test_calibrate.py can ask it on the CPU
// (tests/abi/calib_plan_dump.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/xvec_calib.h"
#include "plan_support.h"
#include "trial_plan.h"

namespace xvec {
namespace calib_plan {

constexpr int kThreads = XVEC_CALIB_THREADS;
constexpr int kItems = XVEC_CALIB_ITEMS;
constexpr int kTile = kThreads * kItems;               // trials a block takes per round of a multi-sum pass
constexpr int kMaxBlocks = XVEC_CALIB_MAX_BLOCKS;
constexpr int kChunk = XVEC_CALIB_HULL_CHUNK;
constexpr int kFinal = XVEC_CALIB_HULL_FINAL;
constexpr int kHullTile = kThreads * kChunk;           // trials a block of the first hull level owns
constexpr int kMaxLevels = 8;                          // 16^6 * 256 > 2^31: six levels at most
constexpr int kPartialWords = 8;                       // doubles (or int64) a block leaves per pass
constexpr int kMaxIter = 1000;
static_assert(kFinal <= kThreads, "the final block owns one group per thread");
static_assert(kMaxBlocks % kThreads == 0, "the reducing block reads whole rounds of partials");

// the trial forms and their checks are the family's (trial_plan.h)
using trial_plan::check_all_pairs;
using trial_plan::check_matrix;
using trial_plan::check_trials;
using trial_plan::count_ok;

// Blocks of a multi-sum pass over n trials: a function of n alone (not of the device), so that the sums' order is too.
inline int64_t pass_blocks(int64_t n) {
    const int64_t b = (n + kTile - 1) / kTile;
    return b < kMaxBlocks ? b : kMaxBlocks;
}

// The most additions a term passes through (include/xvec_calib.h, SUMMATION ORDER).
inline int64_t sum_depth(int64_t n) {
    const int64_t per_round = pass_blocks(n) * kThreads;
    return (n + per_round - 1) / per_round + 22;
}

// Blocks of xvec_calib_apply: tiles of XVEC_CALIB_APPLY_ROWS x XVEC_CALIB_APPLY_COLS cells, row-major.
inline int64_t apply_col_tiles(int64_t n_cols) { return (n_cols + XVEC_CALIB_APPLY_COLS - 1) / XVEC_CALIB_APPLY_COLS; }
inline int64_t apply_tiles(int64_t n_rows, int64_t n_cols) {
    return apply_col_tiles(n_cols) * ((n_rows + XVEC_CALIB_APPLY_ROWS - 1) / XVEC_CALIB_APPLY_ROWS);
}

// ---------------------------------------------------------------- the hull reduction

// After level l there are groups[l] groups, each the lower hull of the points of span[l] consecutive trials, kept in place at
// the front of those trials' slots.  levels >= 1; groups[levels] <= kFinal.
struct HullPlan {
    int32_t levels;
    int64_t groups[kMaxLevels + 1];      // groups[0] = n (every trial its own slot)
    int64_t span[kMaxLevels + 1];        // span[0] = 1
};

// 0, or 1 when n is refused (never for count_ok(n)).
inline int plan_hull(int64_t n, HullPlan* out) {
    HullPlan p{};
    if (!count_ok(n)) return 1;
    p.groups[0] = n;
    p.span[0] = 1;
    int l = 0;
    do {
        if (l == kMaxLevels) return 1;
        ++l;
        p.groups[l] = (p.groups[l - 1] + kChunk - 1) / kChunk;
        p.span[l] = p.span[l - 1] * kChunk;
    } while (p.groups[l] > kFinal);
    p.levels = l;
    *out = p;
    return 0;
}

// ---------------------------------------------------------------- workspace

// Byte offsets of the workspace's parts (each 256-byte aligned).  The fit uses state .. fit_bits, Cllr state and partials,
// minCllr state, block_counts and everything behind fit_bits.
struct Layout {
    size_t state;           // 256 bytes: the Newton state / the totals of a call
    size_t partials;        // double [kMaxBlocks, kPartialWords]
    size_t fit_scores;      // double [n]: the gathered trial scores
    size_t fit_bits;        // uint8 [n]: 1 target, 0 non-target, 2 left out
    size_t eval;            // eval_bytes: the window xvec_eval_sorted_keys works in
    size_t keys;            // uint32 [n]: the sorted keys
    size_t bits;            // uint8 [n]: the bits carried with them
    size_t points;          // int32 [n, 2]: (trials so far, targets so far), the hulls in place
    size_t block_counts;    // uint32 [2, hull_blocks]: targets and kept trials of every block of the first level
    size_t group_counts;    // uint32 [groups[1] + groups[2]]: the points of every group, levels alternating
    size_t total;
    int64_t hull_blocks;
};

// eval_bytes = xvec_eval_workspace_bytes(n) (the library asks eval.hip; the dump program is told).
inline Layout make_layout(int64_t n, size_t eval_bytes) {
    Layout l{};
    HullPlan h;
    if (plan_hull(n, &h) || eval_bytes == 0) return l;
    const size_t un = (size_t)n;
    l.hull_blocks = (n + kHullTile - 1) / kHullTile;
    Carver c;
    l.state = c.take_bytes(256);
    l.partials = c.take_bytes((size_t)kMaxBlocks * kPartialWords * sizeof(double));
    l.fit_scores = c.take_bytes(un * sizeof(double));
    l.fit_bits = c.take_bytes(un);
    l.eval = c.take_bytes(eval_bytes);
    l.keys = c.take_bytes(un * sizeof(uint32_t));
    l.bits = c.take_bytes(un);
    l.points = c.take_bytes(un * 2 * sizeof(int32_t));
    l.block_counts = c.take_bytes((size_t)l.hull_blocks * 2 * sizeof(uint32_t));
    l.group_counts = c.take_bytes((size_t)(h.groups[1] + (h.levels >= 2 ? h.groups[2] : 0)) * sizeof(uint32_t));
    l.total = c.total();
    return l;
}

// ---------------------------------------------------------------- argument checks: 0, or 1 with the reason in why

inline int check_prior(double p_target, Refusal& why) {
    if (!(p_target > 0.0 && p_target < 1.0)) return why.refuse("p_target = %g must lie strictly between 0 and 1", p_target);
    return 0;
}

inline int check_fit(double p_target, int32_t max_iter, Refusal& why) {
    if (check_prior(p_target, why)) return 1;
    if (max_iter < 1 || max_iter > kMaxIter) return why.refuse("max_iter = %d must lie in 1 .. %d", max_iter, kMaxIter);
    return 0;
}

inline int check_costs(double c_miss, double c_fa, double p_target, Refusal& why) {
    if (!(c_miss > 0.0) || !(c_fa > 0.0) || c_miss > 1e300 || c_fa > 1e300)
        return why.refuse("c_miss = %g and c_fa = %g must be finite and > 0", c_miss, c_fa);
    return check_prior(p_target, why);
}

inline int check_apply(const void* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const void* fit, const void* out,
                       int64_t ld_out, Refusal& why, bool* too_large) {
    *too_large = false;
    if (trial_plan::check_shape(n_rows, n_cols, why)) return 1;
    if (ld < n_cols || ld_out < n_cols)
        return why.refuse("ld = %lld and ld_out = %lld must be at least n_cols = %lld", (long long)ld, (long long)ld_out,
                          (long long)n_cols);
    if (!scores || !out || !fit) return why.refuse("null pointer: scores / fit / out");
    if (out == scores && ld_out != ld)
        return why.refuse("in place (out == scores) needs ld_out == ld (got %lld and %lld)", (long long)ld_out, (long long)ld);
    if (apply_tiles(n_rows, n_cols) > 0x7fffffff) {
        *too_large = true;
        return why.refuse("%lld x %lld cells are %lld tiles: more than 2^31 - 1", (long long)n_rows, (long long)n_cols,
                          (long long)apply_tiles(n_rows, n_cols));
    }
    return 0;
}

inline int check_segments(const void* k_end, const void* tp_end, const void* score, const void* llr, int64_t capacity,
                          Refusal& why) {
    if (capacity < 0) return why.refuse("seg_capacity = %lld must not be negative", (long long)capacity);
    if (capacity > 0 && (!k_end || !tp_end || !score || !llr))
        return why.refuse("null pointer: seg_k_end / seg_tp_end / seg_score / seg_llr with seg_capacity = %lld", (long long)capacity);
    return 0;
}

}  // namespace calib_plan
}  // namespace xvec
