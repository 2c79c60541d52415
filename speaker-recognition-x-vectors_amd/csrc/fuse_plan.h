// The host side of score fusion (csrc/fuse.hip, include/xvec_fuse.h): the argument checks, the words a block leaves per pass
// and the workspace layout.  The blocks of a pass and the depth of its sums are calibration's (calib_plan.h): the summation
// order is one.  Host-compilable (no HIP header), so that tests/test_fuse.py can ask it on the CPU
// (tests/abi/fuse_plan_dump.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/xvec_fuse.h"
#include "calib_plan.h"
#include "plan_support.h"
#include "trial_plan.h"

namespace xvec {
namespace fuse_plan {

constexpr int kMaxTerms = XVEC_FUSE_MAX_TERMS;
constexpr int kThreads = calib_plan::kThreads;
constexpr int kItems = calib_plan::kItems;
constexpr int kTile = calib_plan::kTile;
constexpr int kMaxBlocks = calib_plan::kMaxBlocks;
constexpr int kMaxIter = calib_plan::kMaxIter;
constexpr int kStateBytes = 1024;
constexpr int kGatherCounts = 5;                       // targets, non-targets, NaN, bad index, infinite

using calib_plan::apply_col_tiles;
using calib_plan::apply_tiles;
using calib_plan::check_fit;
using calib_plan::pass_blocks;
using calib_plan::sum_depth;
using trial_plan::count_ok;

inline bool terms_ok(int64_t k) { return k >= 1 && k <= kMaxTerms; }

// Sums of one Newton pass: J, K + 1 gradient components, (K + 1)(K + 2) / 2 Hessian entries.
constexpr int pass_words(int k) { return (k + 1) * (k + 4) / 2 + 1; }
// What the gather leaves per block: the counts, then every term's sum, minimum and maximum.
constexpr int gather_words(int k) { return kGatherCounts + 3 * k; }
// Doubles between the rows of two blocks' partials.
constexpr int partial_stride(int k) { return pass_words(k) > gather_words(k) ? pass_words(k) : gather_words(k); }
// Where entry (i, j), j <= i <= K, of the Hessian lies among a pass's words (index K is the bias).
constexpr int hess_word(int k, int i, int j) { return 1 + (k + 1) + i * (i + 1) / 2 + j; }
constexpr int term_ulps(int k) { return XVEC_FUSE_TERM_ULPS(k); }
static_assert(pass_words(kMaxTerms) == 55 && pass_words(1) == 6, "include/xvec_fuse.h: words(K)");
static_assert(term_ulps(1) == XVEC_CALIB_TERM_ULPS, "one term is calibration");

// ---------------------------------------------------------------- workspace

struct Layout {
    size_t state;           // kStateBytes: the Newton state
    size_t partials;        // double [kMaxBlocks, partial_stride(K)]
    size_t planes;          // double [K, n]: the gathered values, plane-major
    size_t fit_bits;        // uint8 [n]: 1 target, 0 non-target, 2 left out
    size_t total;           // 0: n or K refused
};

inline Layout make_layout(int64_t n, int64_t k) {
    Layout l{};
    if (!count_ok(n) || !terms_ok(k)) return l;
    Carver c;
    l.state = c.take_bytes(kStateBytes);
    l.partials = c.take_bytes((size_t)kMaxBlocks * partial_stride((int)k) * sizeof(double));
    l.planes = c.take_bytes((size_t)n * (size_t)k * sizeof(double));
    l.fit_bits = c.take_bytes((size_t)n);
    l.total = c.total();
    return l;
}

// ---------------------------------------------------------------- argument checks: 0, or 1 with the reason in why

// n_cols_min: what a MATRIX term's row stride must reach
inline int check_terms(const xvec_fuse_term* terms, int32_t n_terms, int64_t n_cols, Refusal& why) {
    if (!terms_ok(n_terms)) return why.refuse("n_terms = %d must lie in 1 .. %d", n_terms, kMaxTerms);
    if (!terms) return why.refuse("null pointer: terms");
    for (int k = 0; k < n_terms; ++k) {
        const xvec_fuse_term& t = terms[k];
        if (t.kind != XVEC_FUSE_MATRIX && t.kind != XVEC_FUSE_ROW && t.kind != XVEC_FUSE_COL)
            return why.refuse("term %d: unknown kind %d", k, t.kind);
        if (!t.data) return why.refuse("term %d: null pointer: data", k);
        if (t.kind == XVEC_FUSE_MATRIX && t.ld < n_cols)
            return why.refuse("term %d: ld = %lld is smaller than n_cols = %lld", k, (long long)t.ld, (long long)n_cols);
    }
    return 0;
}

inline int check_ridge(double l2, Refusal& why) {
    if (!(l2 >= 0.0) || l2 > 1.7976931348623157e308) return why.refuse("l2 = %g must be finite and not negative", l2);
    return 0;
}

// the trial list (the pieces of trial_plan::check_trials that do not speak of one matrix)
inline int check_fit_trials(const xvec_fuse_term* terms, int32_t n_terms, int64_t n_rows, int64_t n_cols, const void* row_idx,
                            const void* col_idx, const void* is_target, int64_t n_trials, Refusal& why, bool* too_large) {
    if (trial_plan::check_trial_count(n_trials, why, too_large) || trial_plan::check_shape(n_rows, n_cols, why)) return 1;
    if (check_terms(terms, n_terms, n_cols, why)) return 1;
    if (!is_target) return why.refuse("null pointer: is_target");
    return trial_plan::check_index_pair(row_idx, col_idx, why) ||
           trial_plan::check_vector_form(row_idx, n_rows, n_cols, n_trials, why);
}

inline int check_fit_all_pairs(const xvec_fuse_term* terms, int32_t n_terms, int64_t n_rows, int64_t n_cols,
                               const void* row_class, const void* col_class, Refusal& why, bool* too_large) {
    *too_large = false;
    if (trial_plan::check_shape(n_rows, n_cols, why) || check_terms(terms, n_terms, n_cols, why)) return 1;
    if (!row_class || !col_class) return why.refuse("null pointer: row_class / col_class");
    return trial_plan::check_cell_count(n_rows, n_cols, why, too_large);
}

inline int check_fuse_apply(const xvec_fuse_term* terms, int32_t n_terms, int64_t n_rows, int64_t n_cols, const void* fit,
                            const void* out, int64_t ld_out, Refusal& why, bool* too_large) {
    *too_large = false;
    if (trial_plan::check_shape(n_rows, n_cols, why) || check_terms(terms, n_terms, n_cols, why)) return 1;
    if (ld_out < n_cols)
        return why.refuse("ld_out = %lld must be at least n_cols = %lld", (long long)ld_out, (long long)n_cols);
    if (!out || !fit) return why.refuse("null pointer: fit / out");
    for (int k = 0; k < n_terms; ++k) {
        if (out != terms[k].data) continue;
        if (terms[k].kind != XVEC_FUSE_MATRIX) return why.refuse("out is the data of term %d, which is not a MATRIX term", k);
        if (terms[k].ld != ld_out)
            return why.refuse("in place (out is the data of term %d) needs ld_out == ld (got %lld and %lld)", k,
                              (long long)ld_out, (long long)terms[k].ld);
    }
    if (apply_tiles(n_rows, n_cols) > 0x7fffffff) {
        *too_large = true;
        return why.refuse("%lld x %lld cells are %lld tiles: more than 2^31 - 1", (long long)n_rows, (long long)n_cols,
                          (long long)apply_tiles(n_rows, n_cols));
    }
    return 0;
}

}  // namespace fuse_plan
}  // namespace xvec
