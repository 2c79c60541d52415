// The argument checks of the units that consume a trial list, or every cell of a score matrix as a trial: trial evaluation
// (eval.hip), score calibration (calib_plan.h) and the trial report (report_plan.h).  One text per refusal, so that the three
// units cannot drift apart in what they accept.  Host-compilable (no HIP header), like the plan headers that re-export these
// names.  Every check returns 0, or 1 with the reason in why.
#pragma once
#include <cstddef>
#include <cstdint>

#include "plan_support.h"

namespace xvec {
namespace trial_plan {

inline bool count_ok(int64_t n) { return n >= 1 && n <= 0x7fffffff; }

inline int check_shape(int64_t n_rows, int64_t n_cols, Refusal& why) {
    if (!count_ok(n_rows) || !count_ok(n_cols))
        return why.refuse("score matrix [%lld, %lld]: both sizes must be in 1 .. 2^31 - 1", (long long)n_rows, (long long)n_cols);
    return 0;
}

inline int check_matrix(const void* scores, int64_t ld, int64_t n_rows, int64_t n_cols, Refusal& why) {
    if (!scores) return why.refuse("null pointer: scores");
    if (check_shape(n_rows, n_cols, why)) return 1;
    if (ld < n_cols) return why.refuse("ld = %lld is smaller than n_cols = %lld", (long long)ld, (long long)n_cols);
    return 0;
}

// The pieces of check_trials and check_all_pairs.  eval.hip composes them itself: between them it answers an unnamed "null
// pointer" of its own (include/xvec_eval.h).  *too_large: the refusal is one of size (XVEC_ERR_TOO_LARGE), not of form.

inline int check_trial_count(int64_t n_trials, Refusal& why, bool* too_large) {
    *too_large = false;
    if (n_trials < 1) return why.refuse("n_trials = %lld: need at least one trial", (long long)n_trials);
    if (n_trials > 0x7fffffff) {
        *too_large = true;
        return why.refuse("n_trials = %lld exceeds 2^31 - 1", (long long)n_trials);
    }
    return 0;
}

inline int check_index_pair(const void* row_idx, const void* col_idx, Refusal& why) {
    if ((row_idx == nullptr) != (col_idx == nullptr)) return why.refuse("row_idx and col_idx must both be given or both be null");
    return 0;
}

inline int check_vector_form(const void* row_idx, int64_t n_rows, int64_t n_cols, int64_t n_trials, Refusal& why) {
    if (!row_idx && (n_rows != 1 || n_cols < n_trials))
        return why.refuse("without index arrays the scores are a vector: n_rows = 1 and n_cols >= n_trials (got [%lld, %lld] for "
                          "%lld trials)", (long long)n_rows, (long long)n_cols, (long long)n_trials);
    return 0;
}

// after check_shape: both sizes are below 2^31, the product does not overflow
inline int check_cell_count(int64_t n_rows, int64_t n_cols, Refusal& why, bool* too_large) {
    *too_large = n_rows * n_cols > 0x7fffffff;
    if (*too_large) return why.refuse("%lld x %lld cells exceed 2^31 - 1 trials", (long long)n_rows, (long long)n_cols);
    return 0;
}

inline int check_trials(const void* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const void* row_idx, const void* col_idx,
                        const void* is_target, int64_t n_trials, Refusal& why, bool* too_large) {
    if (check_trial_count(n_trials, why, too_large) || check_matrix(scores, ld, n_rows, n_cols, why)) return 1;
    if (!is_target) return why.refuse("null pointer: is_target");
    return check_index_pair(row_idx, col_idx, why) || check_vector_form(row_idx, n_rows, n_cols, n_trials, why);
}

inline int check_all_pairs(const void* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const void* row_class,
                           const void* col_class, Refusal& why, bool* too_large) {
    *too_large = false;
    if (check_matrix(scores, ld, n_rows, n_cols, why)) return 1;
    if (!row_class || !col_class) return why.refuse("null pointer: row_class / col_class");
    return check_cell_count(n_rows, n_cols, why, too_large);
}

}  // namespace trial_plan
}  // namespace xvec
