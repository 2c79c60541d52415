/* xvec_eval.h -- C ABI of trial-list evaluation in libxvec_hip.so: EER and minDCF from device scores.
 *
 * The last stage of the reference's pipeline (main.py:312-336 -> plda_score_stat.py:36-97): pick the
 * score of every trial out of the score matrix, then speechbrain's EER / minDCF
 * (speechbrain.utils.metric_stats, 0.5.12) over the target and non-target scores.  That package is
 * not vendored: parity with it is UNPINNED; tests/eer_ref.py restates its published threshold walk
 * (candidate thresholds = the sorted unique scores and the midpoints of neighbours;
 * FRR = (pos <= t) / P, FAR = (neg > t) / N; the first strict minimum wins; EER = (FAR + FRR) / 2) and
 * the kernels are checked against that restatement.
 *
 * Here the scores stay on the device.  Each trial's score is rounded to fp32 (round to nearest even:
 * the reference hands float32 tensors to EER / minDCF, plda_score_stat.py:96-97) and mapped to an
 * order-preserving 32-bit key (-0.0 and +0.0 share one key), the (key, target bit) pairs are sorted by
 * a stable least-significant-digit radix sort, and both error rates of every distinct score u_k are
 * read off one prefix sum of the target bit: tp_k = targets <= u_k, nn_k = non-targets <= u_k,
 *   FRR_k = tp_k / P,  FAR_k = (N - nn_k) / N.
 * A midpoint has the rates of its lower neighbour and comes later, so it never wins: the distinct
 * scores are all the thresholds that matter.
 *   EER     arg-min of |(N - nn_k) P - tp_k N| in 64-bit integers, lowest k on ties;
 *   minDCF  arg-min of c_miss FRR_k p_target + c_fa FAR_k (1 - p_target) in fp64, lowest k on ties.
 * DEVIATION from the package: the rates are exact here (integer counts, fp64 quotients), not fp32
 * quotients; the package's values differ from these by its own fp32 rounding (a few 1e-8).
 *
 * Conventions as xvec_hip.h: DEVICE pointers, asynchronous on the caller's stream, no allocation (the
 * caller passes a workspace of the queried size), return codes as xvec_hip.h (0 = OK) with the message
 * from xvec_eval_last_error().  No float atomics, every reduction in a fixed order: repeat calls on the
 * same inputs give bit-identical outputs.  n_trials <= 2^31 - 1.
 */
#ifndef XVEC_EVAL_H
#define XVEC_EVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

/* Written by the device.  A trial whose score is NaN or whose index lies outside the matrix is counted
 * (n_nan, n_bad_index) and left out of everything else; its cell is never read when the index is bad.
 * When no target or no non-target trial is left (the package divides by zero there) the six doubles
 * are NaN: the caller treats n_target == 0 or n_nontarget == 0 as an argument error. */
typedef struct {
    double eer;               /* (far + frr) / 2 at eer_threshold */
    double eer_threshold;     /* the fp32 score u_k of the arg-min */
    double far;               /* non-targets above eer_threshold / n_nontarget */
    double frr;               /* targets at or below eer_threshold / n_target */
    double min_dcf;
    double min_dcf_threshold;
    int64_t n_target;
    int64_t n_nontarget;
    int64_t n_nan;
    int64_t n_bad_index;
} xvec_eval_result;

const char* xvec_eval_last_error(void);

/* Scratch for n_trials trials (0 for a count the entry points would refuse).  For
 * xvec_eval_all_pairs n_trials = n_rows * n_cols. */
size_t xvec_eval_workspace_bytes(int64_t n_trials);

/* Trial t is the cell scores[row_idx[t] * ld + col_idx[t]] of the fp64 [n_rows, n_cols] matrix (as
 * xvec_plda_score / xvec_cosine_score leave it; ld = row stride in elements) and a target trial iff
 * is_target[t] != 0.  row_idx == NULL and col_idx == NULL with n_rows == 1 evaluates the plain vector
 * scores[0 .. n_trials) (n_cols >= n_trials). */
int xvec_eval_trials(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                     const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, double c_miss,
                     double c_fa, double p_target, xvec_eval_result* out, void* workspace,
                     size_t workspace_bytes, xvec_stream stream);

/* Every cell is a trial, a target iff row_class[i] == col_class[j]; skip_diagonal != 0 leaves the cells
 * i == j out (a vector against itself).  n_rows * n_cols <= 2^31 - 1. */
int xvec_eval_all_pairs(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols,
                        const int32_t* row_class, const int32_t* col_class, int32_t skip_diagonal,
                        double c_miss, double c_fa, double p_target, xvec_eval_result* out, void* workspace,
                        size_t workspace_bytes, xvec_stream stream);

/* The first two stages alone, for inspection and tests: the sorted keys [n_trials] and the target bit
 * carried with each (1 target, 0 non-target, 2 a trial left out: those sort last).  Arguments as
 * xvec_eval_trials. */
int xvec_eval_sorted_keys(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols,
                          const int32_t* row_idx, const int32_t* col_idx, const uint8_t* is_target,
                          int64_t n_trials, uint32_t* keys_out, uint8_t* bits_out, void* workspace,
                          size_t workspace_bytes, xvec_stream stream);

/* The same two stages with the trial's place instead of its bit: the sorted keys [n_trials] and, next to each key, the 32-bit
 * index t of its trial (the position in the trial list; for all pairs t = row * n_cols + col).  Trials that are left out
 * carry the key 0xffffffff and sort last, their indices with them.  The sort is STABLE: trials with equal keys (equal fp32
 * scores; every trial left out) keep the order of their indices.  The bootstrap (xvec_boot.h) resamples over this order: a
 * replicate changes the weight of a trial, not its place.  One sort serves both payloads (one byte there, four here); the
 * workspace is xvec_eval_sorted_order_workspace_bytes(n_trials), 0 for a count that is refused. */
size_t xvec_eval_sorted_order_workspace_bytes(int64_t n_trials);

int xvec_eval_sorted_order(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                           const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, uint32_t* keys_out,
                           uint32_t* order_out, void* workspace, size_t workspace_bytes, xvec_stream stream);

/* Arguments as xvec_eval_all_pairs; keys_out / order_out [n_rows * n_cols]. */
int xvec_eval_sorted_order_all_pairs(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols,
                                     const int32_t* row_class, const int32_t* col_class, int32_t skip_diagonal,
                                     uint32_t* keys_out, uint32_t* order_out, void* workspace, size_t workspace_bytes,
                                     xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_EVAL_H */
