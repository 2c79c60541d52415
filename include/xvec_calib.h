/* xvec_calib.h -- C ABI of score calibration in libxvec_hip.so: linear logistic regression, Cllr, PAV minCllr.
 *
 * Not in the reference (plda_score_stat.py stops at EER / minDCF, which are properties of the score ORDER); the step every
 * speaker-verification toolkit puts behind scoring and normalisation so that a score can be read as a log-likelihood ratio
 * (BOSARIS: train_linear_calibration, cllr, min_cllr).  Four calls:
 *   xvec_calib_fit       the affine map llr = a s + b that minimises the prior-weighted logistic objective on a trial list;
 *   xvec_calib_apply     out = a S + b over a score matrix, a and b read from the DEVICE record the fit left;
 *   xvec_calib_cllr      Cllr and the actual DCF at the Bayes threshold of trials read as LLRs;
 *   xvec_calib_min_cllr  Cllr after the best monotone map (pool-adjacent-violators), and that map's segments.
 *
 * TRIALS are selected exactly as include/xvec_eval.h selects them: row_idx / col_idx / is_target over an fp64 matrix with row
 * stride ld; the plain vector (row_idx == col_idx == NULL, n_rows == 1); and every cell with row_class / col_class /
 * skip_diagonal.  A NaN score or an index outside the matrix is counted (n_nan, n_bad_index) and left out; the cell of a bad
 * index is never read.  n_trials <= 2^31 - 1.
 *
 * softplus(x) = max(x, 0) + log1p(exp(-|x|)), and softplus(0) is taken as ln 2 itself: in bits (divided by ln 2) it is
 * exactly 1, so that Cllr of all-zero LLRs and minCllr of all-equal scores are exactly 1.
 *
 * FIT.  With tau = logit(p_target), P targets and N non-targets among the trials kept,
 *   J(a, b) = p_target / P sum_targets softplus(-(a s + b + tau)) + (1 - p_target) / N sum_non-targets softplus(a s + b + tau)
 * over the fp64 scores (not rounded to fp32).  The trials kept and their target bits are gathered once into the workspace;
 * their mean mu and standard deviation sd (sum (s - mu)^2 / n; 1 where that is 0) are taken, and Newton's method runs on
 * (a', b') with z = (s - mu) / sd, a = a' / sd, b = b' - a' mu / sd, from (0, 0), with the exact 2 x 2 Hessian.  One pass
 * per iteration gives J, both gradient components and the three Hessian entries at the trial point y; a one-block kernel
 * reduces the blocks' partials and then
 *   ACCEPTS y when it is the first point or J(y) <= J(x) + 2^-40 |J(x)| (x the last accepted point), else HALVES the step:
 *   y = x + d / 2;
 *   after an acceptance solves H d = -g (when det H <= 1e-12 H_aa H_bb: with 1e-12 trace(H) + 1e-300 added to the
 *   diagonal; each |d| capped at 8), and is CONVERGED when max(|d_a|, |d_b|) <= XVEC_CALIB_STEP_TOL max(1, |a'|, |b'|):
 *   the reported point is y + d, objective_bits is J(y) / ln 2 (it differs from J(y + d) by O(|d|^2) < 1e-17 J).
 * The launch sequence is fixed by max_iter; once the device flag says converged the remaining passes return at once.  No
 * iterate or sum crosses to the host, and no call synchronises with it.
 *
 * SUMMATION ORDER (every floating-point sum of this unit; B = XVEC_CALIB_THREADS).  G = min(ceil(n / (B ITEMS)),
 * XVEC_CALIB_MAX_BLOCKS) blocks of B threads.  Block k, thread t adds its terms in rising index order over the trials
 * k B ITEMS + j B + t (j < ITEMS), then the same G B ITEMS further on, and so on; the 64 lanes of a wave combine in a
 * butterfly, the B / 64 waves' sums are added in wave order; the G block partials are summed the same way by one block
 * (thread t: partials t, t + B, ...).  A term therefore passes through at most
 *   depth(n) = ceil(n / (G B)) + 22
 * additions, and is itself computed to XVEC_CALIB_TERM_ULPS units in the last place: the argument a' z + b' + tau carries five
 * roundings, the logistic function turns a relative argument error r into at most |x| r of the term, and exp / log1p / the
 * quotient add six.  The error of each sum is below  c eps sum |terms|,  c = depth(n) + XVEC_CALIB_TERM_ULPS,  eps = 2^-53.
 * No float atomics anywhere; every output is bit-identical from call to call and whatever the workspace held before.
 *
 * Conventions as xvec_hip.h: DEVICE pointers, asynchronous on the caller's stream, no allocation (the caller passes a
 * workspace of the queried size), return codes as xvec_hip.h (0 = OK) with the message from xvec_calib_last_error().
 */
#ifndef XVEC_CALIB_H
#define XVEC_CALIB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

#define XVEC_CALIB_THREADS 256      /* B: threads of every block of this unit */
#define XVEC_CALIB_ITEMS 8          /* trials a thread takes per round of the multi-sum passes */
#define XVEC_CALIB_MAX_BLOCKS 1024  /* G never exceeds it: one block reduces the partials */
#define XVEC_CALIB_TERM_ULPS 64
#define XVEC_CALIB_HULL_CHUNK 16    /* C: points a thread reduces to their lower hull; groups merged per level */
#define XVEC_CALIB_HULL_FINAL 256   /* F: groups one block finishes */
#define XVEC_CALIB_APPLY_ROWS 8     /* xvec_calib_apply: a block computes a tile of ROWS x COLS cells */
#define XVEC_CALIB_APPLY_COLS 256
#define XVEC_CALIB_STEP_TOL 1e-9

#define XVEC_CALIB_CONVERGED 0
#define XVEC_CALIB_MAX_ITER 1       /* max_iter passes made, or no finite step left to take (a separable set driven to
                                       saturation: gradient and Hessian both 0); a, b: the last accepted point (finite) */
#define XVEC_CALIB_ONE_CLASS 2      /* no target or no non-target left: a, b, objective_bits NaN */
#define XVEC_CALIB_INF_SCORE 3      /* an infinite score among the trials kept: a, b, objective_bits NaN */

/* Written by the device (64 bytes; a and b first: xvec_calib_apply reads them there). */
typedef struct {
    double a, b;
    double objective_bits;    /* J / ln 2: Cllr of the fitted map when p_target = 0.5 */
    int64_t n_target;
    int64_t n_nontarget;
    int64_t n_nan;
    int64_t n_bad_index;
    int32_t n_iter;           /* passes made */
    int32_t status;           /* XVEC_CALIB_CONVERGED ... */
} xvec_calib_fit_result;

/* Written by the device.  threshold = log((1 - p_target) c_fa) - log(p_target c_miss), the Bayes threshold; a trial is
 * rejected iff llr <= threshold (the tie rule of xvec_eval.h), so act_dcf is on the scale of xvec_eval_result.min_dcf:
 * c_miss p_miss p_target + c_fa p_fa (1 - p_target).  Infinite LLRs follow IEEE 754: a target at -inf makes cllr +inf.
 * With no target or no non-target left the four doubles but threshold are NaN. */
typedef struct {
    double cllr;              /* (mean_targets softplus(-l) + mean_non-targets softplus(l)) / (2 ln 2) */
    double act_dcf;
    double p_miss;            /* targets at or below the threshold / n_target */
    double p_fa;              /* non-targets above it / n_nontarget */
    double threshold;
    int64_t n_target;
    int64_t n_nontarget;
    int64_t n_nan;
    int64_t n_bad_index;
} xvec_calib_cllr_result;

/* Written by the device.  n_left_out: trials with a NaN score or a bad index (the sort does not tell them apart). */
typedef struct {
    double min_cllr;          /* NaN with no target or no non-target left */
    int64_t n_segments;       /* always the full count, whatever the capacity of the segment arrays */
    int64_t n_target;
    int64_t n_nontarget;
    int64_t n_left_out;
} xvec_calib_pav_result;

const char* xvec_calib_last_error(void);

/* Scratch for n_trials trials, enough for every call of this unit (0 for a count the calls refuse).  For the all-pairs
 * forms n_trials = n_rows * n_cols. */
size_t xvec_calib_workspace_bytes(int64_t n_trials);

/* The fit over a trial list (arguments as xvec_eval_trials).  0 < p_target < 1; 1 <= max_iter <= 1000. */
int xvec_calib_fit(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                   const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, double p_target, int32_t max_iter,
                   xvec_calib_fit_result* out, void* workspace, size_t workspace_bytes, xvec_stream stream);

/* The fit over every cell (arguments as xvec_eval_all_pairs). */
int xvec_calib_fit_all_pairs(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_class,
                             const int32_t* col_class, int32_t skip_diagonal, double p_target, int32_t max_iter,
                             xvec_calib_fit_result* out, void* workspace, size_t workspace_bytes, xvec_stream stream);

/* out[i, j] = a * scores[i, j] + b over [n_rows, n_cols] (row strides ld, ld_out), a and b from the DEVICE record `fit`.
 * The product and the sum are rounded separately (no fused multiply-add): the result is numpy's a * S + b bit for bit, and a
 * symmetric matrix stays exactly symmetric.  out may be scores itself with ld_out == ld; it must not overlap it otherwise. */
int xvec_calib_apply(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const xvec_calib_fit_result* fit,
                     double* out, int64_t ld_out, xvec_stream stream);

/* Cllr and actual DCF of the trials read as LLRs, one pass (arguments as xvec_eval_trials / xvec_eval_all_pairs).
 * c_miss, c_fa > 0 and finite; 0 < p_target < 1. */
int xvec_calib_cllr(const double* llrs, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                    const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, double c_miss, double c_fa,
                    double p_target, xvec_calib_cllr_result* out, void* workspace, size_t workspace_bytes,
                    xvec_stream stream);
int xvec_calib_cllr_all_pairs(const double* llrs, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_class,
                              const int32_t* col_class, int32_t skip_diagonal, double c_miss, double c_fa, double p_target,
                              xvec_calib_cllr_result* out, void* workspace, size_t workspace_bytes, xvec_stream stream);

/* minCllr by pool-adjacent-violators (arguments as xvec_eval_sorted_keys, which it calls: the scores are rounded to fp32
 * and keyed as the evaluation keys them).  Equal keys form one tie group; the cumulative-sum diagram has one point per tie
 * group at (trials so far, targets so far), and the PAV solution is its greatest convex minorant, found exactly (64-bit
 * integer cross products; collinear interior vertices dropped, so the segment list is unique):
 *   level 1     a thread reduces XVEC_CALIB_HULL_CHUNK consecutive trials to the lower hull of their points;
 *   level l     a thread merges XVEC_CALIB_HULL_CHUNK adjacent groups of level l - 1 into one, in place;
 *   final       once at most XVEC_CALIB_HULL_FINAL groups are left one block merges them pairwise, adds the origin, and
 *               sums, thread t over the segments t, t + B, ... and then as above,
 *                 [t softplus(-llr) / P + f softplus(llr) / N] / (2 ln 2),   llr = log(t / f) - log(P / N)
 *               over the segments with t targets and f non-targets (0 for t = 0 or f = 0; no Laplace correction).
 * Segment j < min(n_segments, seg_capacity): seg_k_end[j], seg_tp_end[j] the trials and targets up to its end,
 * seg_score[j] the largest fp32 score in it, seg_llr[j] its LLR (-inf for t = 0, +inf for f = 0).  The four arrays may be
 * NULL when seg_capacity == 0. */
int xvec_calib_min_cllr(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                        const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, xvec_calib_pav_result* out,
                        int64_t* seg_k_end, int64_t* seg_tp_end, float* seg_score, double* seg_llr, int64_t seg_capacity,
                        void* workspace, size_t workspace_bytes, xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_CALIB_H */
