/* xvec_fuse.h -- C ABI of score fusion in libxvec_hip.so: logistic fusion of several systems' scores and of quality measures.
 *
 * Not in the reference; the link between score calibration (include/xvec_calib.h: one score, llr = a s + b) and the evaluation
 * of the result, which BOSARIS calls train_linear_fusion.  Three calls:
 *   xvec_fuse_fit            the weights and the bias of  llr(i, j) = b + sum_k w_k f_k(i, j)  that minimise the prior-weighted
 *                            logistic objective on a trial list;
 *   xvec_fuse_fit_all_pairs  the same over every cell of the matrices;
 *   xvec_fuse_apply          out = ((w_0 f_0 + w_1 f_1) + ...) + b over the whole matrix, weights and bias read from the DEVICE
 *                            record the fit left.
 * Cllr, the actual DCF, minCllr, EER and the trial report of the fused matrix are the existing calls over `out`.
 *
 * TERMS.  1 <= K <= XVEC_FUSE_MAX_TERMS terms, a HOST array of K xvec_fuse_term (each `data` a DEVICE pointer to fp64):
 *   XVEC_FUSE_MATRIX   f(i, j) = data[i * ld + j]: a score matrix [n_rows, n_cols] with row stride ld >= n_cols;
 *   XVEC_FUSE_ROW      f(i, j) = data[i]: a quality measure of the row side (ld is ignored);
 *   XVEC_FUSE_COL      f(i, j) = data[j]: one of the column side (ld is ignored).
 * Duration-aware calibration llr = a s + c log(dur_enrol) + d log(dur_test) + b is K = 3: a MATRIX, a ROW and a COL term.
 *
 * TRIALS are selected exactly as include/xvec_calib.h and include/xvec_eval.h select them: row_idx / col_idx / is_target; the
 * plain vector (row_idx == col_idx == NULL, n_rows == 1: trial t is cell (0, t)); and every cell with row_class / col_class /
 * skip_diagonal.  A trial with an index outside [n_rows, n_cols] is counted in n_bad_index and none of its cells is read, in
 * any term.  A trial for which ANY term is NaN is counted once in n_nan and left out.  An infinite value in any term of a
 * trial kept ends the fit with XVEC_FUSE_INF_SCORE, no target or no non-target among them with XVEC_FUSE_ONE_CLASS (w, b and
 * the two objectives NaN in both cases).  n_trials <= 2^31 - 1.
 *
 * FIT.  With tau = logit(p_target), P targets and N non-targets among the trials kept, llr = b + sum_k w_k f_k,
 *   J = p_target / P sum_targets softplus(-(llr + tau)) + (1 - p_target) / N sum_non-targets softplus(llr + tau)
 *       + l2 / 2 sum_k w'_k^2
 * (softplus as xvec_calib.h; l2 >= 0 and finite, 0 = none) where w'_k = w_k sd_k are the STANDARDISED weights.  The bias is
 * never penalised.  All on the device; no iterate or sum crosses to the host, no call synchronises with it, and the launch
 * sequence is fixed by max_iter and K:
 *   1. GATHER     the K values of every trial kept go into K planes [K][n_trials] of the workspace (plane-major: every later
 *                 load is coalesced), its target bit into fit_bits as calibration writes it; the same pass takes every
 *                 term's sum, minimum and maximum over the trials kept.
 *   2. STANDARDISE  A term is CONSTANT iff its minimum equals its maximum: an exact test (the rounded mean of equal values
 *                 need not equal them, and a variance of 1e-34 must not become a scale).  For a constant term mu is that
 *                 value, sd = 1, z is exactly 0, the reported weight exactly 0.0 and its bit is set in constant_mask; it takes
 *                 no part in the solve, so the other weights are, bit for bit, those of the fit without it.  Otherwise
 *                 mu = sum / n and sd = sqrt(sum (f - mu)^2 / n) from a second pass; z_k = (f_k - mu_k) * (1 / sd_k).
 *   3. NEWTON     on (w'_1 .. w'_K, b') from 0 with the exact Hessian.  One multi-sum pass per iteration gives J, the K + 1
 *                 gradient components and the (K + 1)(K + 2) / 2 Hessian entries of the data part at the trial point y; a
 *                 one-block kernel reduces the blocks' partials in fixed order, adds the ridge and then
 *                   ACCEPTS y when it is the first point or J(y) <= J(x) + 2^-40 |J(x)| (J the penalised objective, x the last
 *                   accepted point), else HALVES the step: y = x + d / 2;
 *                   after an acceptance solves H d = -g by a Cholesky factorisation of the (at most 9 x 9) matrix of the
 *                   terms that are not constant and the bias.  If a pivot's square is <= 1e-12 times its diagonal entry, or is
 *                   not positive, 1e-12 trace(H) + 1e-300 is added to the whole diagonal and the matrix is factorised again.
 *                   The step is capped at 8 in the max norm, and the fit is CONVERGED when
 *                   max |d| <= XVEC_FUSE_STEP_TOL max(1, max |x|): the reported point is y + d.
 *   4. FINISH     w_k = w'_k / sd_k;  b = b' - sum_k w_k mu_k, the sum taken in term order.  objective_bits is the data part
 *                 of J(y) divided by ln 2 (Cllr of the fused scores when p_target = 0.5), penalty_bits the ridge part of J(y)
 *                 divided by ln 2; y is the point the last step was taken from, so both differ from their values at the
 *                 reported point by at most l2 sum_k |w'_k| max |d| (first order; 0 without a ridge) plus O(|d|^2).
 * Once the device flag says done the remaining passes return at once.
 *
 * SUMMATION ORDER (every floating-point sum of this unit) is that of xvec_calib.h with B = XVEC_CALIB_THREADS, ITEMS =
 * XVEC_CALIB_ITEMS: G = min(ceil(n / (B ITEMS)), XVEC_CALIB_MAX_BLOCKS) blocks; block k, thread t adds its terms in rising
 * index order over the trials k B ITEMS + j B + t (j < ITEMS), then the same G B ITEMS further on; lanes in a butterfly,
 * waves in wave order, the G block partials by one block (thread t: partials t, t + B, ...).  It is a function of n alone:
 * not of K, nor of how many loads a kernel keeps in flight.  A term passes through at most depth(n) = ceil(n / (G B)) + 22
 * additions, and the error of each sum is below
 *   c eps sum |terms|,  c = depth(n) + XVEC_FUSE_TERM_ULPS(K),  eps = 2^-53.
 * The term constant is derived from calibration's.  There the argument a' z + b' + tau carries five roundings (two of z, one
 * product, one sum, one of b' + tau) and exp / log1p / the quotient add six; XVEC_CALIB_TERM_ULPS = 64 allots the remaining
 * 58 units to the five roundings of the argument, 58 / 5 each (the logistic function turns a relative argument error r into
 * at most |x| r of the term).  Here the argument sum_k w'_k z_k + b' + tau carries two roundings per z_k, one product and one
 * addition per term and one of b' + tau: 4 K + 1 roundings at the same 58 / 5 units each, and the transcendental part is
 * unchanged:
 *   XVEC_FUSE_TERM_ULPS(K) = 6 + ceil(58 (4 K + 1) / 5)        (64 at K = 1, 389 at K = 8).
 * No float atomics anywhere; every output is bit-identical from call to call and whatever the workspace held before.
 *
 * WORKSPACE.  xvec_fuse_workspace_bytes(n_trials, n_terms): the state (1024 bytes), the block partials
 * [XVEC_CALIB_MAX_BLOCKS][max(words(K), 5 + 3 K)] doubles (words(K) = (K + 1)(K + 4) / 2 + 1 sums of a pass; the gather
 * leaves five counts and 3 K sums and extremes in the same rows), the planes 8 n K bytes and the bits n bytes, each part
 * 256-byte aligned.  Eight terms over all 23.75 M cells of a 4874 x 4874 matrix are 1.5 GB.
 *
 * Conventions as xvec_hip.h: DEVICE pointers (but for the term array itself), asynchronous on the caller's stream, no
 * allocation, return codes as xvec_hip.h (0 = OK) with the message from xvec_fuse_last_error().
 */
#ifndef XVEC_FUSE_H
#define XVEC_FUSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

#define XVEC_FUSE_MAX_TERMS 8
#define XVEC_FUSE_MATRIX 0
#define XVEC_FUSE_ROW 1
#define XVEC_FUSE_COL 2
#define XVEC_FUSE_STEP_TOL 1e-9
#define XVEC_FUSE_TERM_ULPS(K) (6 + (58 * (4 * (K) + 1) + 4) / 5)

/* numbered as XVEC_CALIB_CONVERGED ... */
#define XVEC_FUSE_CONVERGED 0
#define XVEC_FUSE_MAX_ITER 1        /* max_iter passes made, or no finite step left to take; w, b: the last accepted point */
#define XVEC_FUSE_ONE_CLASS 2
#define XVEC_FUSE_INF_SCORE 3

typedef struct {
    const double* data;       /* device */
    int64_t ld;               /* XVEC_FUSE_MATRIX: the row stride */
    int32_t kind;             /* XVEC_FUSE_MATRIX | XVEC_FUSE_ROW | XVEC_FUSE_COL */
} xvec_fuse_term;

/* Written by the device (128 bytes; w and b first: xvec_fuse_apply reads them there). */
typedef struct {
    double w[XVEC_FUSE_MAX_TERMS];   /* 0 beyond n_terms */
    double b;
    double objective_bits;
    double penalty_bits;
    int64_t n_target;
    int64_t n_nontarget;
    int64_t n_nan;
    int64_t n_bad_index;
    int16_t n_terms;
    int16_t n_iter;                  /* passes made */
    int16_t status;                  /* XVEC_FUSE_CONVERGED ... */
    uint16_t constant_mask;          /* bit k: term k is constant over the trials kept */
} xvec_fuse_result;

const char* xvec_fuse_last_error(void);

/* Scratch of a fit of n_terms terms over n_trials trials (0 for a count or a K the calls refuse).  For the all-pairs form
 * n_trials = n_rows * n_cols. */
size_t xvec_fuse_workspace_bytes(int64_t n_trials, int32_t n_terms);

/* The fit over a trial list.  0 < p_target < 1; l2 >= 0 and finite; 1 <= max_iter <= 1000. */
int xvec_fuse_fit(const xvec_fuse_term* terms, int32_t n_terms, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                  const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, double p_target, double l2,
                  int32_t max_iter, xvec_fuse_result* out, void* workspace, size_t workspace_bytes, xvec_stream stream);

/* The fit over every cell: a target iff row_class[i] == col_class[j]; skip_diagonal leaves the cells i == j out. */
int xvec_fuse_fit_all_pairs(const xvec_fuse_term* terms, int32_t n_terms, int64_t n_rows, int64_t n_cols,
                            const int32_t* row_class, const int32_t* col_class, int32_t skip_diagonal, double p_target,
                            double l2, int32_t max_iter, xvec_fuse_result* out, void* workspace, size_t workspace_bytes,
                            xvec_stream stream);

/* out[i, j] = ((w_0 f_0(i, j) + w_1 f_1(i, j)) + ...) + b over [n_rows, n_cols] (row stride ld_out), the weights and the bias
 * from the DEVICE record `fit`; its w beyond n_terms are not read.  Every product and every sum is rounded separately, in term
 * order with the bias last (no fused multiply-add): numpy's w0 * S0 + w1 * S1 + ... + b bit for bit, so symmetric matrices
 * without a ROW or COL term give an exactly symmetric result.  out may be the data of a MATRIX term with ld_out == ld; it
 * must not overlap a term otherwise (refused where out is a term's data pointer). */
int xvec_fuse_apply(const xvec_fuse_term* terms, int32_t n_terms, int64_t n_rows, int64_t n_cols, const xvec_fuse_result* fit,
                    double* out, int64_t ld_out, xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_FUSE_H */
