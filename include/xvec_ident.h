/* xvec_ident.h -- C ABI of speaker identification in libxvec_hip.so: speaker models enrolled from several vectors, open-set
 * scores, the k best models of every test segment.
 *
 * The reference scores every utterance under its own id with p_known = 0.0 (plda_classifier.py:86); these are the two other
 * branches of the call it makes, speechbrain's fast_PLDA_scoring, and the step an identification system puts behind them.
 *
 * Speaker models (StatObject_SB.mean_stat_per_model): model c is the plain mean of the rows of x that belong to it,
 *   out[c, d] = (sum of x[order[i], d] over model_start[c] <= i < model_start[c + 1]) / (model_start[c + 1] - model_start[c]).
 * The sum is the class-sum column walk PLDA and LDA training use (four interleaved partial sums per column, combined in a
 * fixed order), the division is one rounding.
 *
 * Open-set scores (the package's p_known != 0 branch).  S[N, T] is fp64, row-major with row stride ld >= T, N models by T
 * test segments; with p = p_known
 *   out[i,j] = S[i,j] - log( p (sum over k != i of exp S[k,j]) / (N - 1) + (1 - p) ).
 * The sum over k != i is never formed as "column total minus own term" (that cancels whenever one model dominates a column,
 * which a target trial does).  Per column j the library keeps m1 = the maximum, i1 = the first row that has it and
 * R = sum over k != i1 of exp(S[k,j] - m1); row i1 uses A = R, every other row A = 1 + (R - exp(S[i,j] - m1)) >= 1 (the 1 is
 * the maximum's own term).  The logarithm stays in the log domain: with q = p A / (N - 1)
 *   L = m1 + log(q + (1 - p) exp(-m1))   when m1 > 0 or p == 1 (the second term is an explicit 0 when p == 1),
 *   L = log(exp(m1) q + (1 - p))         otherwise,
 * so that scores of +-900 neither overflow nor underflow.
 *   A column with a NaN cell is NaN throughout (as numpy gives).  A -inf cell adds 0 to the sums and comes out -inf (a column
 *   of nothing but -inf comes out as S - log(1 - p)).  +inf is undefined beyond not faulting.
 * Rows are walked in slices of XVEC_IDENT_SLICE_ROWS (one wave holds a slice of 64 columns in registers), a block combines
 * the XVEC_IDENT_BLOCK_ROWS rows of its four waves in wave order, and when N is larger the blocks' partials (m1, i1, R) go
 * through the workspace and are merged, with rescaling, in block order.  Every sum has one fixed order that depends on N
 * alone: a column's outputs are a function of that column, N and p, bit-identical whatever T, ld, the base alignment (8 bytes
 * is all that is asked) or the other columns are, and from run to run.
 *
 * Identification.  For every column j the k best rows, best first: larger score first, equal scores by lower row index
 * (-0.0 == +0.0; +-inf are ordinary ordered values).  NaN is never selected; places that cannot be filled get index -1 and
 * score NaN.  decision[j] = the best index if its score >= threshold, else -1 (out of set).  Rows are walked in the slices
 * above, XVEC_IDENT_TOPK_BLOCK_ROWS rows to a block; the lists are kept sorted in registers (compile-time lengths 1, 4 and
 * XVEC_IDENT_MAX_K: the smallest that holds k) and merged in slice order.  The result is exact.
 *
 * Conventions as xvec_hip.h: DEVICE pointers, asynchronous on the caller's stream, no allocation (the caller passes a workspace
 * of the queried size), return codes as xvec_hip.h (0 = OK) with the message from xvec_ident_last_error().  No float atomics.
 */
#ifndef XVEC_IDENT_H
#define XVEC_IDENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

#define XVEC_IDENT_X_F32 0
#define XVEC_IDENT_X_F64 1
/* a wave walks XVEC_IDENT_COLS columns, a lane each, in slices of XVEC_IDENT_SLICE_ROWS rows */
#define XVEC_IDENT_COLS 64
#define XVEC_IDENT_SLICE_ROWS 32
/* rows of one block of the column statistics (four waves, a slice each) and of the top-k walk (four waves, four slices each) */
#define XVEC_IDENT_BLOCK_ROWS 128
#define XVEC_IDENT_TOPK_BLOCK_ROWS 512
/* xvec_open_set_scores' second pass: a block computes a tile of XVEC_IDENT_APPLY_ROWS x XVEC_IDENT_APPLY_COLS cells */
#define XVEC_IDENT_APPLY_ROWS 8
#define XVEC_IDENT_APPLY_COLS 256
#define XVEC_IDENT_MAX_K 16

const char* xvec_ident_last_error(void);

/* Bytes of workspace for xvec_model_mean with n_models models (0 for a count the entry point refuses). */
size_t xvec_model_mean_workspace_bytes(int32_t n_models);

/* out [n_models, dim] fp64 = the per-model means of x [n, dim] (fp32 or fp64 by x_dtype, row stride ld >= dim elements), the
 * rows of model c being x[order[i]] for model_start_host[c] <= i < model_start_host[c + 1] (order: a permutation of 0 .. n-1,
 * e.g. a stable argsort of the model names; model_start_host: n_models + 1 increasing offsets from 0 to n, on the HOST -- it
 * is checked there and copied into the workspace on the stream; every model owns at least one row).  n < 2^31 (order is
 * int32).  `order` is a device array and is NOT checked: if it is not a permutation of 0 .. n-1 the outputs are undefined (an
 * entry outside [0, n) is never dereferenced, but the results are wrong). */
int xvec_model_mean(const void* x, int32_t x_dtype, int64_t n, int32_t dim, int64_t ld, const int32_t* order,
                    const int64_t* model_start_host, int32_t n_models, double* out, void* workspace, size_t workspace_bytes,
                    xvec_stream stream);

/* Bytes of workspace that hold for xvec_open_set_scores on an [N, T] score matrix and for xvec_identify_topk on it with this k
 * (k == 0: the open-set scores alone).  0 for arguments the entry points refuse. */
size_t xvec_ident_workspace_bytes(int64_t N, int64_t T, int32_t k);

/* out [N, T] (row stride ld_out) from S (row stride ld) as defined above.  2 <= N, 1 <= T, both at most 2^31 - 1;
 * 0 < p_known <= 1.  out may be S itself with ld_out == ld; it must not overlap it otherwise. */
int xvec_open_set_scores(const double* S, int64_t ld, int64_t N, int64_t T, double p_known, double* out, int64_t ld_out,
                         void* workspace, size_t workspace_bytes, xvec_stream stream);

/* idx [k, T] int32 and val [k, T] fp64 (row r = the r-th best model of every column) of S [N, T] (row stride ld), as defined
 * above.  1 <= N, T <= 2^31 - 1; 1 <= k <= XVEC_IDENT_MAX_K (k may exceed N).  decision [T] int32 may be NULL (then threshold
 * is not read). */
int xvec_identify_topk(const double* S, int64_t ld, int64_t N, int64_t T, int32_t k, double threshold, int32_t* idx, double* val,
                       int32_t* decision, void* workspace, size_t workspace_bytes, xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_IDENT_H */
