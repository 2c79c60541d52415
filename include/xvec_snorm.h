/* xvec_snorm.h -- C ABI of score normalisation against a cohort in libxvec_hip.so: Z-, T-, S- and AS-norm.
 *
 * Not in the reference (plda_score_stat.py evaluates raw scores); the step every x-vector system in use puts between scoring
 * and the trial evaluation.  A cohort score matrix S[n, C] is fp64, row-major with row stride ld >= C: what xvec_plda_score* or
 * xvec_cosine_score write for n vectors against C cohort vectors.  For row i:
 *   a cell j is VALID iff S[i,j] is not NaN and j != skip_col[i] (skip_col may be NULL; an entry of -1 skips nothing: it is
 *   there for a vector that is itself a member of the cohort);
 *   v_i = the valid cells, k_i = v_i if top_k == 0, else min(top_k, v_i);
 *   the SELECTION is the k_i largest valid values (-0.0 == +0.0, +-inf are ordinary ordered values; which of several equal
 *   values at the cut is taken cannot matter);
 *   n_used[i] = k_i, kth[i] = the smallest selected value (+0.0 for a zero of either sign),
 *   mean[i] = sum x / k_i, std[i] = sqrt(sum (x - mean)^2 / (k_i - 1)) (unbiased, as torch.std);
 *   k_i < 2: mean, std and kth are NaN.
 * The selection is EXACT: the values are mapped to order-preserving 64-bit keys and the k-th largest key is found by a radix
 * select (eight passes of 8-bit digit histograms in LDS, integer counts); the row is never sorted.  The sums are two passes
 * (sum x, then sum (x - mean)^2) in a fixed order: a row's outputs are a function of that row and C alone, bit-identical
 * whatever n, ld, the base alignment (8 bytes is all that is asked) or the other rows are, and from run to run.
 *
 * Apply: out[i,j] = w (s_ij - mr_i) / sr_i + w (s_ij - mc_j) / sc_j with the row term alone and w = 1 when only the row
 * statistics are given (Z-norm), the column term alone and w = 1 when only the column statistics are (T-norm), both and
 * w = 0.5 when both are (S-norm; AS-norm when the statistics come from top_k < C).  A standard deviation of 0 is NOT clamped:
 * the result is what IEEE 754 gives (+-inf, or NaN for 0 / 0).  Every operation is rounded on its own (no fused multiply-add),
 * so that a symmetric matrix with the same statistics on both sides comes out exactly symmetric.
 *
 * Conventions as xvec_hip.h: DEVICE pointers, asynchronous on the caller's stream, no allocation (the caller passes a workspace
 * of the queried size), return codes as xvec_hip.h (0 = OK) with the message from xvec_snorm_last_error().  No float atomics.
 */
#ifndef XVEC_SNORM_H
#define XVEC_SNORM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

/* A block of XVEC_SNORM_THREADS threads owns a row.  RESIDENT rows are read from memory ONCE and their keys stay in LDS
 * through the select and both sums: up to XVEC_SNORM_RESIDENT_SMALL cells in a 32 KiB image (four blocks per CU), up to
 * XVEC_SNORM_RESIDENT_MAX cells in a 128 KiB image (one block per CU).  STREAMED rows are read again by every pass: rows longer
 * than XVEC_SNORM_RESIDENT_MAX, and with top_k == 0 (three passes instead of ten) rows longer than XVEC_SNORM_RESIDENT_SMALL.
 * The regimes give the same bits for the same row: they differ in speed only. */
#define XVEC_SNORM_THREADS 512
#define XVEC_SNORM_RESIDENT_SMALL 4096
#define XVEC_SNORM_RESIDENT_MAX 16384
/* xvec_snorm_apply: a block computes a tile of XVEC_SNORM_APPLY_ROWS x XVEC_SNORM_APPLY_COLS cells */
#define XVEC_SNORM_APPLY_ROWS 8
#define XVEC_SNORM_APPLY_COLS 256

/* What the select of one row found, left in the workspace (one record per row, row i at workspace + i * 16 bytes) for
 * inspection and tests. */
typedef struct {
    uint64_t cut_key;   /* key of kth[i] (csrc/snorm_keys.h); 0 when k_i == 0 */
    uint32_t n_above;   /* valid cells strictly above the cut: k_i - n_above cells AT the cut are taken */
    uint32_t n_valid;   /* v_i */
} xvec_snorm_select_record;

const char* xvec_snorm_last_error(void);

/* Bytes of workspace for an [n, C] cohort score matrix (0 for a shape the entry points refuse). */
size_t xvec_snorm_workspace_bytes(int64_t n, int64_t C);

/* mean, std, kth [n] fp64 and n_used [n] int32 of the rows of scores [n, C] (row stride ld elements), as defined above.
 * 1 <= n, C <= 2^31 - 1; top_k >= 0; skip_col [n] int32 or NULL. */
int xvec_snorm_row_stats(const double* scores, int64_t ld, int64_t n, int64_t C, int64_t top_k, const int32_t* skip_col,
                         double* mean, double* std, double* kth, int32_t* n_used, void* workspace, size_t workspace_bytes,
                         xvec_stream stream);

/* out [n_rows, n_cols] (row stride ld_out) from scores (row stride ld) and the statistics of the rows (row_mean, row_std
 * [n_rows]) and / or of the columns (col_mean, col_std [n_cols]).  Either pair may be NULL (both members of it), not both
 * pairs.  out may be scores itself with ld_out == ld; it must not overlap it otherwise. */
int xvec_snorm_apply(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const double* row_mean,
                     const double* row_std, const double* col_mean, const double* col_std, double* out, int64_t ld_out,
                     xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_SNORM_H */
