/* xvec_lda.h -- C ABI of embedding conditioning in libxvec_hip.so: LDA statistics, centring, rotation, length norm.
 *
 * The reference reduces its x-vectors with speechbrain's LDA().do_lda(stat, reduced_dim) (reference
 * plda_classifier.py:103-106, called on every split at plda_score_stat.py:207-212); the recipe an x-vector back end
 * normally runs in front of PLDA is centre -> (whiten | LDA) -> length-normalise (speechbrain's StatObject_SB:
 * center_stat1, whiten_stat1, rotate_stat1, norm_stat1, get_lda_matrix_stat1).  That package is not vendored: parity is
 * UNPINNED against it; the arithmetic below is the specification, tests/lda_ref.py restates it in numpy float64 and the
 * package's xvector_amd.lda is checked against that restatement.
 *
 * What scales with the number of vectors runs here, in fp64 arithmetic on v_mfma_f64_16x16x4_f64:
 *   xvec_lda_stats        once per training set: the mean, the class means, the class-weighted within-class scatter
 *                         and the between-class scatter;
 *   xvec_embed_transform  once per set of vectors: y = (x - mean) W, optionally with every row scaled to unit length.
 * The model-sized eigenproblem (D x D) stays on the host.
 *
 * Conventions as xvec_plda.h: DEVICE pointers unless the name ends in _host, row-major, fp64 outputs, asynchronous on
 * the caller's stream, no allocation (the caller passes a workspace of the queried size), return codes as xvec_hip.h
 * (0 = OK) with the message from xvec_lda_last_error(), argument checks before any device work.  Every sum runs in a
 * fixed order with no float atomics: repeat calls on the same inputs give bit-identical outputs.
 */
#ifndef XVEC_LDA_H
#define XVEC_LDA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

enum { XVEC_LDA_X_F32 = 0, XVEC_LDA_X_F64 = 1 }; /* = XVEC_PLDA_X_* */

/* Largest dim of xvec_embed_transform (rank <= dim).  The kernels stream dim in chunks of 16, so nothing of theirs grows
 * with it; the bound keeps every row offset of W far inside 32 bits of tile arithmetic.  The pooled statistics are 3000. */
#define XVEC_EMBED_MAX_DIM 65536
/* Rows one block of xvec_embed_transform owns (it sweeps every column tile of them and rescales what it wrote). */
#define XVEC_EMBED_ROW_GROUP 64

const char* xvec_lda_last_error(void);

/* Scratch of xvec_lda_stats (0 for arguments it would refuse). */
size_t xvec_lda_stats_workspace_bytes(int64_t n, int32_t dim, int32_t n_classes);

/* x [n, dim] (fp32 or fp64 by x_dtype), `order` and `class_start_host` as in xvec_plda_stats (the rows of class c are
 * x[order[i]] for class_start_host[c] <= i < class_start_host[c + 1]; class_start_host is on the HOST, checked there and
 * copied into the workspace on the stream) -- with one difference: every class must have at least one row, i.e.
 * class_start_host must be STRICTLY increasing from 0 to n; anything else is refused.  With n_c the rows of class c:
 *   mean[dim]                 = sum of all rows / n
 *   class_means[C, dim]       m_c = sum of the class's rows / n_c
 *   s_within[dim, dim]        = sum_c (1 / n_c) sum_{i in c} (x_i - m_c)(x_i - m_c)^T   (each class's biased covariance,
 *                               summed: speechbrain's definition, not the pooled scatter of xvec_plda_stats)
 *   s_between[dim, dim]       = sum_c (m_c - mean)(m_c - mean)^T
 * Both matrices are exactly symmetric (the upper triangle of tiles is computed and mirrored).  The rows are centred by
 * class_means, and the class means by mean, before the products: a large common offset in x costs s_within no digits.
 * 1 <= n_classes <= n < 2^31 (order is int32).  `order` is a device array and is NOT checked: if it is not a permutation
 * of 0 .. n-1 the outputs are undefined (an entry outside [0, n) is never dereferenced, but the results are wrong). */
int xvec_lda_stats(const void* x, int32_t x_dtype, int64_t n, int32_t dim, const int32_t* order,
                   const int64_t* class_start_host, int32_t n_classes, double* mean, double* class_means,
                   double* s_within, double* s_between, void* workspace, size_t workspace_bytes, xvec_stream stream);

/* Scratch of xvec_embed_transform (0 for arguments it would refuse): the clipped row norms. */
size_t xvec_embed_transform_workspace_bytes(int64_t n, int32_t dim, int32_t rank);

/* y[i, :] = (x[i, :] - mean) W for x [n, dim] (fp32 or fp64, row stride ldx elements), mean [dim] fp64, W [dim, rank]
 * row-major fp64, y [n, rank] fp64 (row stride ldy elements); if normalize != 0 then y[i, :] /= max(||y[i, :]||_2, 1e-8)
 * (speechbrain's norm_stat1 clip: an all-zero row stays all-zero).
 *   mean == NULL   no centring
 *   w == NULL      the identity: requires rank == dim; a pure centre / length-norm pass without a product
 * 1 <= rank <= dim <= XVEC_EMBED_MAX_DIM, 1 <= n < 2^31, ldx >= dim, ldy >= rank.  y must not overlap x: refused where the two
 * address ranges show it.  Only the n x rank cells of y are written (padding columns of a wider ldy stay untouched). */
int xvec_embed_transform(const void* x, int32_t x_dtype, int64_t n, int32_t dim, int64_t ldx, const double* mean,
                         const double* w, int32_t rank, int32_t normalize, double* y, int64_t ldy, void* workspace,
                         size_t workspace_bytes, xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_LDA_H */
