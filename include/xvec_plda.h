/* xvec_plda.h -- C ABI of PLDA model training in libxvec_hip.so.
 *
 * The reference trains its PLDA model with speechbrain's PLDA.plda(stat) (reference
 * main.py:271-310, plda_classifier.py:51-57) in numpy float64.  That package is not vendored:
 * parity is UNPINNED against it; tests/plda_em_ref.py restates its EM loop and the package's
 * training (xvector_amd.plda) is checked against that restatement.
 *
 * What scales with the number of training vectors runs here, in fp64 arithmetic:
 *   xvec_plda_stats        once per training set: the mean, the class counts, the centred class
 *                          sums and the centred scatter matrix (v_mfma_f64_16x16x4_f64);
 *   xvec_plda_em_products  once per EM iteration: the class-scale products of the E-step.
 * The model-sized factorizations (eigh, Cholesky, solve; D x D and R x R) stay on the host.
 *
 * Conventions as xvec_hip.h: DEVICE pointers unless the name ends in _host, row-major, fp64
 * outputs, asynchronous on the caller's stream, no allocation (the caller passes a workspace of
 * the queried size), return codes as xvec_hip.h (0 = OK) with the message from
 * xvec_plda_last_error().  Every sum runs in a fixed order with no float atomics: repeat calls
 * on the same inputs give bit-identical outputs.
 */
#ifndef XVEC_PLDA_H
#define XVEC_PLDA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

enum { XVEC_PLDA_X_F32 = 0, XVEC_PLDA_X_F64 = 1 };

const char* xvec_plda_last_error(void);

/* Scratch of xvec_plda_stats (0 for arguments it would refuse). */
size_t xvec_plda_stats_workspace_bytes(int64_t n, int32_t dim, int32_t n_classes);

/* x [n, dim] (fp32 or fp64 by x_dtype), the rows of class c being x[order[i]] for
 * class_start_host[c] <= i < class_start_host[c + 1] (order: a permutation of 0 .. n-1, e.g. a stable
 * argsort of the class ids; class_start_host: n_classes + 1 non-decreasing offsets from 0 to n, on the
 * HOST -- it is checked there and copied into the workspace on the stream).  Outputs:
 *   mean[dim]                     = sum of all rows / n
 *   counts[n_classes]             = scaling_factor * rows of the class
 *   class_sums[n_classes, dim]    = scaling_factor * (sum of the class's rows) - counts[c] * mean
 *   class_sums_t[dim, n_classes]  = its transpose (may be NULL)
 *   sigma_obs[dim, dim]           = (x - mean)^T (x - mean) / n, exactly symmetric
 * n < 2^31 (order is int32).  `order` is a device array and is NOT checked: if it is not a permutation of
 * 0 .. n-1 the outputs are undefined (an entry outside [0, n) is never dereferenced, but the results are wrong). */
int xvec_plda_stats(const void* x, int32_t x_dtype, int64_t n, int32_t dim, const int32_t* order,
                    const int64_t* class_start_host, int32_t n_classes, double scaling_factor, double* mean,
                    double* counts, double* class_sums, double* class_sums_t, double* sigma_obs, void* workspace,
                    size_t workspace_bytes, xvec_stream stream);

/* Scratch of xvec_plda_em_products (0 for arguments it would refuse). */
size_t xvec_plda_em_workspace_bytes(int32_t n_classes, int32_t rank);

/* One E-step's class-scale products.  With S = class_sums [C, dim], n = counts [C], pq_t [rank, dim]
 * (= (Sigma^-1 F Q)^T, Q the eigenvectors and lam [rank] the eigenvalues of F^T Sigma^-1 F) and
 *   H[c, k] = (S pq_t^T)[c, k] / (n[c] lam[k] + 1)
 * out [rank, 2 rank + dim] receives [ H^T H | H^T diag(n) H | H^T S ].  rank <= dim. */
int xvec_plda_em_products(const double* pq_t, const double* class_sums, const double* class_sums_t,
                          const double* counts, const double* lam, int32_t n_classes, int32_t dim, int32_t rank,
                          double* out, void* workspace, size_t workspace_bytes, xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_PLDA_H */
