/* xvec_tsne.h -- C ABI of exact t-SNE in libxvec_hip.so: what the reference's plot_images (plda_score_stat.py) needs computed
 * for its TSNE scatter plot, without the plotting.
 *
 * The reference calls sklearn.manifold.TSNE(2), which is Barnes-Hut: an approximation chosen because the exact method costs
 * N^2 per iteration on a CPU.  On the device the exact method is an N^2 pass over a matrix that stays in HBM, so that is what
 * runs here: scikit-learn's method='exact' (1.7: _joint_probabilities, _kl_divergence, _gradient_descent with
 * degrees_of_freedom = 1), restated in tests/tsne_ref.py and pinned by a fixture written from scikit-learn itself
 * (tests/golden/g11_tsne.npz).
 *
 * Three steps, all fp64, row-major, strides in elements:
 *
 * xvec_tsne_sqdist.  D2[i, j] = max((-2 x_i.x_j + |x_i|^2) + |x_j|^2, 0), D2[i, i] = 0: scikit-learn's
 * euclidean_distances(squared=True).  The rows are widened to fp64 (fp32 input is exact in it), the Gram matrix is one
 * xvec_gemm_nt_f64 product, |x_i|^2 is the sum of the squares by lane (lane l adds columns l, l + 64, ... ascending from 0.0,
 * then for stride = 32, 16, ..., 1: lane[l] += lane[l ^ stride]).  With round_f32 every distance is rounded to float32 and
 * widened again: scikit-learn does that before its perplexity search, and only with it does an fp64 search reproduce
 * scikit-learn's P to rounding (without: 1e-7 .. 1e-5 of difference).
 *
 * xvec_tsne_affinities.  Row i runs _binary_search_perplexity on D2[i, :] (j != i): beta = 1; at most 100 steps of
 *   e_j = exp(-D2[i, j] * beta);  S = sum e_j, and S = (double)1e-8f if S == 0;  H = log(S) + beta * (sum D2[i, j] e_j) / S
 *   stop if |H - log(perplexity)| <= (double)1e-5f;  H too large: beta doubles, or bisects towards the upper bracket once there
 *   is one; else: beta halves, or bisects towards the lower bracket.
 * (The two constants are scikit-learn's `cdef float`s, hence the float32 values.)  C[i, j] = e_j / S at the last beta that was
 * evaluated (betas[i], optional), C[i, i] = 0.  Then P[i, j] = max((C[i, j] + C[j, i]) / max(2 sum C, eps), eps) off the
 * diagonal and 0 on it, eps = DBL_EPSILON.  A row's sums: thread t of 256 adds columns t, t + 256, ... ascending, the 64 lanes
 * of a wave combine as above, the four waves are added in order.  sum C adds the rows' sums the same way (rows for columns).
 *
 * xvec_tsne_steps.  n_steps iterations of _gradient_descent on _kl_divergence.  With w_ij = 1 / (1 + |y_i - y_j|^2), j != i:
 *   attraction_i = sum_j (exaggeration P_ij) w_ij (y_i - y_j);  repulsion_i = sum_j w_ij^2 (y_i - y_j);  Z = sum_i sum_j w_ij
 *   grad_i = 4 (attraction_i - repulsion_i / Z)
 *   gains += 0.2 where update * grad < 0, else gains *= 0.8; gains = max(gains, min_gain)
 *   update = momentum update - learning_rate (gains grad);  y += update
 * An iteration is two launches.  The pair pass gives a block a group of rows and a slice of the columns (xvec_tsne_plan); the
 * slice's y sits in LDS, P is read once.  Within a (row, slice) lane l of the row's wave adds the slice's columns 2l, 2l + 1,
 * 2l + 128, 2l + 129, ... ascending, the lanes combine as above, and the five sums go to the workspace as [slice][row][5].  The
 * update adds a row's slices in order; Z adds the rows' sums as sum C above.  Every sum has a fixed order that depends on n
 * and the plan alone: a call is bit-identical from run to run, whatever the strides, the alignment of P and the workspace's
 * previous contents are, and step(10) is ten step(1).
 * DEVIATION.  scikit-learn floors Q_ij = w_ij / Z at eps before it subtracts it from P_ij.  Z is not known during the pair pass,
 * so the gradient here does not: the two differ only where w_ij / Z < 2.2e-16 (|y_i - y_j| around 1e8 / sqrt(Z)).
 * kl_out (optional): the KL divergence of the y that ENTERED the last of the n_steps iterations, what scikit-learn reports at a
 * check iteration: 2 sum_{i<j} cP log(max(cP, eps) / max(w_ij / Z, eps)), cP = exaggeration P_ij, the floor kept.  It is one
 * more pass over P in that iteration (and two small launches).  grad_norm_out (optional): the 2-norm of that iteration's grad,
 * BEFORE the gains are applied (scikit-learn takes it after; its min_grad_norm stop is compared against this one here).
 *
 * Conventions as xvec_diar.h: DEVICE pointers (8-byte aligned), asynchronous on the caller's stream, graph-capturable, no
 * allocation (the caller passes a workspace of the queried size, whose previous contents never matter), no block waits on
 * another, no float atomics, no grid-wide barrier: stream order between launches is the only one.  Return codes as xvec_hip.h
 * (0 = OK) with the message from xvec_tsne_last_error(), a channel of its own, per thread.  Argument errors return
 * XVEC_ERR_ARG (a small workspace XVEC_ERR_WORKSPACE) before the device is touched.
 */
#ifndef XVEC_TSNE_H
#define XVEC_TSNE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

/* points at most: a dense P is then 512 MiB */
#define XVEC_TSNE_MAX_POINTS 8192
/* columns of x at most */
#define XVEC_TSNE_MAX_DIM 65536
/* threads of every block; distances a thread of the affinity kernel keeps in registers, at most */
#define XVEC_TSNE_THREADS 256
#define XVEC_TSNE_ROW_ITEMS 32
/* columns of a slice of the pair pass: a multiple of XVEC_TSNE_SLICE_STEP, at most XVEC_TSNE_SLICE_MAX (32 KiB of y in LDS) */
#define XVEC_TSNE_SLICE_STEP 128
#define XVEC_TSNE_SLICE_MAX 2048
/* rows of a block of the pair pass, at most (a power of two; four waves share them) */
#define XVEC_TSNE_ROWS_MAX 16
#define XVEC_TSNE_ROWS_MIN 4
/* steps of the perplexity search */
#define XVEC_TSNE_SEARCH_STEPS 100

#define XVEC_TSNE_X_F32 0
#define XVEC_TSNE_X_F64 1

const char* xvec_tsne_last_error(void);

/* Bytes of workspace for n points: enough for every call below, with x of d columns (d = 0: xvec_tsne_sqdist is not called).
 * 0 for arguments the calls would refuse. */
size_t xvec_tsne_workspace_bytes(int32_t n, int32_t d);

/* The pair pass's plan for n points on a device of `cus` compute units (cus < 1: the current device's): rows of a block,
 * slices of the columns, columns of a slice (the last one may be shorter). */
int xvec_tsne_plan(int32_t n, int32_t cus, int32_t* rows_per_block, int32_t* slices, int32_t* slice_cols);

/* x [n, d] fp32 or fp64 (x_dtype), row stride ldx >= d; d2 [n, n], row stride ldd >= n.  d2 must not overlap x. */
int xvec_tsne_sqdist(const void* x, int32_t x_dtype, int32_t n, int32_t d, int64_t ldx, int32_t round_f32, double* d2,
                     int64_t ldd, void* workspace, size_t workspace_bytes, xvec_stream stream);

/* d2 [n, n] (row stride ldd) -> p [n, n] (row stride ldp); 0 < perplexity < n, finite.  betas [n] may be NULL.  p must not
 * overlap d2. */
int xvec_tsne_affinities(const double* d2, int64_t ldd, int32_t n, double perplexity, double* p, int64_t ldp, double* betas,
                         void* workspace, size_t workspace_bytes, xvec_stream stream);

/* p [n, n] (row stride ldp, read only); y, update, gains [n, 2] (one row stride ldy >= 2 for the three), updated in place.
 * n_components must be 2, n_steps at least 1.  kl_out and grad_norm_out (one double each, on the device) may be NULL. */
int xvec_tsne_steps(const double* p, int64_t ldp, int32_t n, int32_t n_components, double* y, double* update, double* gains,
                    int64_t ldy, int32_t n_steps, double exaggeration, double momentum, double learning_rate, double min_gain,
                    double* kl_out, double* grad_norm_out, void* workspace, size_t workspace_bytes, xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_TSNE_H */
