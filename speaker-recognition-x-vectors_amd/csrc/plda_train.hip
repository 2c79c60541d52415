// PLDA training: the N-scale statistics and the per-iteration class-scale products, fp64.
//   reference: main.py:271-310 -> speechbrain 0.5.12 PLDA.plda(stat) (numpy float64)
// C ABI: include/xvec_plda.h.  The EM loop itself (eigh / Cholesky / solve of D x D and R x R matrices) runs on the host,
// xvector_amd.plda.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

#include "../../include/xvec_hip.h"
#include "../../include/xvec_plda.h"
#include "../../include/xvec_score.h"
#include "host_support.h"
#include "tdnn_common.h"

namespace xvec {
namespace {

#include "class_scatter.h"      // inside the anonymous namespace: this file's own instances of the shared statistics kernels

// ---------------------------------------------------------------- class sums, centring

// One block per class: sums[c, :] = sum of the class's rows in `order` order (class_sum_columns), counts[c] = scaling * rows; a
// row of `order` outside [0, n) is still counted.
template <typename T>
__global__ __launch_bounds__(256) void plda_class_sum_kernel(const T* __restrict__ x, int64_t n, int dim,
                                                             const int* __restrict__ order,
                                                             const int64_t* __restrict__ cstart, double scaling,
                                                             double* __restrict__ sums, double* __restrict__ counts) {
    const int c = blockIdx.x;
    int64_t b, e;
    class_rows(cstart, c, n, b, e);
    if (threadIdx.x == 0) counts[c] = scaling * (double)(e - b);
    class_sum_columns(x, n, dim, order, c, b, e, sums);
}

// sums[c, d] <- scaling * sums[c, d] - counts[c] * mean[d] (counts already scaled), and its transpose
__global__ __launch_bounds__(256) void plda_centre_kernel(double* __restrict__ sums, double* __restrict__ sums_t,
                                                          const double* __restrict__ counts,
                                                          const double* __restrict__ mean, int n_classes, int dim,
                                                          double scaling) {
    const int64_t idx = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (idx >= (int64_t)n_classes * dim) return;
    const int c = (int)(idx / dim), d = (int)(idx - (int64_t)c * dim);
    const double v = scaling * sums[idx] - counts[c] * mean[d];
    sums[idx] = v;
    if (sums_t) sums_t[(int64_t)d * n_classes + c] = v;
}

// ---------------------------------------------------------------- E-step scaling

// yt [rank, C] -> hh [2 rank, C]: rows k = yt[k, c] / (n[c] lam[k] + 1), rows rank + k = n[c] times that
__global__ __launch_bounds__(256) void plda_em_scale_kernel(const double* __restrict__ yt, const double* __restrict__ counts,
                                                            const double* __restrict__ lam, int rank, int n_classes,
                                                            double* __restrict__ hh) {
    const int64_t idx = blockIdx.x * (int64_t)256 + threadIdx.x;
    const int64_t total = (int64_t)rank * n_classes;
    if (idx >= total) return;
    const int k = (int)(idx / n_classes), c = (int)(idx - (int64_t)k * n_classes);
    const double h = yt[idx] / (counts[c] * lam[k] + 1.0);
    hh[idx] = h;
    hh[total + idx] = counts[c] * h;
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_perr;

constexpr int kSliceRows = 256;        // a slice is worth opening for this many rows

struct StatsPlan {
    int tiles, n_tri;
    ScatterPlan scatter;
    int64_t* cstart;      // device copy of class_start
    double* slab;         // scatter partials, one kTS x kTS tile per (slice, triangle tile)
    size_t total;
};

StatsPlan make_stats_plan(void* ws, int64_t n, int dim, int n_classes) {
    StatsPlan p{};
    p.tiles = (dim + kTS - 1) / kTS;
    p.n_tri = p.tiles * (p.tiles + 1) / 2;
    p.scatter = make_scatter_plan(n, p.n_tri, kSliceRows);
    Carver c(ws);
    p.cstart = c.take<int64_t>((size_t)n_classes + 1);
    p.slab = c.take<double>((size_t)p.scatter.slices * p.n_tri * kTS * kTS);
    p.total = c.total();
    return p;
}

struct EmPlan {
    double *yt, *hh;      // Y^T [rank, C];  [H^T ; (n H)^T] [2 rank, C]
    size_t total;
};

EmPlan make_em_plan(void* ws, int n_classes, int rank) {
    EmPlan p{};
    Carver c(ws);
    p.yt = c.take<double>((size_t)rank * n_classes);
    p.hh = c.take<double>((size_t)2 * rank * n_classes);
    p.total = c.total();
    return p;
}

// one product through the public scorer entry; its message moves into this module's channel
int product(const char* what, const double* A, int64_t lda, const double* B, int64_t ldb, int64_t M, int64_t N, int K, double* C,
            int64_t ldc, xvec_stream stream) {
    const int rc = xvec_gemm_nt_f64(A, lda, B, ldb, M, N, K, nullptr, nullptr, 0.0, 1.0, C, ldc, stream);
    return rc ? g_perr.fail(rc, "%s: %s", what, xvec_score_last_error()) : XVEC_OK;
}

bool stats_args_ok(int64_t n, int dim, int n_classes) {
    return n >= 2 && n <= 0x7fffffff && dim >= 1 && n_classes >= 1 && n_classes <= n;
}

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_plda_last_error(void) { return g_perr.c_str(); }

size_t xvec_plda_stats_workspace_bytes(int64_t n, int32_t dim, int32_t n_classes) {
    if (!stats_args_ok(n, dim, n_classes)) return 0;
    return make_stats_plan(nullptr, n, dim, n_classes).total;
}

// Launches: class sums (one block per class), mean, centring (+ transpose), scatter partials, scatter reduce.
int xvec_plda_stats(const void* x, int32_t x_dtype, int64_t n, int32_t dim, const int32_t* order,
                    const int64_t* class_start_host, int32_t n_classes, double scaling_factor, double* mean,
                    double* counts, double* class_sums, double* class_sums_t, double* sigma_obs, void* workspace,
                    size_t workspace_bytes, xvec_stream stream) {
    if (n < 2) return g_perr.fail(XVEC_ERR_ARG, "need at least two training vectors (n = %lld)", (long long)n);
    if (n > 0x7fffffff) return g_perr.fail(XVEC_ERR_TOO_LARGE, "n = %lld: row indices are int32", (long long)n);
    if (dim < 1 || n_classes < 1) return g_perr.fail(XVEC_ERR_ARG, "dim = %d and n_classes = %d must be >= 1", dim, n_classes);
    if (n_classes > n) return g_perr.fail(XVEC_ERR_ARG, "more classes (%d) than vectors (%lld)", n_classes, (long long)n);
    if (x_dtype != XVEC_PLDA_X_F32 && x_dtype != XVEC_PLDA_X_F64) return g_perr.fail(XVEC_ERR_ARG, "x_dtype %d unknown", x_dtype);
    if (!x || !order || !class_start_host || !mean || !counts || !class_sums || !sigma_obs || !workspace)
        return g_perr.fail(XVEC_ERR_ARG, "null pointer");
    int rc;
    if ((rc = class_start_spans(class_start_host, n_classes, n, g_perr))) return rc;
    if (const int c = first_short_class(class_start_host, n_classes, 0); c >= 0)
        return g_perr.fail(XVEC_ERR_ARG, "class_start decreases at class %d", c);
    const StatsPlan p = make_stats_plan(workspace, n, dim, n_classes);
    if ((rc = workspace_ok(workspace_bytes, p.total, g_perr))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((rc = upload_class_start(p.cstart, class_start_host, n_classes, s, g_perr))) return rc;
    if (x_dtype == XVEC_PLDA_X_F32)
        plda_class_sum_kernel<float><<<n_classes, 256, 0, s>>>(static_cast<const float*>(x), n, dim, order, p.cstart,
                                                                scaling_factor, class_sums, counts);
    else
        plda_class_sum_kernel<double><<<n_classes, 256, 0, s>>>(static_cast<const double*>(x), n, dim, order, p.cstart,
                                                                 scaling_factor, class_sums, counts);
    if ((rc = g_perr.launch_ok("plda_class_sum_kernel"))) return rc;
    stats_mean_kernel<<<(dim + kMeanCols - 1) / kMeanCols, 256, 0, s>>>(class_sums, n_classes, dim, n, mean);
    if ((rc = g_perr.launch_ok("stats_mean_kernel"))) return rc;
    const int64_t cd = (int64_t)n_classes * dim;
    plda_centre_kernel<<<(unsigned)((cd + 255) / 256), 256, 0, s>>>(class_sums, class_sums_t, counts, mean, n_classes, dim,
                                                                   scaling_factor);
    if ((rc = g_perr.launch_ok("plda_centre_kernel"))) return rc;
    // sigma_obs: every row of x in storage order, centred by the mean, over n
    ScatterArgs g{};
    g.x = x;
    g.centre = mean;
    g.slab = p.slab;
    g.n = n;
    g.dim = dim;
    g.tiles = p.tiles;
    g.n_tri = p.n_tri;
    return launch_scatter<false>(g, x_dtype == XVEC_PLDA_X_F32, p.scatter, (double)n, sigma_obs, s, g_perr);
}

size_t xvec_plda_em_workspace_bytes(int32_t n_classes, int32_t rank) {
    if (n_classes < 1 || rank < 1) return 0;
    return make_em_plan(nullptr, n_classes, rank).total;
}

// Launches: Y^T = pq_t S^T (xvec_gemm_nt_f64), the scaling into [H^T ; (n H)^T], then [H^T H | H^T diag(n) H] and H^T S
// (two more products into the column blocks of `out`).
int xvec_plda_em_products(const double* pq_t, const double* class_sums, const double* class_sums_t,
                          const double* counts, const double* lam, int32_t n_classes, int32_t dim, int32_t rank,
                          double* out, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    if (n_classes < 1 || dim < 1 || rank < 1)
        return g_perr.fail(XVEC_ERR_ARG, "n_classes = %d, dim = %d and rank = %d must be >= 1", n_classes, dim, rank);
    if (rank > dim) return g_perr.fail(XVEC_ERR_ARG, "rank_f = %d exceeds dim = %d", rank, dim);
    if (!pq_t || !class_sums || !class_sums_t || !counts || !lam || !out || !workspace)
        return g_perr.fail(XVEC_ERR_ARG, "null pointer");
    const EmPlan p = make_em_plan(workspace, n_classes, rank);
    int rc;
    if ((rc = workspace_ok(workspace_bytes, p.total, g_perr))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t C = n_classes, R = rank, ldo = 2 * R + dim;
    if ((rc = product("Y product", pq_t, dim, class_sums, dim, R, C, dim, p.yt, C, stream))) return rc;
    const int64_t rc_total = R * C;
    plda_em_scale_kernel<<<(unsigned)((rc_total + 255) / 256), 256, 0, s>>>(p.yt, counts, lam, rank, n_classes, p.hh);
    if ((rc = g_perr.launch_ok("plda_em_scale_kernel"))) return rc;
    if ((rc = product("H products", p.hh, C, p.hh, C, R, 2 * R, n_classes, out, ldo, stream))) return rc;
    return product("H^T S product", p.hh, C, class_sums_t, C, R, dim, n_classes, out + 2 * R, ldo, stream);
}

}  // extern "C"
