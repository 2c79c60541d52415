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

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- class sums, mean, centring

// One block per class: sums[c, :] = sum of the class's rows in `order` order (four interleaved partial sums per column,
// combined in a fixed order), counts[c] = scaling * rows.  `order` must be a permutation of 0 .. n-1 (the ABI cannot check a
// device array; include/xvec_plda.h): an index outside [0, n) is only kept from reading out of bounds -- it adds nothing
// while still being counted, and the outputs are undefined.
template <typename T>
__global__ __launch_bounds__(256) void plda_class_sum_kernel(const T* __restrict__ x, int64_t n, int dim,
                                                             const int* __restrict__ order,
                                                             const int64_t* __restrict__ cstart, double scaling,
                                                             double* __restrict__ sums, double* __restrict__ counts) {
    const int c = blockIdx.x;
    const int64_t b = std::min<int64_t>(std::max<int64_t>(cstart[c], 0), n);
    const int64_t e = std::min<int64_t>(std::max<int64_t>(cstart[c + 1], b), n);
    if (threadIdx.x == 0) counts[c] = scaling * (double)(e - b);
    auto at = [&](int r, int d) -> double { return (r >= 0 && r < n) ? (double)x[(int64_t)r * dim + d] : 0.0; };
    for (int d = threadIdx.x; d < dim; d += 256) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int64_t i = b;
        for (; i + 4 <= e; i += 4) {
            const int r0 = order[i], r1 = order[i + 1], r2 = order[i + 2], r3 = order[i + 3];
            a0 += at(r0, d);
            a1 += at(r1, d);
            a2 += at(r2, d);
            a3 += at(r3, d);
        }
        for (; i < e; ++i) a0 += at(order[i], d);
        sums[(int64_t)c * dim + d] = (a0 + a1) + (a2 + a3);
    }
}

// mean[d] = (sum of the raw class sums) / n.  A block takes 16 columns; its 16 groups of 16 threads sum the classes
// c = g, g + 16, g + 32, .. of their column, and thread g = 0 adds the 16 group partials in group order (fixed order).
constexpr int kMeanCols = 16, kMeanGroups = 16;
__global__ __launch_bounds__(256) void plda_mean_kernel(const double* __restrict__ sums, int n_classes, int dim,
                                                        int64_t n, double* __restrict__ mean) {
    __shared__ double part[kMeanGroups][kMeanCols];
    const int col = threadIdx.x % kMeanCols, grp = threadIdx.x / kMeanCols;
    const int d = blockIdx.x * kMeanCols + col;
    double s = 0.0;
    if (d < dim) {
#pragma unroll 4
        for (int c = grp; c < n_classes; c += kMeanGroups) s += sums[(int64_t)c * dim + d];
    }
    part[grp][col] = s;
    __syncthreads();
    if (grp == 0 && d < dim) {
        double t = part[0][col];
        for (int g = 1; g < kMeanGroups; ++g) t += part[g][col];
        mean[d] = t / (double)n;
    }
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

// ---------------------------------------------------------------- centred scatter matrix

// (x - mean)^T (x - mean) over the tiles on or above the diagonal of a (64 x 64)-tiled [dim, dim] grid, K split over rows:
// block = (row slice, tile); it writes its 64 x 64 partial to slab[slice][tile].  A second launch sums the slices in order
// and mirrors the result.  4 waves as 2 x 2, each 32 x 32 = 2 x 2 tiles of v_mfma_f64_16x16x4_f64 (A[i][k] = x[k][i]: both
// operands are read from row-major [k][column] LDS images, lane l takes k = l >> 4, column l & 15).  Rows in chunks of 16
// through double-buffered LDS; the next chunk's global loads fly while the current one's 16 MFMAs per wave run.
constexpr int kTS = 64;        // tile edge
constexpr int kKC = 16;        // rows per chunk
constexpr int kLD = 80;        // LDS row stride in doubles (640 B): the four k rows of one ds_read_b64 land 128 B apart in the banks
constexpr int kScatterBlocks = 1024;   // slices x tiles aimed at: four blocks per CU on 256 CUs (fixed: results do not depend on the device)

struct ScatterArgs {
    const void* x;
    const double* mean;
    double* slab;
    int64_t n, rows_per_slice;
    int dim, tiles, n_tri;
};

// tile t of the row-major upper triangle of a T x T grid -> (row, column)
__device__ __forceinline__ void tri_rc(int t, int T, int& r, int& c) {
    int r0 = 0;
    while (t >= T - r0) {
        t -= T - r0;
        ++r0;
    }
    r = r0;
    c = r0 + t;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256, 4) void plda_scatter_kernel(const ScatterArgs g) {
    __shared__ __attribute__((aligned(16))) double sA[2][kKC][kLD];
    __shared__ __attribute__((aligned(16))) double sB[2][kKC][kLD];
    const int logical = xcd_remap(blockIdx.x, gridDim.x);       // the tiles of one slice share an XCD's L2
    const int tile = logical % g.n_tri, slice = logical / g.n_tri;
    int tr, tc;
    tri_rc(tile, g.tiles, tr, tc);
    const bool diag = tr == tc;                                 // A == B: one operand staged
    const int i0 = tr * kTS, j0 = tc * kTS;
    const int64_t row_begin = (int64_t)slice * g.rows_per_slice;
    const int64_t row_end = std::min<int64_t>(g.n, row_begin + g.rows_per_slice);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    const int lrow = tid >> 4, lcol = (tid & 15) * 4;            // staging: 16 rows x 64 columns, four columns a thread
    const T* __restrict__ x = static_cast<const T*>(g.x);

    bool va[4], vb[4];
    double ma[4], mb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        va[q] = i0 + lcol + q < g.dim;
        vb[q] = j0 + lcol + q < g.dim;
        ma[q] = va[q] ? g.mean[i0 + lcol + q] : 0.0;
        mb[q] = vb[q] ? g.mean[j0 + lcol + q] : 0.0;
    }
    T ra[4], rb[4];
    bool rvalid = false;
    auto gload = [&](int64_t r0) {
        const int64_t row = r0 + lrow;
        rvalid = row < row_end;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ra[q] = T(0);
            rb[q] = T(0);
        }
        if (!rvalid) return;
        const T* p = x + row * g.dim;
        if constexpr (VEC) {            // dim % 4 == 0, 16-byte aligned base: the four columns are all in or all out
            if (va[0]) {
                if constexpr (sizeof(T) == 4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(p + i0 + lcol);
                    ra[0] = v.x; ra[1] = v.y; ra[2] = v.z; ra[3] = v.w;
                } else {
                    const f64x2 v0 = *reinterpret_cast<const f64x2*>(p + i0 + lcol);
                    const f64x2 v1 = *reinterpret_cast<const f64x2*>(p + i0 + lcol + 2);
                    ra[0] = v0.x; ra[1] = v0.y; ra[2] = v1.x; ra[3] = v1.y;
                }
            }
            if (!diag && vb[0]) {
                if constexpr (sizeof(T) == 4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(p + j0 + lcol);
                    rb[0] = v.x; rb[1] = v.y; rb[2] = v.z; rb[3] = v.w;
                } else {
                    const f64x2 v0 = *reinterpret_cast<const f64x2*>(p + j0 + lcol);
                    const f64x2 v1 = *reinterpret_cast<const f64x2*>(p + j0 + lcol + 2);
                    rb[0] = v0.x; rb[1] = v0.y; rb[2] = v1.x; rb[3] = v1.y;
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (va[q]) ra[q] = p[i0 + lcol + q];
                if (!diag && vb[q]) rb[q] = p[j0 + lcol + q];
            }
        }
    };
    // centring while staged; rows past the slice and columns past dim stay exactly zero
    auto lstore = [&](int buf) {
        double a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a[q] = rvalid && va[q] ? (double)ra[q] - ma[q] : 0.0;
            b[q] = rvalid && vb[q] ? (double)rb[q] - mb[q] : 0.0;
        }
        *reinterpret_cast<f64x2*>(&sA[buf][lrow][lcol]) = f64x2{a[0], a[1]};
        *reinterpret_cast<f64x2*>(&sA[buf][lrow][lcol + 2]) = f64x2{a[2], a[3]};
        if (!diag) {
            *reinterpret_cast<f64x2*>(&sB[buf][lrow][lcol]) = f64x2{b[0], b[1]};
            *reinterpret_cast<f64x2*>(&sB[buf][lrow][lcol + 2]) = f64x2{b[2], b[3]};
        }
    };

    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

    const int64_t rows = std::max<int64_t>(row_end - row_begin, 0);
    const int64_t n_chunks = (rows + kKC - 1) / kKC;
    if (n_chunks > 0) {
        gload(row_begin);
        lstore(0);
        __syncthreads();
    }
    for (int64_t ch = 0; ch < n_chunks; ++ch) {
        const int buf = (int)(ch & 1);
        if (ch + 1 < n_chunks) gload(row_begin + (ch + 1) * kKC);
        const double(*opB)[kLD] = diag ? sA[buf] : sB[buf];
#pragma unroll
        for (int ks = 0; ks < kKC / 4; ++ks) {
            const int k = ks * 4 + l4;
            double a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = sA[buf][k][wr * 32 + i * 16 + l15];
                b[i] = opB[k][wc * 32 + i * 16 + l15];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (ch + 1 < n_chunks) lstore(buf ^ 1);
        __syncthreads();
    }

    // C/D of the f64 MFMA: column lane & 15, row (lane >> 4) + 4 reg; 16 lanes write 128 contiguous bytes
    double* out = g.slab + ((size_t)slice * g.n_tri + tile) * (kTS * kTS);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                out[(wr * 32 + i * 16 + l4 + 4 * r) * kTS + wc * 32 + j * 16 + l15] = acc[i][j][r];
}

// sigma[i, j] = sigma[j, i] = (sum over slices, in slice order, of the partials of (i, j), i <= j) / n
__global__ __launch_bounds__(256) void plda_scatter_reduce_kernel(const double* __restrict__ slab, int slices, int n_tri,
                                                                  int tiles, int dim, int64_t n,
                                                                  double* __restrict__ sigma) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= dim || i > j) return;
    const int tr = i / kTS, tc = j / kTS;
    const int t = tr * tiles - tr * (tr - 1) / 2 + (tc - tr);
    const double* p = slab + (size_t)t * (kTS * kTS) + (i % kTS) * kTS + (j % kTS);
    const size_t stride = (size_t)n_tri * (kTS * kTS);
    double s = 0.0;
    for (int sl = 0; sl < slices; ++sl) s += p[sl * stride];
    const double v = s / (double)n;
    sigma[(int64_t)i * dim + j] = v;
    sigma[(int64_t)j * dim + i] = v;      // the same bits: sigma == sigma^T exactly
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

struct StatsPlan {
    int tiles, n_tri, slices;
    int64_t rows_per_slice;
    int64_t* cstart;      // device copy of class_start
    double* slab;         // scatter partials, one kTS x kTS tile per (slice, triangle tile)
    size_t total;
};

StatsPlan make_stats_plan(void* ws, int64_t n, int dim, int n_classes) {
    StatsPlan p{};
    p.tiles = (dim + kTS - 1) / kTS;
    p.n_tri = p.tiles * (p.tiles + 1) / 2;
    const int64_t by_blocks = std::max<int64_t>(1, kScatterBlocks / p.n_tri);
    const int64_t by_rows = std::max<int64_t>(1, (n + 255) / 256);         // at least 256 rows a slice
    p.slices = (int)std::min(by_blocks, by_rows);
    p.rows_per_slice = ((n + p.slices - 1) / p.slices + kKC - 1) / kKC * kKC;
    Carver c(ws);
    p.cstart = c.take<int64_t>((size_t)n_classes + 1);
    p.slab = c.take<double>((size_t)p.slices * p.n_tri * kTS * kTS);
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
    if (class_start_host[0] != 0 || class_start_host[n_classes] != n)
        return g_perr.fail(XVEC_ERR_ARG, "class_start must run from 0 to n = %lld (got %lld .. %lld)", (long long)n,
                           (long long)class_start_host[0], (long long)class_start_host[n_classes]);
    for (int c = 0; c < n_classes; ++c)
        if (class_start_host[c + 1] < class_start_host[c])
            return g_perr.fail(XVEC_ERR_ARG, "class_start decreases at class %d", c);
    const StatsPlan p = make_stats_plan(workspace, n, dim, n_classes);
    int rc;
    if ((rc = workspace_ok(workspace_bytes, p.total, g_perr))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(p.cstart, class_start_host, (size_t)(n_classes + 1) * sizeof(int64_t),
                                  hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return g_perr.fail(XVEC_ERR_HIP, "class_start copy failed: %s", hipGetErrorString(e));
    if (x_dtype == XVEC_PLDA_X_F32)
        plda_class_sum_kernel<float><<<n_classes, 256, 0, s>>>(static_cast<const float*>(x), n, dim, order, p.cstart,
                                                                scaling_factor, class_sums, counts);
    else
        plda_class_sum_kernel<double><<<n_classes, 256, 0, s>>>(static_cast<const double*>(x), n, dim, order, p.cstart,
                                                                 scaling_factor, class_sums, counts);
    if ((rc = g_perr.launch_ok("plda_class_sum_kernel"))) return rc;
    plda_mean_kernel<<<(dim + kMeanCols - 1) / kMeanCols, 256, 0, s>>>(class_sums, n_classes, dim, n, mean);
    if ((rc = g_perr.launch_ok("plda_mean_kernel"))) return rc;
    const int64_t cd = (int64_t)n_classes * dim;
    plda_centre_kernel<<<(unsigned)((cd + 255) / 256), 256, 0, s>>>(class_sums, class_sums_t, counts, mean, n_classes, dim,
                                                                   scaling_factor);
    if ((rc = g_perr.launch_ok("plda_centre_kernel"))) return rc;
    ScatterArgs g{};
    g.x = x;
    g.mean = mean;
    g.slab = p.slab;
    g.n = n;
    g.rows_per_slice = p.rows_per_slice;
    g.dim = dim;
    g.tiles = p.tiles;
    g.n_tri = p.n_tri;
    const unsigned grid = (unsigned)(p.slices * p.n_tri);
    const bool vec = dim % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0;
    if (x_dtype == XVEC_PLDA_X_F32) {
        if (vec) plda_scatter_kernel<float, true><<<grid, 256, 0, s>>>(g);
        else plda_scatter_kernel<float, false><<<grid, 256, 0, s>>>(g);
    } else {
        if (vec) plda_scatter_kernel<double, true><<<grid, 256, 0, s>>>(g);
        else plda_scatter_kernel<double, false><<<grid, 256, 0, s>>>(g);
    }
    if ((rc = g_perr.launch_ok("plda_scatter_kernel"))) return rc;
    plda_scatter_reduce_kernel<<<dim3((dim + 255) / 256, dim), 256, 0, s>>>(p.slab, p.slices, p.n_tri, p.tiles, dim, n,
                                                                           sigma_obs);
    return g_perr.launch_ok("plda_scatter_reduce_kernel");
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
