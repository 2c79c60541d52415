// Embedding conditioning: the N-scale statistics of LDA and the affine transform with a length-norm epilogue, fp64.
//   reference: plda_classifier.py:103-106 -> speechbrain 0.5.12 LDA().do_lda(stat, reduced_dim) (numpy float64),
//              called at plda_score_stat.py:207-212; StatObject_SB.center_stat1 / rotate_stat1 / whiten_stat1 / norm_stat1
// C ABI: include/xvec_lda.h.  The D x D eigenproblem runs on the host, xvector_amd.lda.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

#include "../../include/xvec_hip.h"
#include "../../include/xvec_lda.h"
#include "host_support.h"
#include "tdnn_common.h"

namespace xvec {
namespace {

#include "class_scatter.h"      // inside the anonymous namespace: this file's own instances of the shared statistics kernels

// ---------------------------------------------------------------- class sums, class means

// One block per class: sums[c, :] = sum of the class's rows in `order` order (class_sum_columns); cls[i] = c for the class's
// positions i of `order`, inv_n[c] = 1 / rows.
template <typename T>
__global__ __launch_bounds__(256) void lda_class_sum_kernel(const T* __restrict__ x, int64_t n, int dim,
                                                            const int* __restrict__ order,
                                                            const int64_t* __restrict__ cstart, double* __restrict__ sums,
                                                            int* __restrict__ cls, double* __restrict__ inv_n) {
    const int c = blockIdx.x;
    int64_t b, e;
    class_rows(cstart, c, n, b, e);
    if (threadIdx.x == 0) inv_n[c] = 1.0 / (double)(e - b);
    for (int64_t i = b + threadIdx.x; i < e; i += 256) cls[i] = c;
    class_sum_columns(x, n, dim, order, c, b, e, sums);
}

// sums[c, d] <- sums[c, d] / rows of class c: the class means, in place
__global__ __launch_bounds__(256) void lda_class_mean_kernel(double* __restrict__ sums, const int64_t* __restrict__ cstart,
                                                             int n_classes, int dim) {
    const int64_t idx = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (idx >= (int64_t)n_classes * dim) return;
    const int c = (int)(idx / dim);
    sums[idx] = sums[idx] / (double)(cstart[c + 1] - cstart[c]);
}

// ---------------------------------------------------------------- transform with the length-norm epilogue

// Sum of squares of row `yrow` [rank] over the 16 threads of a group (t = lane & 15): thread t takes the columns
// t, t + 16, .. in order, then a butterfly over the 16 partials (a + b is commutative: every lane gets the same bits).
// All 64 lanes of the wave must call it (a lane without a row passes yrow == nullptr).
__device__ __forceinline__ double row_sumsq16(const double* yrow, int rank, int t) {
    double s = 0.0;
    if (yrow)
        for (int j = t; j < rank; j += 16) {
            const double v = yrow[j];
            s = __builtin_fma(v, v, s);
        }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) s += __shfl_xor(s, m, 16);
    return s;
}

constexpr double kNormClip = 1e-8;      // speechbrain's norm_stat1: vect_norm = clip(norm, a_min=1e-8)
constexpr int kRG = XVEC_EMBED_ROW_GROUP;       // rows a block owns
constexpr int kLDX = 18;       // LDS row stride of the x image in doubles (144 B): the 16 rows x 2 k of half a wave's ds_read_b64 hit 32 bank pairs

struct EmbedArgs {
    const void* x;
    const double* mean;
    const double* w;
    double* y;
    double* norms;
    int64_t n, ldx, ldy;
    int dim, rank, normalize;
};

// y = (x - mean) W for one group of 64 rows: the block sweeps the column tiles (64 wide) of its rows, K = dim in chunks of 16
// through double-buffered LDS -- the x chunk as [row][k] (centred while staged), the W chunk as [k][column] -- 4 waves as
// 2 x 2, each 32 x 32 = 2 x 2 tiles of v_mfma_f64_16x16x4_f64 (A[i][k]: lane l takes row l & 15, k = l >> 4).  With
// `normalize` the block then takes the norm of each of its rows from what it wrote (row_sumsq16) and divides the row by it.
template <typename T, bool VEC>
__global__ __launch_bounds__(256, 4) void embed_transform_kernel(const EmbedArgs g) {
    __shared__ __attribute__((aligned(16))) double sX[2][kRG][kLDX];
    __shared__ __attribute__((aligned(16))) double sW[2][kKC][kLD];
    const int64_t g0 = (int64_t)blockIdx.x * kRG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    const int xrow = tid >> 2, xk = (tid & 3) * 4;               // x staging: 64 rows x 16 k, four k a thread
    const int wk = tid >> 4, wcol = (tid & 15) * 4;              // W staging: 16 k x 64 columns, four columns a thread
    const T* __restrict__ x = static_cast<const T*>(g.x);
    const bool xvalid = g0 + xrow < g.n;
    const T* __restrict__ xp = x + (xvalid ? (g0 + xrow) * g.ldx : 0);
    const int n_chunks = (g.dim + kKC - 1) / kKC;

    for (int j0 = 0; j0 < g.rank; j0 += kTS) {
        T rx[4];
        double rm[4], rw[4];
        bool kv[4];
        auto gload = [&](int k0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                kv[q] = k0 + xk + q < g.dim;
                rx[q] = T(0);
                rm[q] = (g.mean && kv[q]) ? g.mean[k0 + xk + q] : 0.0;
            }
            if (xvalid) {
                if constexpr (VEC) {        // dim % 4 == 0, ldx % 4 == 0, 16-byte aligned base
                    if (kv[0]) {
                        if constexpr (sizeof(T) == 4) {
                            const f32x4 v = *reinterpret_cast<const f32x4*>(xp + k0 + xk);
                            rx[0] = v.x; rx[1] = v.y; rx[2] = v.z; rx[3] = v.w;
                        } else {
                            const f64x2 v0 = *reinterpret_cast<const f64x2*>(xp + k0 + xk);
                            const f64x2 v1 = *reinterpret_cast<const f64x2*>(xp + k0 + xk + 2);
                            rx[0] = v0.x; rx[1] = v0.y; rx[2] = v1.x; rx[3] = v1.y;
                        }
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (kv[q]) rx[q] = xp[k0 + xk + q];
                }
            }
            const bool wkv = k0 + wk < g.dim;
            const double* wp = g.w + (int64_t)(wkv ? k0 + wk : 0) * g.rank;
#pragma unroll
            for (int q = 0; q < 4; ++q) rw[q] = (wkv && j0 + wcol + q < g.rank) ? wp[j0 + wcol + q] : 0.0;
        };
        // rows past n, k past dim and columns past rank stay exactly zero
        auto lstore = [&](int buf) {
            double a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = xvalid && kv[q] ? (double)rx[q] - rm[q] : 0.0;
            *reinterpret_cast<f64x2*>(&sX[buf][xrow][xk]) = f64x2{a[0], a[1]};
            *reinterpret_cast<f64x2*>(&sX[buf][xrow][xk + 2]) = f64x2{a[2], a[3]};
            *reinterpret_cast<f64x2*>(&sW[buf][wk][wcol]) = f64x2{rw[0], rw[1]};
            *reinterpret_cast<f64x2*>(&sW[buf][wk][wcol + 2]) = f64x2{rw[2], rw[3]};
        };

        f64x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
        const int nj = std::min(2, std::max(0, (g.rank - j0 - wc * 32 + 15) / 16));   // 16-column tiles of this wave that hold columns

        gload(0);
        lstore(0);
        __syncthreads();
        for (int ch = 0; ch < n_chunks; ++ch) {
            const int buf = ch & 1;
            if (ch + 1 < n_chunks) gload((ch + 1) * kKC);
#pragma unroll
            for (int ks = 0; ks < kKC / 4; ++ks) {
                const int k = ks * 4 + l4;
                double a[2], b[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    a[i] = sX[buf][wr * 32 + i * 16 + l15][k];
                    b[i] = sW[buf][k][wc * 32 + i * 16 + l15];
                }
                if (nj > 0) {
                    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b[0], acc[0][0], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], b[0], acc[1][0], 0, 0, 0);
                }
                if (nj > 1) {
                    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b[1], acc[0][1], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], b[1], acc[1][1], 0, 0, 0);
                }
            }
            if (ch + 1 < n_chunks) lstore(buf ^ 1);
            __syncthreads();
        }

        // C/D of the f64 MFMA: column lane & 15, row (lane >> 4) + 4 reg
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t row = g0 + wr * 32 + i * 16 + l4 + 4 * r;
                    const int col = j0 + wc * 32 + j * 16 + l15;
                    if (row < g.n && col < g.rank) g.y[row * g.ldy + col] = acc[i][j][r];
                }
    }
    if (!g.normalize) return;

    __threadfence_block();
    __syncthreads();          // the block's own rows of y are complete and visible to all of its threads
    const int t = tid & 15;
#pragma unroll 1
    for (int rr = 0; rr < kRG / 16; ++rr) {
        const int64_t row = g0 + rr * 16 + (tid >> 4);
        double* yrow = row < g.n ? g.y + row * g.ldy : nullptr;
        const double norm = std::max(sqrt(row_sumsq16(yrow, g.rank, t)), kNormClip);
        if (!yrow) continue;
        if (t == 0) g.norms[row] = norm;
        for (int j = t; j < g.rank; j += 16) yrow[j] = yrow[j] / norm;
    }
}

// w == nullptr: y = x - mean, and with `normalize` each row divided by its clipped norm.  16 rows a block, 16 threads a row;
// a thread writes the columns t, t + 16, .. and rescales exactly those.
template <typename T>
__global__ __launch_bounds__(256) void embed_centre_kernel(const EmbedArgs g) {
    const int t = threadIdx.x & 15;
    const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool valid = row < g.n;
    const T* __restrict__ xp = static_cast<const T*>(g.x) + (valid ? row * g.ldx : 0);
    double* yrow = valid ? g.y + row * g.ldy : nullptr;
    if (valid)
        for (int j = t; j < g.dim; j += 16) yrow[j] = (double)xp[j] - (g.mean ? g.mean[j] : 0.0);
    if (!g.normalize) return;
    // each thread reads back only what it wrote itself
    const double norm = std::max(sqrt(row_sumsq16(yrow, g.dim, t)), kNormClip);
    if (!valid) return;
    if (t == 0) g.norms[row] = norm;
    for (int j = t; j < g.dim; j += 16) yrow[j] = yrow[j] / norm;
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_lerr;

constexpr int kSliceRows = 32;         // a slice is worth opening for this many rows

struct StatsPlan {
    int tiles, n_tri;
    ScatterPlan within, between;
    int64_t* cstart;      // device copy of class_start
    int* cls;             // class of every position of `order`
    double* inv_n;        // 1 / rows of the class
    double* slab;         // scatter partials, one kTS x kTS tile per (slice, triangle tile); both products use it in turn
    size_t total;
};

StatsPlan make_stats_plan(void* ws, int64_t n, int dim, int n_classes) {
    StatsPlan p{};
    p.tiles = (dim + kTS - 1) / kTS;
    p.n_tri = p.tiles * (p.tiles + 1) / 2;
    p.within = make_scatter_plan(n, p.n_tri, kSliceRows);
    p.between = make_scatter_plan(n_classes, p.n_tri, kSliceRows);
    Carver c(ws);
    p.cstart = c.take<int64_t>((size_t)n_classes + 1);
    p.cls = c.take<int>((size_t)n);
    p.inv_n = c.take<double>((size_t)n_classes);
    p.slab = c.take<double>((size_t)std::max(p.within.slices, p.between.slices) * p.n_tri * kTS * kTS);
    p.total = c.total();
    return p;
}

bool stats_args_ok(int64_t n, int dim, int n_classes) {
    return n >= 1 && n <= 0x7fffffff && dim >= 1 && n_classes >= 1 && n_classes <= n;
}

bool embed_args_ok(int64_t n, int dim, int rank) {
    return n >= 1 && n <= 0x7fffffff && dim >= 1 && dim <= XVEC_EMBED_MAX_DIM && rank >= 1 && rank <= dim;
}

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_lda_last_error(void) { return g_lerr.c_str(); }

size_t xvec_lda_stats_workspace_bytes(int64_t n, int32_t dim, int32_t n_classes) {
    if (!stats_args_ok(n, dim, n_classes)) return 0;
    return make_stats_plan(nullptr, n, dim, n_classes).total;
}

// Launches: class sums (one block per class), mean, class means, then twice (within, between) scatter partials + reduce.
int xvec_lda_stats(const void* x, int32_t x_dtype, int64_t n, int32_t dim, const int32_t* order,
                   const int64_t* class_start_host, int32_t n_classes, double* mean, double* class_means, double* s_within,
                   double* s_between, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    if (n < 1) return g_lerr.fail(XVEC_ERR_ARG, "need at least one vector (n = %lld)", (long long)n);
    if (n > 0x7fffffff) return g_lerr.fail(XVEC_ERR_TOO_LARGE, "n = %lld: row indices are int32", (long long)n);
    if (dim < 1 || n_classes < 1) return g_lerr.fail(XVEC_ERR_ARG, "dim = %d and n_classes = %d must be >= 1", dim, n_classes);
    if (n_classes > n) return g_lerr.fail(XVEC_ERR_ARG, "more classes (%d) than vectors (%lld)", n_classes, (long long)n);
    if (x_dtype != XVEC_LDA_X_F32 && x_dtype != XVEC_LDA_X_F64) return g_lerr.fail(XVEC_ERR_ARG, "x_dtype %d unknown", x_dtype);
    if (!x || !order || !class_start_host || !mean || !class_means || !s_within || !s_between || !workspace)
        return g_lerr.fail(XVEC_ERR_ARG, "null pointer");
    int rc;
    if ((rc = class_start_spans(class_start_host, n_classes, n, g_lerr))) return rc;
    if (const int c = first_short_class(class_start_host, n_classes, 1); c >= 0)
        return g_lerr.fail(XVEC_ERR_ARG, "class %d is empty or class_start decreases: every class needs a row", c);
    const StatsPlan p = make_stats_plan(workspace, n, dim, n_classes);
    if ((rc = workspace_ok(workspace_bytes, p.total, g_lerr))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((rc = upload_class_start(p.cstart, class_start_host, n_classes, s, g_lerr))) return rc;
    if (x_dtype == XVEC_LDA_X_F32)
        lda_class_sum_kernel<float><<<n_classes, 256, 0, s>>>(static_cast<const float*>(x), n, dim, order, p.cstart,
                                                               class_means, p.cls, p.inv_n);
    else
        lda_class_sum_kernel<double><<<n_classes, 256, 0, s>>>(static_cast<const double*>(x), n, dim, order, p.cstart,
                                                                class_means, p.cls, p.inv_n);
    if ((rc = g_lerr.launch_ok("lda_class_sum_kernel"))) return rc;
    stats_mean_kernel<<<(dim + kMeanCols - 1) / kMeanCols, 256, 0, s>>>(class_means, n_classes, dim, n, mean);
    if ((rc = g_lerr.launch_ok("stats_mean_kernel"))) return rc;
    const int64_t cd = (int64_t)n_classes * dim;
    lda_class_mean_kernel<<<(unsigned)((cd + 255) / 256), 256, 0, s>>>(class_means, p.cstart, n_classes, dim);
    if ((rc = g_lerr.launch_ok("lda_class_mean_kernel"))) return rc;

    ScatterArgs g{};
    g.slab = p.slab;
    g.dim = dim;
    g.tiles = p.tiles;
    g.n_tri = p.n_tri;
    // within-class: the rows of x through `order`, centred by their class mean, weighted by 1 / n_c
    g.x = x;
    g.order = order;
    g.cls = p.cls;
    g.centre = class_means;
    g.wts = p.inv_n;
    g.n = n;
    g.n_centres = n_classes;
    if ((rc = launch_scatter<true>(g, x_dtype == XVEC_LDA_X_F32, p.within, 1.0, s_within, s, g_lerr))) return rc;
    // between-class: the class means, centred by the mean, weight 1
    g.x = class_means;
    g.order = nullptr;
    g.cls = nullptr;
    g.centre = mean;
    g.wts = nullptr;
    g.n = n_classes;
    g.n_centres = 1;
    return launch_scatter<true>(g, false, p.between, 1.0, s_between, s, g_lerr);
}

size_t xvec_embed_transform_workspace_bytes(int64_t n, int32_t dim, int32_t rank) {
    if (!embed_args_ok(n, dim, rank)) return 0;
    return align256((size_t)n * sizeof(double));
}

// One launch: embed_transform_kernel (w given) or embed_centre_kernel (w == NULL); the norm epilogue is part of it.
int xvec_embed_transform(const void* x, int32_t x_dtype, int64_t n, int32_t dim, int64_t ldx, const double* mean,
                         const double* w, int32_t rank, int32_t normalize, double* y, int64_t ldy, void* workspace,
                         size_t workspace_bytes, xvec_stream stream) {
    if (n < 1) return g_lerr.fail(XVEC_ERR_ARG, "need at least one vector (n = %lld)", (long long)n);
    if (dim < 1 || dim > XVEC_EMBED_MAX_DIM)
        return g_lerr.fail(dim < 1 ? XVEC_ERR_ARG : XVEC_ERR_TOO_LARGE, "dim = %d must lie in [1, %d]", dim, XVEC_EMBED_MAX_DIM);
    if (rank < 1 || rank > dim) return g_lerr.fail(XVEC_ERR_ARG, "rank = %d must lie in [1, dim = %d]", rank, dim);
    if (x_dtype != XVEC_LDA_X_F32 && x_dtype != XVEC_LDA_X_F64) return g_lerr.fail(XVEC_ERR_ARG, "x_dtype %d unknown", x_dtype);
    if (!x || !y || !workspace) return g_lerr.fail(XVEC_ERR_ARG, "null pointer");
    if (!w && rank != dim) return g_lerr.fail(XVEC_ERR_ARG, "w == NULL is the identity: rank = %d must equal dim = %d", rank, dim);
    if (ldx < dim || ldy < rank)
        return g_lerr.fail(XVEC_ERR_ARG, "row strides ldx = %lld, ldy = %lld must cover dim = %d, rank = %d", (long long)ldx,
                           (long long)ldy, dim, rank);
    if (n > 0x7fffffff) return g_lerr.fail(XVEC_ERR_TOO_LARGE, "n = %lld: at most 2^31 - 1 rows a call", (long long)n);
    const size_t xsz = x_dtype == XVEC_LDA_X_F32 ? 4 : 8;
    const uintptr_t xb = reinterpret_cast<uintptr_t>(x), xe = xb + ((size_t)(n - 1) * ldx + dim) * xsz;
    const uintptr_t yb = reinterpret_cast<uintptr_t>(y), ye = yb + ((size_t)(n - 1) * ldy + rank) * sizeof(double);
    if (xb < ye && yb < xe) return g_lerr.fail(XVEC_ERR_ARG, "y overlaps x: the transform does not run in place");
    int rc;
    if ((rc = workspace_ok(workspace_bytes, align256((size_t)n * sizeof(double)), g_lerr))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    EmbedArgs g{};
    g.x = x;
    g.mean = mean;
    g.w = w;
    g.y = y;
    g.norms = static_cast<double*>(workspace);
    g.n = n;
    g.ldx = ldx;
    g.ldy = ldy;
    g.dim = dim;
    g.rank = rank;
    g.normalize = normalize != 0;
    if (!w) {
        const unsigned grid = (unsigned)((n + 15) / 16);
        if (x_dtype == XVEC_LDA_X_F32) embed_centre_kernel<float><<<grid, 256, 0, s>>>(g);
        else embed_centre_kernel<double><<<grid, 256, 0, s>>>(g);
        return g_lerr.launch_ok("embed_centre_kernel");
    }
    const unsigned grid = (unsigned)((n + kRG - 1) / kRG);
    const bool vec = dim % 4 == 0 && ldx % 4 == 0 && xb % 16 == 0;
    if (x_dtype == XVEC_LDA_X_F32) {
        if (vec) embed_transform_kernel<float, true><<<grid, 256, 0, s>>>(g);
        else embed_transform_kernel<float, false><<<grid, 256, 0, s>>>(g);
    } else {
        if (vec) embed_transform_kernel<double, true><<<grid, 256, 0, s>>>(g);
        else embed_transform_kernel<double, false><<<grid, 256, 0, s>>>(g);
    }
    return g_lerr.launch_ok("embed_transform_kernel");
}

}  // extern "C"
