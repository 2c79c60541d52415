// Speaker identification: per-model means of the enrolment vectors, open-set scores, the k best models of every test column.
// C ABI and the definitions: include/xvec_ident.h.
//   model mean  one block per model: the class-sum column walk of class_sums.h (what PLDA and LDA training sum their classes
//               with), then the division by the model's row count.
//   col stats   per column of S[N, T] the maximum m1, its first row i1 and R = sum over k != i1 of exp(S[k] - m1).  A lane owns
//               a column (a wave reads 64 consecutive columns of a row: 512 contiguous bytes), a wave a slice of 32 rows that it
//               holds in registers (every load in flight at once), a block the 128 rows of its four waves: the waves'
//               partials are combined through LDS in wave order.  N > 128: the blocks' partials go to the workspace and
//               ident_col_merge_kernel combines them in block order.
//   apply       out = S - L, tiles of 8 rows x 256 columns, a thread per column (one exp and one log per cell).
//   top-k       the same slices, four per wave (512 rows per block); a lane keeps its column's KK best (value, row) sorted in
//               registers, lists are merged in slice order through LDS and, for N > 512, through the workspace.
// No atomics at all.  Every sum and every merge has one order, fixed by N alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "../../include/xvec_hip.h"
#include "../../include/xvec_ident.h"
#include "host_support.h"

// Every operation rounds on its own: the error bound of tests/test_ident_gpu.py counts roundings.
#pragma clang fp contract(off)

namespace xvec {
namespace {

#include "class_sums.h"      // inside the anonymous namespace, as class_scatter.h includes it for plda_train.hip and lda.hip

constexpr int kCols = XVEC_IDENT_COLS;
constexpr int kSlice = XVEC_IDENT_SLICE_ROWS;
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kBlockRows = XVEC_IDENT_BLOCK_ROWS;
constexpr int kTopkBlockRows = XVEC_IDENT_TOPK_BLOCK_ROWS;
constexpr int kTopkSlices = kTopkBlockRows / (kWaves * kSlice);      // slices a wave of the top-k walk takes, one after the other
constexpr int kApplyRows = XVEC_IDENT_APPLY_ROWS;
constexpr int kApplyCols = XVEC_IDENT_APPLY_COLS;
constexpr int kMaxK = XVEC_IDENT_MAX_K;
static_assert(kCols == 64, "a lane per column");
static_assert(kBlockRows == kWaves * kSlice && kTopkBlockRows == kWaves * kSlice * kTopkSlices, "block rows");

// ---------------------------------------------------------------- model mean

template <typename T>
__global__ __launch_bounds__(256) void model_mean_kernel(const T* __restrict__ x, int64_t n, int dim, int64_t ld,
                                                         const int* __restrict__ order, const int64_t* __restrict__ mstart,
                                                         double* __restrict__ out) {
    const int c = blockIdx.x;
    int64_t b, e;
    class_rows(mstart, c, n, b, e);
    class_sum_columns(x, n, dim, ld, order, c, b, e, out);
    // the thread that summed column d divides it: no other thread touches out[c, d]
    const double rows = (double)(e - b);
    for (int d = threadIdx.x; d < dim; d += 256) {
        double* p = out + (int64_t)c * dim + d;
        *p = *p / rows;
    }
}

// ---------------------------------------------------------------- slices

// The slice's cell of this lane's column in row r0 + k, k = 0 .. kSlice - 1; rows past N and columns past T are not read.
__device__ __forceinline__ void load_slice(const double* __restrict__ S, int64_t ld, int64_t N, int64_t r0, int64_t col,
                                           bool col_ok, double (&x)[kSlice]) {
#pragma unroll
    for (int k = 0; k < kSlice; ++k) {
        const int64_t row = r0 + k;
        x[k] = (col_ok && row < N) ? S[row * ld + col] : 0.0;
    }
}

// ---------------------------------------------------------------- column statistics

// What a range of rows knows of its column: the maximum m, the first row i that has it (-1: no rows), and
// R = sum over the range's other rows of exp(S - m).  A NaN cell makes m and R NaN.
struct Partial {
    double m, R;
    int i;
};

// exp(x - m) for x <= m; a -inf cell adds nothing (m = -inf too: a range of nothing but -inf)
__device__ __forceinline__ double exp_below(double x, double m) {
    return x == -std::numeric_limits<double>::infinity() ? 0.0 : exp(x - m);
}

// a's rows come before b's.  The side whose maximum loses is rescaled to the winner's, and its own maximum joins the sum
// as the + 1; equal maxima keep a's row (the lower index).  A factor exp(0) is exactly 1.
__device__ __forceinline__ Partial merge(const Partial& a, const Partial& b) {
    Partial r;
    if (a.m != a.m || b.m != b.m) {
        r.m = r.R = std::numeric_limits<double>::quiet_NaN();
        r.i = a.m != a.m ? a.i : b.i;
    } else if (a.i < 0 || b.m > a.m) {
        r.m = b.m;
        r.i = b.i;
        r.R = (a.i >= 0 ? (a.R + 1.0) * exp_below(a.m, b.m) : 0.0) + b.R;
    } else {
        r.m = a.m;
        r.i = a.i;
        r.R = a.R + (b.i >= 0 ? (b.R + 1.0) * exp_below(b.m, a.m) : 0.0);
    }
    return r;
}

// rows [r0, r0 + kSlice) of the lane's column
__device__ __forceinline__ Partial slice_partial(const double (&x)[kSlice], int64_t r0, int64_t N) {
    const double ninf = -std::numeric_limits<double>::infinity();
    const int rows = (int)std::min<int64_t>(std::max<int64_t>(N - r0, 0), kSlice);
    Partial p{ninf, 0.0, -1};
    bool nan = false;
    int at = -1;
#pragma unroll
    for (int k = 0; k < kSlice; ++k) {
        if (k < rows) {
            nan |= x[k] != x[k];
            if (at < 0 || x[k] > p.m) {
                p.m = x[k];
                at = k;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kSlice; ++k)
        if (k < rows && k != at) p.R += exp_below(x[k], p.m);
    if (at >= 0) p.i = (int)(r0 + at);
    if (nan) p.m = p.R = std::numeric_limits<double>::quiet_NaN();
    return p;
}

struct ColStatsArgs {
    const double* S;
    int64_t ld, N, T, col_tiles, row_blocks;
    double *m, *R;      // row_blocks == 1: the column statistics [T]; else the blocks' partials [row_blocks, T]
    int* i;
};

__global__ __launch_bounds__(kThreads) void ident_col_stats_kernel(const ColStatsArgs g) {
    __shared__ double sm[kWaves - 1][kCols], sR[kWaves - 1][kCols];
    __shared__ int si[kWaves - 1][kCols];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rb = blockIdx.x / g.col_tiles, ct = blockIdx.x - rb * g.col_tiles;
    const int64_t col = ct * kCols + lane;
    const bool col_ok = col < g.T;
    const int64_t r0 = rb * kBlockRows + (int64_t)wave * kSlice;
    double x[kSlice];
    load_slice(g.S, g.ld, g.N, r0, col, col_ok, x);
    Partial p = slice_partial(x, r0, g.N);
    if (wave > 0) {
        sm[wave - 1][lane] = p.m;
        sR[wave - 1][lane] = p.R;
        si[wave - 1][lane] = p.i;
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int w = 0; w < kWaves - 1; ++w) p = merge(p, Partial{sm[w][lane], sR[w][lane], si[w][lane]});
        if (col_ok) {
            const int64_t o = rb * g.T + col;
            g.m[o] = p.m;
            g.R[o] = p.R;
            g.i[o] = p.i;
        }
    }
}

// the blocks' partials of a column, in block order
__global__ __launch_bounds__(256) void ident_col_merge_kernel(const double* __restrict__ pm, const double* __restrict__ pR,
                                                              const int* __restrict__ pi, int64_t row_blocks, int64_t T,
                                                              double* __restrict__ m, double* __restrict__ R,
                                                              int* __restrict__ i) {
    const int64_t col = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (col >= T) return;
    Partial p{pm[col], pR[col], pi[col]};
    for (int64_t rb = 1; rb < row_blocks; ++rb) p = merge(p, Partial{pm[rb * T + col], pR[rb * T + col], pi[rb * T + col]});
    m[col] = p.m;
    R[col] = p.R;
    i[col] = p.i;
}

struct OpenSetArgs {
    const double* S;
    double* out;
    int64_t ld, ld_out, N, T, col_tiles;
    const double *m, *R;
    const int* i;
    double p;
};

__global__ __launch_bounds__(kApplyCols) void ident_open_set_kernel(const OpenSetArgs g) {
    const int64_t tile_r = blockIdx.x / g.col_tiles, tile_c = blockIdx.x - tile_r * g.col_tiles;
    const int64_t j = tile_c * kApplyCols + threadIdx.x;
    if (j >= g.T) return;
    const double m1 = g.m[j], R = g.R[j];
    const int64_t i1 = g.i[j];
    const double p = g.p, others = (double)(g.N - 1), rest = 1.0 - p;
    // the side the logarithm is taken on (a NaN maximum takes the second, which gives NaN as well)
    const bool shifted = m1 > 0.0 || p == 1.0;
    // shifted: the (1 - p) term scaled down by exp(-m1), an explicit 0 for p == 1 (0 * exp(900) is NaN); else exp(m1) <= 1
    const double c = shifted ? (p == 1.0 ? 0.0 : rest * exp(-m1)) : exp(m1);
    const int64_t i0 = tile_r * kApplyRows;
#pragma unroll
    for (int r = 0; r < kApplyRows; ++r) {
        const int64_t i = i0 + r;
        if (i >= g.N) break;
        const double s = g.S[i * g.ld + j];
        const double A = i == i1 ? R : 1.0 + (R - exp_below(s, m1));
        const double q = (p * A) / others;
        const double L = shifted ? m1 + log(q + c) : log(c * q + rest);
        g.out[i * g.ld_out + j] = s - L;
    }
}

// ---------------------------------------------------------------- top-k

// The KK best (value, row) of a column, best first; a free place has row -1 and value NaN.
template <int KK>
struct TopList {
    double v[KK];
    int i[KK];
};

// does the candidate (av, ai), a real cell that is not NaN, come before the entry (bv, bi)?
__device__ __forceinline__ bool before(double av, int ai, double bv, int bi) {
    return bi < 0 || av > bv || (av == bv && ai < bi);
}

template <int KK>
__device__ __forceinline__ void clear(TopList<KK>& t) {
#pragma unroll
    for (int j = 0; j < KK; ++j) {
        t.v[j] = std::numeric_limits<double>::quiet_NaN();
        t.i[j] = -1;
    }
}

// The candidate takes the last place if it comes before what is there, and moves up while it comes before its neighbour;
// the loop has no exit so that every index is a constant and the list stays in registers.
template <int KK>
__device__ __forceinline__ void insert(TopList<KK>& t, double v, int i) {
    if (!before(v, i, t.v[KK - 1], t.i[KK - 1])) return;
    t.v[KK - 1] = v;
    t.i[KK - 1] = i;
#pragma unroll
    for (int j = KK - 1; j >= 1; --j) {
        const bool up = t.i[j] >= 0 && before(t.v[j], t.i[j], t.v[j - 1], t.i[j - 1]);
        const double hv = t.v[j - 1];
        const int hi = t.i[j - 1];
        t.v[j - 1] = up ? t.v[j] : hv;
        t.i[j - 1] = up ? t.i[j] : hi;
        t.v[j] = up ? hv : t.v[j];
        t.i[j] = up ? hi : t.i[j];
    }
}

struct TopkArgs {
    const double* S;
    int64_t ld, N, T, col_tiles, row_blocks;
    int k;
    double threshold;
    double* part_v;     // row_blocks > 1: the blocks' lists [row_blocks, KK, T]
    int* part_i;
    int* idx;           // [k, T]
    double* val;
    int* decision;      // [T] or null
};

template <int KK>
__device__ __forceinline__ void write_result(const TopkArgs& g, const TopList<KK>& t, int64_t col) {
#pragma unroll
    for (int j = 0; j < KK; ++j) {
        if (j < g.k) {
            g.idx[j * g.T + col] = t.i[j];
            g.val[j * g.T + col] = t.v[j];
        }
    }
    if (g.decision) g.decision[col] = t.i[0] >= 0 && t.v[0] >= g.threshold ? t.i[0] : -1;
}

template <int KK>
__global__ __launch_bounds__(kThreads) void ident_topk_kernel(const TopkArgs g) {
    __shared__ double sv[kWaves - 1][KK][kCols];
    __shared__ int si[kWaves - 1][KK][kCols];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rb = blockIdx.x / g.col_tiles, ct = blockIdx.x - rb * g.col_tiles;
    const int64_t col = ct * kCols + lane;
    const bool col_ok = col < g.T;
    TopList<KK> t;
    clear(t);
    for (int s = 0; s < kTopkSlices; ++s) {
        const int64_t r0 = rb * kTopkBlockRows + ((int64_t)wave * kTopkSlices + s) * kSlice;
        if (r0 >= g.N) break;
        double x[kSlice];
        load_slice(g.S, g.ld, g.N, r0, col, col_ok, x);
        const int rows = (int)std::min<int64_t>(g.N - r0, kSlice);
#pragma unroll
        for (int k = 0; k < kSlice; ++k)
            if (k < rows && x[k] == x[k]) insert(t, x[k], (int)(r0 + k));
    }
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < KK; ++j) {
            sv[wave - 1][j][lane] = t.v[j];
            si[wave - 1][j][lane] = t.i[j];
        }
    }
    __syncthreads();
    if (wave != 0) return;
    for (int w = 0; w < kWaves - 1; ++w) {
#pragma unroll
        for (int j = 0; j < KK; ++j) {
            const int i = si[w][j][lane];
            if (i >= 0) insert(t, sv[w][j][lane], i);
        }
    }
    if (!col_ok) return;
    if (g.row_blocks == 1) {
        write_result(g, t, col);
    } else {
#pragma unroll
        for (int j = 0; j < KK; ++j) {
            const int64_t o = (rb * KK + j) * g.T + col;
            g.part_v[o] = t.v[j];
            g.part_i[o] = t.i[j];
        }
    }
}

// the blocks' lists of a column, in block order
template <int KK>
__global__ __launch_bounds__(256) void ident_topk_merge_kernel(const TopkArgs g) {
    const int64_t col = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (col >= g.T) return;
    TopList<KK> t;
    clear(t);
    for (int64_t rb = 0; rb < g.row_blocks; ++rb) {
#pragma unroll
        for (int j = 0; j < KK; ++j) {
            const int64_t o = (rb * KK + j) * g.T + col;
            const int i = g.part_i[o];
            if (i >= 0) insert(t, g.part_v[o], i);
        }
    }
    write_result(g, t, col);
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_ierr;

constexpr int64_t kMaxDim = 0x7fffffff;

int list_length(int k) { return k <= 1 ? 1 : (k <= 4 ? 4 : kMaxK); }

struct OpenSetPlan {
    int64_t row_blocks;
    double *m, *R, *pm, *pR;      // the column statistics [T]; the blocks' partials [row_blocks, T] (row_blocks > 1)
    int *i, *pi;
    size_t total;
};

OpenSetPlan make_open_set_plan(void* ws, int64_t N, int64_t T) {
    OpenSetPlan p{};
    p.row_blocks = (N + kBlockRows - 1) / kBlockRows;
    Carver c(ws);
    p.m = c.take<double>((size_t)T);
    p.R = c.take<double>((size_t)T);
    p.i = c.take<int>((size_t)T);
    if (p.row_blocks > 1) {
        p.pm = c.take<double>((size_t)p.row_blocks * T);
        p.pR = c.take<double>((size_t)p.row_blocks * T);
        p.pi = c.take<int>((size_t)p.row_blocks * T);
    }
    p.total = c.total();
    return p;
}

struct TopkPlan {
    int64_t row_blocks;
    int kk;
    double* pv;
    int* pi;
    size_t total;
};

TopkPlan make_topk_plan(void* ws, int64_t N, int64_t T, int k) {
    TopkPlan p{};
    p.row_blocks = (N + kTopkBlockRows - 1) / kTopkBlockRows;
    p.kk = list_length(k);
    Carver c(ws);
    if (p.row_blocks > 1) {
        p.pv = c.take<double>((size_t)p.row_blocks * p.kk * T);
        p.pi = c.take<int>((size_t)p.row_blocks * p.kk * T);
    }
    p.total = c.total();
    return p;
}

bool shape_ok(int64_t N, int64_t T) { return N >= 1 && T >= 1 && N <= kMaxDim && T <= kMaxDim; }

// blocks of a (row blocks) x (column tiles) grid, or -1 when they pass 2^31 - 1
int64_t grid_blocks(int64_t row_blocks, int64_t col_tiles) {
    const int64_t blocks = row_blocks * col_tiles;      // both below 2^31: no overflow
    return blocks <= kMaxDim ? blocks : -1;
}

template <int KK>
int launch_topk(const TopkArgs& g, unsigned grid, hipStream_t s) {
    ident_topk_kernel<KK><<<grid, kThreads, 0, s>>>(g);
    if (const int rc = g_ierr.launch_ok("ident_topk_kernel")) return rc;
    if (g.row_blocks == 1) return XVEC_OK;
    ident_topk_merge_kernel<KK><<<(unsigned)((g.T + 255) / 256), 256, 0, s>>>(g);
    return g_ierr.launch_ok("ident_topk_merge_kernel");
}

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_ident_last_error(void) { return g_ierr.c_str(); }

size_t xvec_model_mean_workspace_bytes(int32_t n_models) {
    if (n_models < 1) return 0;
    Carver c(nullptr);
    c.take<int64_t>((size_t)n_models + 1);
    return c.total();
}

int xvec_model_mean(const void* x, int32_t x_dtype, int64_t n, int32_t dim, int64_t ld, const int32_t* order,
                    const int64_t* model_start_host, int32_t n_models, double* out, void* workspace, size_t workspace_bytes,
                    xvec_stream stream) {
    if (n < 1) return g_ierr.fail(XVEC_ERR_ARG, "need at least one enrolment vector (n = %lld)", (long long)n);
    if (n > 0x7fffffff) return g_ierr.fail(XVEC_ERR_TOO_LARGE, "n = %lld: row indices are int32", (long long)n);
    if (dim < 1 || n_models < 1) return g_ierr.fail(XVEC_ERR_ARG, "dim = %d and n_models = %d must be >= 1", dim, n_models);
    if (n_models > n) return g_ierr.fail(XVEC_ERR_ARG, "more models (%d) than vectors (%lld)", n_models, (long long)n);
    if (ld < dim) return g_ierr.fail(XVEC_ERR_ARG, "ld = %lld is smaller than dim = %d", (long long)ld, dim);
    if (x_dtype != XVEC_IDENT_X_F32 && x_dtype != XVEC_IDENT_X_F64) return g_ierr.fail(XVEC_ERR_ARG, "x_dtype %d unknown", x_dtype);
    if (!x || !order || !model_start_host || !out || !workspace) return g_ierr.fail(XVEC_ERR_ARG, "null pointer");
    int rc;
    if ((rc = class_start_spans(model_start_host, n_models, n, g_ierr))) return rc;
    if (const int c = first_short_class(model_start_host, n_models, 1); c >= 0)
        return g_ierr.fail(XVEC_ERR_ARG, "model %d is empty or model_start decreases: every model needs a row", c);
    if ((rc = workspace_ok(workspace_bytes, xvec_model_mean_workspace_bytes(n_models), g_ierr))) return rc;
    int64_t* mstart = static_cast<int64_t*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((rc = upload_class_start(mstart, model_start_host, n_models, s, g_ierr))) return rc;
    if (x_dtype == XVEC_IDENT_X_F32)
        model_mean_kernel<float><<<n_models, 256, 0, s>>>(static_cast<const float*>(x), n, dim, ld, order, mstart, out);
    else
        model_mean_kernel<double><<<n_models, 256, 0, s>>>(static_cast<const double*>(x), n, dim, ld, order, mstart, out);
    return g_ierr.launch_ok("model_mean_kernel");
}

size_t xvec_ident_workspace_bytes(int64_t N, int64_t T, int32_t k) {
    if (!shape_ok(N, T) || k < 0 || k > kMaxK) return 0;
    const size_t open_set = N >= 2 ? make_open_set_plan(nullptr, N, T).total : 0;
    const size_t topk = k >= 1 ? make_topk_plan(nullptr, N, T, k).total : 0;
    return std::max<size_t>(std::max(open_set, topk), 256);      // never 0 for a shape that is served
}

int xvec_open_set_scores(const double* S, int64_t ld, int64_t N, int64_t T, double p_known, double* out, int64_t ld_out,
                         void* workspace, size_t workspace_bytes, xvec_stream stream) {
    if (N < 2) return g_ierr.fail(XVEC_ERR_ARG, "N = %lld: open-set scores need at least two models", (long long)N);
    if (T < 1) return g_ierr.fail(XVEC_ERR_ARG, "T = %lld: need at least one test column", (long long)T);
    if (N > kMaxDim || T > kMaxDim)
        return g_ierr.fail(XVEC_ERR_TOO_LARGE, "score matrix [%lld, %lld]: both sizes must be at most 2^31 - 1", (long long)N,
                           (long long)T);
    if (!(p_known > 0.0 && p_known <= 1.0)) return g_ierr.fail(XVEC_ERR_ARG, "p_known = %g must lie in (0, 1]", p_known);
    if (ld < T || ld_out < T)
        return g_ierr.fail(XVEC_ERR_ARG, "ld = %lld and ld_out = %lld must be at least T = %lld", (long long)ld, (long long)ld_out,
                           (long long)T);
    if (!S || !out) return g_ierr.fail(XVEC_ERR_ARG, "null pointer: S / out");
    if (out == S && ld_out != ld)
        return g_ierr.fail(XVEC_ERR_ARG, "in place (out == S) needs ld_out == ld (got %lld and %lld)", (long long)ld_out,
                           (long long)ld);
    const OpenSetPlan p = make_open_set_plan(workspace, N, T);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, p.total, g_ierr))) return rc;
    ColStatsArgs cs{};
    cs.S = S;
    cs.ld = ld;
    cs.N = N;
    cs.T = T;
    cs.col_tiles = (T + kCols - 1) / kCols;
    cs.row_blocks = p.row_blocks;
    const bool one = p.row_blocks == 1;
    cs.m = one ? p.m : p.pm;
    cs.R = one ? p.R : p.pR;
    cs.i = one ? p.i : p.pi;
    OpenSetArgs g{};
    g.S = S;
    g.out = out;
    g.ld = ld;
    g.ld_out = ld_out;
    g.N = N;
    g.T = T;
    g.col_tiles = (T + kApplyCols - 1) / kApplyCols;
    g.m = p.m;
    g.R = p.R;
    g.i = p.i;
    g.p = p_known;
    const int64_t stat_blocks = grid_blocks(p.row_blocks, cs.col_tiles);
    const int64_t tiles = grid_blocks((N + kApplyRows - 1) / kApplyRows, g.col_tiles);
    if (stat_blocks < 0 || tiles < 0)
        return g_ierr.fail(XVEC_ERR_TOO_LARGE, "%lld x %lld cells: more than 2^31 - 1 blocks", (long long)N, (long long)T);
    hipStream_t s = static_cast<hipStream_t>(stream);
    ident_col_stats_kernel<<<(unsigned)stat_blocks, kThreads, 0, s>>>(cs);
    if ((rc = g_ierr.launch_ok("ident_col_stats_kernel"))) return rc;
    if (!one) {
        ident_col_merge_kernel<<<(unsigned)((T + 255) / 256), 256, 0, s>>>(p.pm, p.pR, p.pi, p.row_blocks, T, p.m, p.R, p.i);
        if ((rc = g_ierr.launch_ok("ident_col_merge_kernel"))) return rc;
    }
    ident_open_set_kernel<<<(unsigned)tiles, kApplyCols, 0, s>>>(g);
    return g_ierr.launch_ok("ident_open_set_kernel");
}

int xvec_identify_topk(const double* S, int64_t ld, int64_t N, int64_t T, int32_t k, double threshold, int32_t* idx, double* val,
                       int32_t* decision, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    if (N < 1 || T < 1)
        return g_ierr.fail(XVEC_ERR_ARG, "score matrix [%lld, %lld]: need at least one model and one test column", (long long)N,
                           (long long)T);
    if (N > kMaxDim || T > kMaxDim)
        return g_ierr.fail(XVEC_ERR_TOO_LARGE, "score matrix [%lld, %lld]: both sizes must be at most 2^31 - 1", (long long)N,
                           (long long)T);
    if (k < 1 || k > kMaxK) return g_ierr.fail(XVEC_ERR_ARG, "k = %d must lie in 1 .. %d", k, kMaxK);
    if (ld < T) return g_ierr.fail(XVEC_ERR_ARG, "ld = %lld is smaller than T = %lld", (long long)ld, (long long)T);
    if (!S || !idx || !val) return g_ierr.fail(XVEC_ERR_ARG, "null pointer: S / idx / val");
    const TopkPlan p = make_topk_plan(workspace, N, T, k);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, p.total, g_ierr))) return rc;
    TopkArgs g{};
    g.S = S;
    g.ld = ld;
    g.N = N;
    g.T = T;
    g.col_tiles = (T + kCols - 1) / kCols;
    g.row_blocks = p.row_blocks;
    g.k = k;
    g.threshold = threshold;
    g.part_v = p.pv;
    g.part_i = p.pi;
    g.idx = idx;
    g.val = val;
    g.decision = decision;
    const int64_t blocks = grid_blocks(p.row_blocks, g.col_tiles);
    if (blocks < 0)
        return g_ierr.fail(XVEC_ERR_TOO_LARGE, "%lld x %lld cells: more than 2^31 - 1 blocks", (long long)N, (long long)T);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (p.kk) {
        case 1: return launch_topk<1>(g, (unsigned)blocks, s);
        case 4: return launch_topk<4>(g, (unsigned)blocks, s);
        default: return launch_topk<kMaxK>(g, (unsigned)blocks, s);
    }
}

}  // extern "C"
