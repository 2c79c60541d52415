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

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- class sums, mean, class means

// One block per class: sums[c, :] = sum of the class's rows in `order` order (four interleaved partial sums per column,
// combined in a fixed order); cls[i] = c for the class's positions i of `order`, inv_n[c] = 1 / rows.  An entry of `order`
// outside [0, n) is only kept from reading out of bounds (include/xvec_lda.h: the outputs are then undefined).
template <typename T>
__global__ __launch_bounds__(256) void lda_class_sum_kernel(const T* __restrict__ x, int64_t n, int dim,
                                                            const int* __restrict__ order,
                                                            const int64_t* __restrict__ cstart, double* __restrict__ sums,
                                                            int* __restrict__ cls, double* __restrict__ inv_n) {
    const int c = blockIdx.x;
    const int64_t b = std::min<int64_t>(std::max<int64_t>(cstart[c], 0), n);
    const int64_t e = std::min<int64_t>(std::max<int64_t>(cstart[c + 1], b), n);
    if (threadIdx.x == 0) inv_n[c] = 1.0 / (double)(e - b);
    for (int64_t i = b + threadIdx.x; i < e; i += 256) cls[i] = c;
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

// mean[d] = (sum of the class sums) / n.  A block takes 16 columns; its 16 groups of 16 threads sum the classes
// c = g, g + 16, g + 32, .. of their column, and thread g = 0 adds the 16 group partials in group order.
constexpr int kMeanCols = 16, kMeanGroups = 16;
__global__ __launch_bounds__(256) void lda_mean_kernel(const double* __restrict__ sums, int n_classes, int dim, int64_t n,
                                                       double* __restrict__ mean) {
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

// sums[c, d] <- sums[c, d] / rows of class c: the class means, in place
__global__ __launch_bounds__(256) void lda_class_mean_kernel(double* __restrict__ sums, const int64_t* __restrict__ cstart,
                                                             int n_classes, int dim) {
    const int64_t idx = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (idx >= (int64_t)n_classes * dim) return;
    const int c = (int)(idx / dim);
    sums[idx] = sums[idx] / (double)(cstart[c + 1] - cstart[c]);
}

// ---------------------------------------------------------------- weighted centred scatter

// sum over rows i of w_i (x_i - centre_i)(x_i - centre_i)^T over the tiles on or above the diagonal of a (64 x 64)-tiled
// [dim, dim] grid, rows split into slices: block = (row slice, tile); it writes its 64 x 64 partial to slab[slice][tile], and
// lda_scatter_reduce_kernel sums the slices in order and mirrors the result.  The structure of plda_scatter_kernel
// (csrc/plda_train.hip): 4 waves as 2 x 2, each 32 x 32 = 2 x 2 tiles of v_mfma_f64_16x16x4_f64, both operands read from
// row-major [k][column] LDS images (lane l takes k = l >> 4, column l & 15), rows in chunks of 16 through double-buffered
// LDS.  What differs: row i of the walk is x[order[i]] (order == nullptr: x[i]), centred by centre[cls[i]] (cls == nullptr:
// centre[0]) and weighted by wts[cls[i]] (wts == nullptr: 1).  The weight goes into the A image only, so a diagonal tile
// stages both images too; the reduce kernel reads the (i <= j) half of it.
//   within-class:  x, order, cls, centre = class_means, wts = 1 / n_c
//   between-class: x = class_means (C rows), no order, centre = mean, no weights
constexpr int kTS = 64;        // tile edge
constexpr int kKC = 16;        // rows per chunk
constexpr int kLD = 80;        // LDS row stride in doubles (640 B): the four k rows of one ds_read_b64 land 128 B apart in the banks
constexpr int kScatterBlocks = 1024;   // slices x tiles aimed at: four blocks per CU on 256 CUs (fixed: results do not depend on the device)
constexpr int kSliceRows = 32;         // a slice is worth opening for this many rows

struct ScatterArgs {
    const void* x;
    const int* order;
    const int* cls;
    const double* centre;
    const double* wts;
    double* slab;
    int64_t n, rows_per_slice;
    int dim, tiles, n_tri, n_centres;
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
__global__ __launch_bounds__(256, 4) void lda_scatter_kernel(const ScatterArgs g) {
    __shared__ __attribute__((aligned(16))) double sA[2][kKC][kLD];
    __shared__ __attribute__((aligned(16))) double sB[2][kKC][kLD];
    const int logical = xcd_remap(blockIdx.x, gridDim.x);       // the tiles of one slice share an XCD's L2
    const int tile = logical % g.n_tri, slice = logical / g.n_tri;
    int tr, tc;
    tri_rc(tile, g.tiles, tr, tc);
    const int i0 = tr * kTS, j0 = tc * kTS;
    const int64_t row_begin = (int64_t)slice * g.rows_per_slice;
    const int64_t row_end = std::min<int64_t>(g.n, row_begin + g.rows_per_slice);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    const int lrow = tid >> 4, lcol = (tid & 15) * 4;            // staging: 16 rows x 64 columns, four columns a thread
    const T* __restrict__ x = static_cast<const T*>(g.x);

    bool va[4], vb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        va[q] = i0 + lcol + q < g.dim;
        vb[q] = j0 + lcol + q < g.dim;
    }
    T ra[4], rb[4];
    double ca[4], cb[4], wt = 1.0;
    bool rvalid = false;
    auto gload = [&](int64_t r0) {
        const int64_t pos = r0 + lrow;
        rvalid = pos < row_end;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ra[q] = T(0);
            rb[q] = T(0);
            ca[q] = 0.0;
            cb[q] = 0.0;
        }
        if (!rvalid) return;
        const int64_t row = g.order ? (int64_t)g.order[pos] : pos;
        if (row < 0 || row >= g.n) {      // not a permutation: the row adds nothing
            rvalid = false;
            return;
        }
        const int c = g.cls ? std::min(std::max(g.cls[pos], 0), g.n_centres - 1) : 0;
        wt = g.wts ? g.wts[c] : 1.0;
        const double* m = g.centre + (int64_t)c * g.dim;
        const T* p = x + row * g.dim;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (va[q]) ca[q] = m[i0 + lcol + q];
            if (vb[q]) cb[q] = m[j0 + lcol + q];
        }
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
            if (vb[0]) {
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
                if (vb[q]) rb[q] = p[j0 + lcol + q];
            }
        }
    };
    // centring (and the weight, on the A side) while staged; rows past the slice and columns past dim stay exactly zero
    auto lstore = [&](int buf) {
        double a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a[q] = rvalid && va[q] ? ((double)ra[q] - ca[q]) * wt : 0.0;
            b[q] = rvalid && vb[q] ? (double)rb[q] - cb[q] : 0.0;
        }
        *reinterpret_cast<f64x2*>(&sA[buf][lrow][lcol]) = f64x2{a[0], a[1]};
        *reinterpret_cast<f64x2*>(&sA[buf][lrow][lcol + 2]) = f64x2{a[2], a[3]};
        *reinterpret_cast<f64x2*>(&sB[buf][lrow][lcol]) = f64x2{b[0], b[1]};
        *reinterpret_cast<f64x2*>(&sB[buf][lrow][lcol + 2]) = f64x2{b[2], b[3]};
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
#pragma unroll
        for (int ks = 0; ks < kKC / 4; ++ks) {
            const int k = ks * 4 + l4;
            double a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = sA[buf][k][wr * 32 + i * 16 + l15];
                b[i] = sB[buf][k][wc * 32 + i * 16 + l15];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (ch + 1 < n_chunks) lstore(buf ^ 1);
        __syncthreads();
    }

    // C/D of the f64 MFMA: column lane & 15, row (lane >> 4) + 4 reg; 16 lanes write 128 contiguous bytes.  A slice
    // without rows writes zeros.
    double* out = g.slab + ((size_t)slice * g.n_tri + tile) * (kTS * kTS);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                out[(wr * 32 + i * 16 + l4 + 4 * r) * kTS + wc * 32 + j * 16 + l15] = acc[i][j][r];
}

// s[i, j] = s[j, i] = sum over slices, in slice order, of the partials of (i, j), i <= j
__global__ __launch_bounds__(256) void lda_scatter_reduce_kernel(const double* __restrict__ slab, int slices, int n_tri,
                                                                 int tiles, int dim, double* __restrict__ s_out) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= dim || i > j) return;
    const int tr = i / kTS, tc = j / kTS;
    const int t = tr * tiles - tr * (tr - 1) / 2 + (tc - tr);
    const double* p = slab + (size_t)t * (kTS * kTS) + (i % kTS) * kTS + (j % kTS);
    const size_t stride = (size_t)n_tri * (kTS * kTS);
    double s = 0.0;
    for (int sl = 0; sl < slices; ++sl) s += p[sl * stride];
    s_out[(int64_t)i * dim + j] = s;
    s_out[(int64_t)j * dim + i] = s;      // the same bits: s == s^T exactly
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

struct ScatterPlan {
    int slices;
    int64_t rows_per_slice;
};

ScatterPlan make_scatter_plan(int64_t rows, int n_tri) {
    ScatterPlan p{};
    const int64_t by_blocks = std::max<int64_t>(1, kScatterBlocks / n_tri);
    const int64_t by_rows = std::max<int64_t>(1, (rows + kSliceRows - 1) / kSliceRows);
    p.slices = (int)std::min(by_blocks, by_rows);
    p.rows_per_slice = ((rows + p.slices - 1) / p.slices + kKC - 1) / kKC * kKC;
    return p;
}

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
    p.within = make_scatter_plan(n, p.n_tri);
    p.between = make_scatter_plan(n_classes, p.n_tri);
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

template <typename T>
void launch_scatter(const ScatterArgs& g, unsigned grid, bool vec, hipStream_t s) {
    if (vec) lda_scatter_kernel<T, true><<<grid, 256, 0, s>>>(g);
    else lda_scatter_kernel<T, false><<<grid, 256, 0, s>>>(g);
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
    if (class_start_host[0] != 0 || class_start_host[n_classes] != n)
        return g_lerr.fail(XVEC_ERR_ARG, "class_start must run from 0 to n = %lld (got %lld .. %lld)", (long long)n,
                           (long long)class_start_host[0], (long long)class_start_host[n_classes]);
    for (int c = 0; c < n_classes; ++c)
        if (class_start_host[c + 1] <= class_start_host[c])
            return g_lerr.fail(XVEC_ERR_ARG, "class %d is empty or class_start decreases: every class needs a row", c);
    const StatsPlan p = make_stats_plan(workspace, n, dim, n_classes);
    int rc;
    if ((rc = workspace_ok(workspace_bytes, p.total, g_lerr))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(p.cstart, class_start_host, (size_t)(n_classes + 1) * sizeof(int64_t),
                                  hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return g_lerr.fail(XVEC_ERR_HIP, "class_start copy failed: %s", hipGetErrorString(e));
    if (x_dtype == XVEC_LDA_X_F32)
        lda_class_sum_kernel<float><<<n_classes, 256, 0, s>>>(static_cast<const float*>(x), n, dim, order, p.cstart,
                                                               class_means, p.cls, p.inv_n);
    else
        lda_class_sum_kernel<double><<<n_classes, 256, 0, s>>>(static_cast<const double*>(x), n, dim, order, p.cstart,
                                                                class_means, p.cls, p.inv_n);
    if ((rc = g_lerr.launch_ok("lda_class_sum_kernel"))) return rc;
    lda_mean_kernel<<<(dim + kMeanCols - 1) / kMeanCols, 256, 0, s>>>(class_means, n_classes, dim, n, mean);
    if ((rc = g_lerr.launch_ok("lda_mean_kernel"))) return rc;
    const int64_t cd = (int64_t)n_classes * dim;
    lda_class_mean_kernel<<<(unsigned)((cd + 255) / 256), 256, 0, s>>>(class_means, p.cstart, n_classes, dim);
    if ((rc = g_lerr.launch_ok("lda_class_mean_kernel"))) return rc;

    ScatterArgs g{};
    g.slab = p.slab;
    g.dim = dim;
    g.tiles = p.tiles;
    g.n_tri = p.n_tri;
    const dim3 rgrid((dim + 255) / 256, dim);
    // within-class: the rows of x through `order`, centred by their class mean, weighted by 1 / n_c
    g.x = x;
    g.order = order;
    g.cls = p.cls;
    g.centre = class_means;
    g.wts = p.inv_n;
    g.n = n;
    g.n_centres = n_classes;
    g.rows_per_slice = p.within.rows_per_slice;
    const bool vec = dim % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0;
    if (x_dtype == XVEC_LDA_X_F32) launch_scatter<float>(g, (unsigned)(p.within.slices * p.n_tri), vec, s);
    else launch_scatter<double>(g, (unsigned)(p.within.slices * p.n_tri), vec, s);
    if ((rc = g_lerr.launch_ok("lda_scatter_kernel (within)"))) return rc;
    lda_scatter_reduce_kernel<<<rgrid, 256, 0, s>>>(p.slab, p.within.slices, p.n_tri, p.tiles, dim, s_within);
    if ((rc = g_lerr.launch_ok("lda_scatter_reduce_kernel (within)"))) return rc;
    // between-class: the class means, centred by the mean, weight 1
    g.x = class_means;
    g.order = nullptr;
    g.cls = nullptr;
    g.centre = mean;
    g.wts = nullptr;
    g.n = n_classes;
    g.n_centres = 1;
    g.rows_per_slice = p.between.rows_per_slice;
    launch_scatter<double>(g, (unsigned)(p.between.slices * p.n_tri),
                           dim % 4 == 0 && reinterpret_cast<uintptr_t>(class_means) % 16 == 0, s);
    if ((rc = g_lerr.launch_ok("lda_scatter_kernel (between)"))) return rc;
    lda_scatter_reduce_kernel<<<rgrid, 256, 0, s>>>(p.slab, p.between.slices, p.n_tri, p.tiles, dim, s_between);
    return g_lerr.launch_ok("lda_scatter_reduce_kernel (between)");
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
