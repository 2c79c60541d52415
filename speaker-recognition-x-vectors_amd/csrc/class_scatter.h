// Class statistics and centred scatter matrices in fp64: what xvec_plda_stats (plda_train.hip) and xvec_lda_stats (lda.hip)
// share.  The class-sum column walk and the class_start checks and upload (class_sums.h), the mean from the class sums, and
// the scatter kernel on v_mfma_f64_16x16x4_f64 with its slice plan, launch and reduce.
// Included INSIDE the including file's anonymous namespace, after host_support.h and tdnn_common.h: each translation unit
// instantiates its own kernels.
#pragma once

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- class sums, mean

#include "class_sums.h"      // class_rows, class_sum_columns

// mean[d] = (sum of the raw class sums) / n.  A block takes 16 columns; its 16 groups of 16 threads sum the classes
// c = g, g + 16, g + 32, .. of their column, and thread g = 0 adds the 16 group partials in group order (fixed order).
constexpr int kMeanCols = 16, kMeanGroups = 16;
__global__ __launch_bounds__(256) void stats_mean_kernel(const double* __restrict__ sums, int n_classes, int dim, int64_t n,
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

// ---------------------------------------------------------------- weighted centred scatter

// sum over rows i of w_i (x_i - centre_i)(x_i - centre_i)^T over the tiles on or above the diagonal of a (64 x 64)-tiled
// [dim, dim] grid, rows split into slices: block = (row slice, tile); it writes its 64 x 64 partial to slab[slice][tile], and
// class_scatter_reduce_kernel sums the slices in order and mirrors the result.  4 waves as 2 x 2, each 32 x 32 = 2 x 2 tiles
// of v_mfma_f64_16x16x4_f64 (A[i][k] = x[k][i]: both operands are read from row-major [k][column] LDS images, lane l takes
// k = l >> 4, column l & 15).  Rows in chunks of 16 through double-buffered LDS; the next chunk's global loads fly while the
// current one's 16 MFMAs per wave run.
//   PER_ROW = false: row i is x[i], every row centred by centre[0 .. dim) (read once into registers), weight 1; `order`,
//     `cls`, `wts` and `n_centres` are not read.  The two images of a diagonal tile are equal: one operand is staged.
//   PER_ROW = true: row i of the walk is x[order[i]] (order == nullptr: x[i]), centred by centre[cls[i]] (cls == nullptr:
//     centre[0]) and weighted by wts[cls[i]] (wts == nullptr: 1).  The weight goes into the A image only, so a diagonal tile
//     stages both images too; the reduce kernel reads the (i <= j) half of it.
constexpr int kTS = 64;        // tile edge
constexpr int kKC = 16;        // rows per chunk
constexpr int kLD = 80;        // LDS row stride in doubles (640 B): the four k rows of one ds_read_b64 land 128 B apart in the banks
constexpr int kScatterBlocks = 1024;   // slices x tiles aimed at: four blocks per CU on 256 CUs (fixed: results do not depend on the device)

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

// four consecutive elements from a 16-byte aligned address
template <typename T>
__device__ __forceinline__ void load_vec4(const T* p, T (&r)[4]) {
    if constexpr (sizeof(T) == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    } else {
        const f64x2 v0 = *reinterpret_cast<const f64x2*>(p);
        const f64x2 v1 = *reinterpret_cast<const f64x2*>(p + 2);
        r[0] = v0.x; r[1] = v0.y; r[2] = v1.x; r[3] = v1.y;
    }
}

template <typename T, bool VEC, bool PER_ROW>
__global__ __launch_bounds__(256, 4) void class_scatter_kernel(const ScatterArgs g) {
    __shared__ __attribute__((aligned(16))) double sA[2][kKC][kLD];
    __shared__ __attribute__((aligned(16))) double sB[2][kKC][kLD];
    const int logical = xcd_remap(blockIdx.x, gridDim.x);       // the tiles of one slice share an XCD's L2
    const int tile = logical % g.n_tri, slice = logical / g.n_tri;
    int tr, tc;
    tri_rc(tile, g.tiles, tr, tc);
    const bool diag = !PER_ROW && tr == tc;                     // A == B: one operand staged
    const int i0 = tr * kTS, j0 = tc * kTS;
    const int64_t row_begin = (int64_t)slice * g.rows_per_slice;
    const int64_t row_end = std::min<int64_t>(g.n, row_begin + g.rows_per_slice);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    const int lrow = tid >> 4, lcol = (tid & 15) * 4;            // staging: 16 rows x 64 columns, four columns a thread
    const T* __restrict__ x = static_cast<const T*>(g.x);

    bool va[4], vb[4];
    double ca[4], cb[4], wt = 1.0;       // the centre of the staged row at its columns of A and B; its weight
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        va[q] = i0 + lcol + q < g.dim;
        vb[q] = j0 + lcol + q < g.dim;
        if constexpr (!PER_ROW) {
            ca[q] = va[q] ? g.centre[i0 + lcol + q] : 0.0;
            cb[q] = vb[q] ? g.centre[j0 + lcol + q] : 0.0;
        }
    }
    T ra[4], rb[4];
    bool rvalid = false;
    auto gload = [&](int64_t r0) {
        const int64_t pos = r0 + lrow;
        rvalid = pos < row_end;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ra[q] = T(0);
            rb[q] = T(0);
            if constexpr (PER_ROW) {
                ca[q] = 0.0;
                cb[q] = 0.0;
            }
        }
        if (!rvalid) return;
        int64_t row = pos;
        if constexpr (PER_ROW) {
            if (g.order) row = (int64_t)g.order[pos];
            if (row < 0 || row >= g.n) {      // not a permutation: the row adds nothing
                rvalid = false;
                return;
            }
            const int c = g.cls ? std::min(std::max(g.cls[pos], 0), g.n_centres - 1) : 0;
            wt = g.wts ? g.wts[c] : 1.0;
            const double* m = g.centre + (int64_t)c * g.dim;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (va[q]) ca[q] = m[i0 + lcol + q];
                if (vb[q]) cb[q] = m[j0 + lcol + q];
            }
        }
        const T* p = x + row * g.dim;
        if constexpr (VEC) {            // dim % 4 == 0, 16-byte aligned base: the four columns are all in or all out
            if (va[0]) load_vec4(p + i0 + lcol, ra);
            if (!diag && vb[0]) load_vec4(p + j0 + lcol, rb);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (va[q]) ra[q] = p[i0 + lcol + q];
                if (!diag && vb[q]) rb[q] = p[j0 + lcol + q];
            }
        }
    };
    // centring (and the weight, on the A side) while staged; rows past the slice and columns past dim stay exactly zero
    auto lstore = [&](int buf) {
        double a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if constexpr (PER_ROW) a[q] = rvalid && va[q] ? ((double)ra[q] - ca[q]) * wt : 0.0;
            else a[q] = rvalid && va[q] ? (double)ra[q] - ca[q] : 0.0;
            b[q] = rvalid && vb[q] ? (double)rb[q] - cb[q] : 0.0;
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

// s[i, j] = s[j, i] = (sum over slices, in slice order, of the partials of (i, j), i <= j) / divisor (1.0: the sum itself)
__global__ __launch_bounds__(256) void class_scatter_reduce_kernel(const double* __restrict__ slab, int slices, int n_tri,
                                                                   int tiles, int dim, double divisor,
                                                                   double* __restrict__ s_out) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= dim || i > j) return;
    const int tr = i / kTS, tc = j / kTS;
    const int t = tr * tiles - tr * (tr - 1) / 2 + (tc - tr);
    const double* p = slab + (size_t)t * (kTS * kTS) + (i % kTS) * kTS + (j % kTS);
    const size_t stride = (size_t)n_tri * (kTS * kTS);
    double s = 0.0;
    for (int sl = 0; sl < slices; ++sl) s += p[sl * stride];
    const double v = s / divisor;
    s_out[(int64_t)i * dim + j] = v;
    s_out[(int64_t)j * dim + i] = v;      // the same bits: s == s^T exactly
}

// ---------------------------------------------------------------- host side

// Slices of one scatter product: as many as keep kScatterBlocks blocks busy, each worth at least `min_rows` rows and a whole
// number of chunks.
struct ScatterPlan {
    int slices;
    int64_t rows_per_slice;
};

inline ScatterPlan make_scatter_plan(int64_t rows, int n_tri, int min_rows) {
    ScatterPlan p{};
    const int64_t by_blocks = std::max<int64_t>(1, kScatterBlocks / n_tri);
    const int64_t by_rows = std::max<int64_t>(1, (rows + min_rows - 1) / min_rows);
    p.slices = (int)std::min(by_blocks, by_rows);
    p.rows_per_slice = ((rows + p.slices - 1) / p.slices + kKC - 1) / kKC * kKC;
    return p;
}

// One scatter product into s_out: g (x, n, the centres; dim, tiles, n_tri and slab set by the caller) over the slices of `plan`,
// then the reduce.
template <bool PER_ROW>
int launch_scatter(ScatterArgs g, bool x_is_f32, const ScatterPlan& plan, double divisor, double* s_out, hipStream_t s,
                   ErrorChannel& err) {
    g.rows_per_slice = plan.rows_per_slice;
    const unsigned grid = (unsigned)(plan.slices * g.n_tri);
    const bool vec = g.dim % 4 == 0 && reinterpret_cast<uintptr_t>(g.x) % 16 == 0;
    if (x_is_f32) {
        if (vec) class_scatter_kernel<float, true, PER_ROW><<<grid, 256, 0, s>>>(g);
        else class_scatter_kernel<float, false, PER_ROW><<<grid, 256, 0, s>>>(g);
    } else {
        if (vec) class_scatter_kernel<double, true, PER_ROW><<<grid, 256, 0, s>>>(g);
        else class_scatter_kernel<double, false, PER_ROW><<<grid, 256, 0, s>>>(g);
    }
    if (const int rc = err.launch_ok("class_scatter_kernel")) return rc;
    class_scatter_reduce_kernel<<<dim3((g.dim + 255) / 256, g.dim), 256, 0, s>>>(g.slab, plan.slices, g.n_tri, g.tiles, g.dim,
                                                                                divisor, s_out);
    return err.launch_ok("class_scatter_reduce_kernel");
}
