// GMM-UBM: diagonal-covariance EM, Baum-Welch statistics, relevance MAP and scores.  C ABI, the definitions and the summation
// order: include/xvec_gmm.h.  Plan, checks and layouts: gmm_plan.h.  The N x C posterior matrix is recomputed, never stored.
//   offsets    one block: the scan of the utterance counts
//   prepare    P = (mu / v, -0.5 / v) and g per component
//   lse        block = 64 frames: walks the component tiles, each ll tile on v_mfma_f64_16x16x4_f64 (X' and P chunks of 16 K
//              values through double-buffered LDS), an online (max, sum) per frame
//   gamma      block = (frame tile, component tile): the dense posteriors, for small C and for tests
//   sums       block = an utterance (or all frames): the sum of lse over, and the count of, the good frames
//   stats      block = (frame slice | utterance, component tile, column tile of (1, x, x^2)): per chunk of 64 frames the ll tile
//              again, gamma = exp(ll - lse) staged [frame][component] in LDS, then gamma^T . (1, x, x^2) on the same MFMA
//   reduce     the slices of the global form in rising order
//   mstep      weights (one block), then means and variances
//   em_*       the device's state of xvec_gmm_em: every kernel above returns at once when it says "stop"
//   map, super_model, super_test   relevance MAP and the supervectors of linear scoring and their product with a blocked sum over K
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/xvec_gmm.h"
#include "../../include/xvec_hip.h"
#include "gmm_plan.h"
#include "host_support.h"

namespace xvec {
namespace {

using namespace gmm_plan;

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kStage = 2 * 2 * kKC * kLD;        // doubles of the two double-buffered operand images; also gamma [64][kLD]
static_assert(kStage == kFT * kLD, "the gamma image takes the place of the staging buffers");
static_assert(kFT * (kCT + 1) <= kStage, "and so does the ll tile of the lse kernel");
static_assert(kFT == 64 && kCT == 64 && kYT == 64 && kThreads == 256, "4 waves as 2 x 2, each 32 x 32");

struct EmState {           // kEmStateBytes
    double prev;           // the lower bound of the iteration before
    int32_t stop;          // later iterations return at once
    int32_t n_iter;
};
static_assert(sizeof(EmState) <= kEmStateBytes, "gmm_plan.h: kEmStateBytes");

struct FrameArgs {
    const void* x;
    int64_t ldx, rows;
    const int64_t* first;  // [U]
    const int64_t* off;    // [U + 1]: frames before utterance u
    int64_t n_utts, n_total;
};

__device__ __forceinline__ bool stopped(const int32_t* stop) { return stop && *stop; }

// the row of frame j (0 <= j < n_total): the last utterance u with off[u] <= j holds it
__device__ __forceinline__ int64_t row_of(const FrameArgs& fa, int64_t j) {
    int64_t lo = 0, hi = fa.n_utts;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (fa.off[mid] <= j) lo = mid;
        else hi = mid;
    }
    return fa.first[lo] + (j - fa.off[lo]);
}

// fixed tree over the 256 threads of a block; every thread gets the sum.  buf: 256 elements of LDS.
template <typename V>
__device__ __forceinline__ V block_tree(V v, V* buf) {
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) buf[threadIdx.x] += buf[threadIdx.x + s];
        __syncthreads();
    }
    const V r = buf[0];
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------- utterance offsets

// one block: off[0 .. U) holds the counts and becomes, in place, the frames before each utterance; off[U] the total.  Thread i
// scans the utterances [i per, (i + 1) per).
__global__ __launch_bounds__(256) void gmm_offsets_kernel(int64_t U, int64_t* __restrict__ off) {
    __shared__ int64_t part[kThreads];
    const int64_t per = (U + kThreads - 1) / kThreads;
    const int64_t b = std::min<int64_t>(U, per * threadIdx.x), e = std::min<int64_t>(U, b + per);
    int64_t s = 0;
    for (int64_t u = b; u < e; ++u) s += off[u];
    part[threadIdx.x] = s;
    __syncthreads();
    int64_t before = 0;
    for (int t = 0; t < (int)threadIdx.x; ++t) before += part[t];
    for (int64_t u = b; u < e; ++u) {
        const int64_t n = off[u];
        off[u] = before;
        before += n;
    }
    if (threadIdx.x == kThreads - 1) off[U] = before;      // (its range ends at U: it holds the total)
}

// ---------------------------------------------------------------- the prepared model

__global__ __launch_bounds__(256) void gmm_prepare_kernel(const double* __restrict__ w, const double* __restrict__ mu,
                                                          const double* __restrict__ v, int C, int D, double* __restrict__ P,
                                                          double* __restrict__ g, const int32_t* stop) {
    if (stopped(stop)) return;
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    double logdet = 0.0, quad = 0.0;
    for (int d = 0; d < D; ++d) {
        const double m = mu[(int64_t)c * D + d], var = v[(int64_t)c * D + d];
        P[(int64_t)c * 2 * D + d] = m / var;
        P[(int64_t)c * 2 * D + D + d] = -0.5 / var;
        logdet += log(var);
        quad += m * m / var;
    }
    g[c] = log(w[c]) - 0.5 * ((double)D * 1.8378770664093453 + logdet + quad);      // log(2 pi)
}

// ---------------------------------------------------------------- one 64 x 64 tile of a product over K

// acc[i][j][r] = sum over k < K of a(col_a, k) b(col_b, k) for the 64 x 64 pairs of a block: row wr 32 + i 16 + (lane >> 4) + 4 r
// of the A side, column wc 32 + j 16 + (lane & 15) of the B side.  load_a(col, k) / load_b(col, k) give the operands' values (0
// for what is not there; they are asked for k < K only).  Staging: a wave takes four K values of all 64 columns; chunks of kKC
// through the two double-buffered images in `stage` (kStage doubles of LDS), the next chunk's loads in flight while the
// current one's 16 MFMAs per wave run.  K runs in rising chunks whatever the tile: the same operands give the same bits in
// every kernel.  BLOCK = 0: one running sum.  BLOCK > 0: BLOCK terms are added into `run`, `run` then into `acc` -- the longest
// chain of additions is BLOCK + K / BLOCK long, not K.  Ends behind a __syncthreads: the staging buffers are free.
template <int BLOCK, typename LoadA, typename LoadB>
__device__ __forceinline__ void tile_product(LoadA load_a, LoadB load_b, int64_t K, double* stage, f64x4 (&acc)[2][2]) {
    static_assert(BLOCK % kKC == 0, "a block of the sum is a whole number of chunks");
    double(*sA)[kKC][kLD] = reinterpret_cast<double(*)[kKC][kLD]>(stage);
    double(*sB)[kKC][kLD] = reinterpret_cast<double(*)[kKC][kLD]>(stage + 2 * kKC * kLD);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    const int col = tid & 63, kq = (tid >> 6) * 4;
    double ra[4], rb[4];
    auto gload = [&](int64_t k0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t kk = k0 + kq + q;
            ra[q] = kk < K ? load_a(col, kk) : 0.0;
            rb[q] = kk < K ? load_b(col, kk) : 0.0;
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            sA[buf][kq + q][col] = ra[q];
            sB[buf][kq + q][col] = rb[q];
        }
    };
    f64x4 run[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = run[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int64_t n_chunks = (K + kKC - 1) / kKC;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int64_t ch = 0; ch < n_chunks; ++ch) {
        const int buf = (int)(ch & 1);
        if (ch + 1 < n_chunks) gload((ch + 1) * kKC);
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
                for (int j = 0; j < 2; ++j) {
                    if constexpr (BLOCK > 0) run[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], run[i][j], 0, 0, 0);
                    else acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
                }
        }
        if constexpr (BLOCK > 0) {
            if ((ch + 1) % (BLOCK / kKC) == 0 || ch + 1 == n_chunks) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        acc[i][j] += run[i][j];
                        run[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
                    }
            }
        }
        if (ch + 1 < n_chunks) lstore(buf ^ 1);
        __syncthreads();
    }
}

// The ll tile: X' . P^T.  srow [64] (LDS): the row of each frame of the tile, -1 for none (its X' is zeros); the squares are
// taken in fp64 from the widened value; components from c0, zeros past C.
template <typename T>
__device__ __forceinline__ void ll_tile(const T* __restrict__ x, int64_t ldx, const int64_t* srow, const double* __restrict__ P,
                                        int C, int D, int c0, double* stage, f64x4 (&acc)[2][2]) {
    auto load_x = [&](int col, int64_t k) -> double {
        const int64_t row = srow[col];
        if (row < 0) return 0.0;
        const double t = (double)x[row * ldx + (k < D ? k : k - D)];
        return k < D ? t : t * t;
    };
    auto load_p = [&](int col, int64_t k) -> double { return c0 + col < C ? P[(int64_t)(c0 + col) * 2 * D + k] : 0.0; };
    tile_product<0>(load_x, load_p, (int64_t)2 * D, stage, acc);
}

// ---------------------------------------------------------------- pass 1: lse

template <typename T>
__global__ __launch_bounds__(256) void gmm_lse_kernel(const FrameArgs fa, const double* __restrict__ P, const double* __restrict__ g,
                                                      int C, int D, double* __restrict__ lse, const int32_t* stop) {
    if (stopped(stop)) return;
    __shared__ __attribute__((aligned(16))) double stage[kStage];
    __shared__ int64_t srow[kFT];
    __shared__ double sm[kFT][4], ss[kFT][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    const int64_t j0 = (int64_t)blockIdx.x * kFT;
    if (tid < kFT) srow[tid] = j0 + tid < fa.n_total ? row_of(fa, j0 + tid) : -1;
    __syncthreads();
    double(*sLL)[kCT + 1] = reinterpret_cast<double(*)[kCT + 1]>(stage);
    const int fr = tid >> 2, q = tid & 3;               // the online pair of frame fr over the components (c % 64) / 16 == q
    double m = -INFINITY, s = 0.0;
    const int tiles = (C + kCT - 1) / kCT;
    for (int ct = 0; ct < tiles; ++ct) {
        const int c0 = ct * kCT;
        f64x4 acc[2][2];
        ll_tile(static_cast<const T*>(fa.x), fa.ldx, srow, P, C, D, c0, stage, acc);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int comp = wc * 32 + j * 16 + l15;
                const double gc = c0 + comp < C ? g[c0 + comp] : -INFINITY;
#pragma unroll
                for (int r = 0; r < 4; ++r) sLL[wr * 32 + i * 16 + l4 + 4 * r][comp] = acc[i][j][r] + gc;
            }
        __syncthreads();
        double t[16], tm = -INFINITY;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            t[c] = sLL[fr][q * 16 + c];
            tm = t[c] > tm ? t[c] : tm;               // (a NaN never wins: it reaches the sum below)
        }
        const double mn = tm > m ? tm : m;
        if (mn != -INFINITY) {
            double add = 0.0;
#pragma unroll
            for (int c = 0; c < 16; ++c) add += exp(t[c] - mn);
            s = (m == -INFINITY ? s : s * exp(m - mn)) + add;          // (with m = -inf, s is 0 or the NaN met so far)
            m = mn;
        } else {
#pragma unroll
            for (int c = 0; c < 16; ++c) s += t[c] != t[c] ? t[c] : 0.0;      // all -inf or NaN: the NaN must show
        }
        __syncthreads();
    }
    sm[fr][q] = m;
    ss[fr][q] = s;
    __syncthreads();
    if (tid < kFT && j0 + tid < fa.n_total) {
        double M = -INFINITY;
        for (int p = 0; p < 4; ++p) M = sm[tid][p] > M ? sm[tid][p] : M;
        double S = 0.0;
        for (int p = 0; p < 4; ++p) {
            const double mp = sm[tid][p], sp = ss[tid][p];
            S += mp == -INFINITY ? sp : sp * exp(mp - M);          // (sp is 0, or the NaN of an all-NaN group)
        }
        lse[j0 + tid] = M == -INFINITY ? (S != S ? S : -INFINITY) : M + log(S);
    }
}

// ---------------------------------------------------------------- the dense posteriors

template <typename T>
__global__ __launch_bounds__(256) void gmm_gamma_kernel(const FrameArgs fa, const double* __restrict__ P, const double* __restrict__ g,
                                                        int C, int D, const double* __restrict__ lse, double* __restrict__ gamma) {
    __shared__ __attribute__((aligned(16))) double stage[kStage];
    __shared__ int64_t srow[kFT];
    __shared__ double slse[kFT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    const int64_t j0 = (int64_t)blockIdx.x * kFT;
    const int c0 = blockIdx.y * kCT;
    if (tid < kFT) {
        const int64_t j = j0 + tid;
        const double l = j < fa.n_total ? lse[j] : NAN;
        const bool good = l - l == 0.0;
        srow[tid] = good ? row_of(fa, j) : -1;
        slse[tid] = l;
    }
    __syncthreads();
    f64x4 acc[2][2];
    ll_tile(static_cast<const T*>(fa.x), fa.ldx, srow, P, C, D, c0, stage, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = c0 + wc * 32 + j * 16 + l15;
            if (c >= C) continue;
            const double gc = g[c];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = wr * 32 + i * 16 + l4 + 4 * r;
                if (j0 + f < fa.n_total) gamma[(j0 + f) * C + c] = srow[f] >= 0 ? exp(acc[i][j][r] + gc - slse[f]) : 0.0;
            }
        }
}

// ---------------------------------------------------------------- sums of lse

// block u: the frames [off[u], off[u + 1]) (all == 0), or all frames as one (all != 0, one block, which WRITES n_bad -- a
// memset in front of it would not be behind the stop flag and would wipe the count of the last iteration run); with all == 0
// the blocks add to n_bad, which the caller has cleared.
__global__ __launch_bounds__(256) void gmm_sums_kernel(const double* __restrict__ lse, const int64_t* __restrict__ off, int64_t n_total,
                                                       int all, double* __restrict__ llsum, int64_t* __restrict__ n_frames,
                                                       unsigned long long* __restrict__ n_bad, const int32_t* stop) {
    if (stopped(stop)) return;
    __shared__ double sd[kThreads];
    __shared__ int64_t si[kThreads];
    const int64_t b = all ? 0 : off[blockIdx.x], e = all ? n_total : off[blockIdx.x + 1];
    double s = 0.0;
    int64_t good = 0, bad = 0;
    for (int64_t j = b + threadIdx.x; j < e; j += kThreads) {
        const double l = lse[j];
        if (l - l == 0.0) {
            s += l;
            ++good;
        } else {
            ++bad;
        }
    }
    s = block_tree(s, sd);
    good = block_tree(good, si);
    bad = block_tree(bad, si);
    if (threadIdx.x == 0) {
        llsum[blockIdx.x] = s;
        n_frames[blockIdx.x] = good;
        if (all) *n_bad = (unsigned long long)bad;
        else if (bad) atomicAdd(n_bad, (unsigned long long)bad);
    }
}

// ---------------------------------------------------------------- pass 2: the statistics

struct StatArgs {
    FrameArgs fa;
    const double* P;
    const double* g;
    const double* lse;
    double* slab;          // global form
    double* n;             // per-utterance form
    double* f;
    int64_t slice_frames;
    int C, D, ctiles, ytiles;
    const int32_t* stop;
};

template <typename T, bool PER_UTT>
__global__ __launch_bounds__(256) void gmm_stats_kernel(const StatArgs a) {
    if (stopped(a.stop)) return;
    __shared__ __attribute__((aligned(16))) double stage[kStage];
    __shared__ __attribute__((aligned(16))) double sY[kFT / 2][kLD];
    __shared__ int64_t srow[kFT];
    __shared__ double slse[kFT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    const int part = blockIdx.x;                               // slice or utterance
    const int c0 = blockIdx.y * kCT, y0 = blockIdx.z * kYT;
    const int C = a.C, D = a.D;
    const int W = PER_UTT ? 1 + D : 1 + 2 * D;
    int64_t begin, end;
    if constexpr (PER_UTT) {
        begin = a.fa.off[part];
        end = a.fa.off[part + 1];
    } else {
        begin = std::min<int64_t>(a.fa.n_total, (int64_t)part * a.slice_frames);
        end = std::min<int64_t>(a.fa.n_total, begin + a.slice_frames);
    }
    const T* __restrict__ x = static_cast<const T*>(a.fa.x);
    double(*sG)[kLD] = reinterpret_cast<double(*)[kLD]>(stage);
    f64x4 out[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) out[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

    for (int64_t j0 = begin; j0 < end; j0 += kFT) {
        if (tid < kFT) {
            const int64_t j = j0 + tid;
            const double l = j < end ? a.lse[j] : NAN;
            const bool good = l - l == 0.0;                    // a bad frame adds nothing: its X' and its (1, x, x^2) are zeros
            srow[tid] = good ? row_of(a.fa, j) : -1;
            slse[tid] = l;
        }
        __syncthreads();
        f64x4 acc[2][2];
        ll_tile(x, a.fa.ldx, srow, a.P, C, D, c0, stage, acc);
        // gamma [frame][component], by selection 0 for a frame that is not there and a component past C
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int comp = wc * 32 + j * 16 + l15;
                const bool in = c0 + comp < C;
                const double gc = in ? a.g[c0 + comp] : 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = wr * 32 + i * 16 + l4 + 4 * r;
                    sG[f][comp] = in && srow[f] >= 0 ? exp(acc[i][j][r] + gc - slse[f]) : 0.0;
                }
            }
        for (int half = 0; half < 2; ++half) {
            // (1, x, x^2) of 32 frames, 64 columns from y0: thread = (frame, 8 columns)
            {
                const int fl = tid >> 3, cg = (tid & 7) * 8;
                const int64_t row = srow[half * 32 + fl];
                const T* __restrict__ xr = x + (row < 0 ? 0 : row) * a.fa.ldx;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int y = y0 + cg + q;
                    double val = 0.0;
                    if (row >= 0 && y < W) {
                        if (y == 0) val = 1.0;
                        else {
                            const double t = (double)xr[y <= D ? y - 1 : y - 1 - D];
                            val = y <= D ? t : t * t;
                        }
                    }
                    sY[fl][cg + q] = val;
                }
            }
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < kFT / 2 / 4; ++ks) {
                const int k = ks * 4 + l4;
                double ga[2], yb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    ga[i] = sG[half * 32 + k][wr * 32 + i * 16 + l15];
                    yb[i] = sY[k][wc * 32 + i * 16 + l15];
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) out[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[i], yb[j], out[i][j], 0, 0, 0);
            }
            __syncthreads();
        }
    }
    // out[i][j][r]: component wr 32 + i 16 + (lane >> 4) + 4 r, column wc 32 + j 16 + (lane & 15)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int comp = wr * 32 + i * 16 + l4 + 4 * r, ycol = wc * 32 + j * 16 + l15;
                if constexpr (PER_UTT) {
                    const int c = c0 + comp, y = y0 + ycol;
                    if (c < C && y < W) {
                        if (y == 0) a.n[(int64_t)part * C + c] = out[i][j][r];
                        else a.f[((int64_t)part * C + c) * D + (y - 1)] = out[i][j][r];
                    }
                } else {
                    double* tile = a.slab + (((size_t)part * a.ctiles + blockIdx.y) * a.ytiles + blockIdx.z) * (kCT * kYT);
                    tile[comp * kYT + ycol] = out[i][j][r];
                }
            }
}

// n, f, s = the slices' partials added in rising order; thread = (component, column of (1, x, x^2))
__global__ __launch_bounds__(256) void gmm_reduce_kernel(const double* __restrict__ slab, int slices, int ctiles, int ytiles, int C, int D,
                                                         double* __restrict__ n, double* __restrict__ f, double* __restrict__ s,
                                                         const int32_t* stop) {
    if (stopped(stop)) return;
    const int W = 1 + 2 * D;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (int64_t)C * W) return;
    const int c = (int)(i / W), y = (int)(i % W);
    const double* p = slab + ((size_t)(c / kCT) * ytiles + y / kYT) * (kCT * kYT) + (c % kCT) * kYT + y % kYT;
    const size_t stride = (size_t)ctiles * ytiles * (kCT * kYT);
    double t = 0.0;
    for (int sl = 0; sl < slices; ++sl) t += p[sl * stride];
    if (y == 0) n[c] = t;
    else if (y <= D) f[(int64_t)c * D + (y - 1)] = t;
    else s[(int64_t)c * D + (y - 1 - D)] = t;
}

// ---------------------------------------------------------------- M-step

// one block: nk = n + 10 eps, w = (nk / N) / sum_c (nk / N); the sum as thread i's c = i, i + 256, .. and a fixed tree
__global__ __launch_bounds__(256) void gmm_mstep_weights_kernel(const double* __restrict__ n, const int64_t* __restrict__ n_frames, int C,
                                                                double* __restrict__ w, const int32_t* stop) {
    if (stopped(stop)) return;
    __shared__ double sd[kThreads];
    const double N = (double)*n_frames;
    double t = 0.0;
    for (int c = threadIdx.x; c < C; c += kThreads) t += (n[c] + 10.0 * 2.220446049250313e-16) / N;
    const double sum = block_tree(t, sd);
    for (int c = threadIdx.x; c < C; c += kThreads) w[c] = (n[c] + 10.0 * 2.220446049250313e-16) / N / sum;
}

__global__ __launch_bounds__(256) void gmm_mstep_moments_kernel(const double* __restrict__ n, const double* __restrict__ f,
                                                                const double* __restrict__ s, int C, int D, double reg_covar,
                                                                double var_floor, double min_count, double* __restrict__ mu,
                                                                double* __restrict__ v, const int32_t* stop) {
    if (stopped(stop)) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (int64_t)C * D) return;
    const double nc = n[i / D];
    if (nc < min_count) return;
    const double nk = nc + 10.0 * 2.220446049250313e-16;
    const double m = f[i] / nk;
    const double var = s[i] / nk - m * m + reg_covar;
    mu[i] = m;
    v[i] = var > var_floor ? var : var_floor;
}

// ---------------------------------------------------------------- the EM's state

__global__ void gmm_em_init_kernel(EmState* st, double* lower_bound, int max_iter, int32_t* n_iter_done) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < max_iter) lower_bound[i] = NAN;
    if (i == 0) {
        st->prev = -INFINITY;
        st->stop = 0;
        st->n_iter = 0;
        *n_iter_done = 0;
    }
}

// after the M-step of iteration it: the lower bound of its E-step and the stopping test
__global__ void gmm_em_check_kernel(EmState* st, const double* sums_ll, const int64_t* sums_n, int it, double tol, double* lower_bound,
                                    int32_t* n_iter_done) {
    if (st->stop) return;
    const double lb = *sums_ll / (double)*sums_n;
    lower_bound[it] = lb;
    st->n_iter = it + 1;
    *n_iter_done = it + 1;
    const double change = lb - st->prev;
    if (fabs(change) < tol) st->stop = 1;
    st->prev = lb;
}

// ---------------------------------------------------------------- MAP and the supervectors

__global__ __launch_bounds__(256) void gmm_map_kernel(const double* __restrict__ n, const double* __restrict__ f, const double* __restrict__ mu,
                                                      int64_t total, int C, int D, double relevance, double* __restrict__ mu_hat) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int64_t cd = i % ((int64_t)C * D);
    const double nc = n[i / D], m = mu[cd];
    double r = m;
    if (nc > 0.0) {
        const double alpha = nc / (nc + relevance);
        r = alpha * (f[i] / nc) + (1.0 - alpha) * m;
    }
    mu_hat[i] = r;
}

__global__ __launch_bounds__(256) void gmm_super_model_kernel(const double* __restrict__ mu_hat, const double* __restrict__ mu,
                                                              const double* __restrict__ v, int64_t total, int64_t CD,
                                                              double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int64_t cd = i % CD;
    out[i] = (mu_hat[i] - mu[cd]) / v[cd];
}

// block u: (f - n mu) / sum_c n, the sum as thread i's c = i, i + 256, .. and a fixed tree; zeros where the sum is 0
__global__ __launch_bounds__(256) void gmm_super_test_kernel(const double* __restrict__ n, const double* __restrict__ f,
                                                             const double* __restrict__ mu, int C, int D, double* __restrict__ out) {
    __shared__ double sd[kThreads];
    const int64_t u = blockIdx.x;
    double t = 0.0;
    for (int c = threadIdx.x; c < C; c += kThreads) t += n[u * C + c];
    const double sum = block_tree(t, sd);
    const int64_t CD = (int64_t)C * D;
    for (int64_t i = threadIdx.x; i < CD; i += kThreads)
        out[u * CD + i] = sum > 0.0 ? (f[u * CD + i] - n[u * C + i / D] * mu[i]) / sum : 0.0;
}

// S[m, u] = sum_k A[m, k] B[u, k] over the supervectors; block = a 64 x 64 tile of S.  The sum over K = C D, thousands of terms,
// is blocked (tile_product<kScoreBlock>): the scores are held to a bar of a few ulps, which a single running sum of that length
// does not keep.  The order is fixed.
constexpr int kScoreBlock = 32;

__global__ __launch_bounds__(256) void gmm_scores_kernel(const double* __restrict__ A, const double* __restrict__ B, int64_t M, int64_t U,
                                                         int64_t K, double* __restrict__ S, int64_t ld_s) {
    __shared__ __attribute__((aligned(16))) double stage[kStage];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    const int64_t u_tiles = (U + kCT - 1) / kCT;
    const int64_t m0 = (int64_t)blockIdx.x / u_tiles * kFT, u0 = (int64_t)blockIdx.x % u_tiles * kCT;
    auto load_a = [&](int col, int64_t k) -> double { return m0 + col < M ? A[(m0 + col) * K + k] : 0.0; };
    auto load_b = [&](int col, int64_t k) -> double { return u0 + col < U ? B[(u0 + col) * K + k] : 0.0; };
    f64x4 acc[2][2];
    tile_product<kScoreBlock>(load_a, load_b, K, stage, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t m = m0 + wr * 32 + i * 16 + l4 + 4 * r, u = u0 + wc * 32 + j * 16 + l15;
                if (m < M && u < U) S[m * ld_s + u] = acc[i][j][r];
            }
}

// ================================================================ host

thread_local ErrorChannel g_gerr;

int refused(const Refusal& why) { return g_gerr.refused(XVEC_ERR_ARG, why); }

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// the utterances onto the device: utt_first as it is, utt_count into the slots of the offsets, scanned there in place
int put_frames(const xvec_gmm_frames* fr, int64_t n_total, void* ws, const Layout& l, FrameArgs& fa, hipStream_t s) {
    int64_t* first = part<int64_t>(ws, l.first);
    int64_t* off = part<int64_t>(ws, l.off);
    int rc;
    if ((rc = upload(first, fr->utt_first, (size_t)fr->n_utts, "utt_first", s, g_gerr))) return rc;
    if ((rc = upload(off, fr->utt_count, (size_t)fr->n_utts, "utt_count", s, g_gerr))) return rc;
    gmm_offsets_kernel<<<1, kThreads, 0, s>>>(fr->n_utts, off);
    if ((rc = g_gerr.launch_ok("gmm_offsets_kernel"))) return rc;
    fa.x = fr->x;
    fa.ldx = fr->ldx;
    fa.rows = fr->rows;
    fa.first = first;
    fa.off = off;
    fa.n_utts = fr->n_utts;
    fa.n_total = n_total;
    return XVEC_OK;
}

int prepare(const double* w, const double* mu, const double* v, int C, int D, double* P, double* g, const int32_t* stop, hipStream_t s) {
    gmm_prepare_kernel<<<blocks_for(C), kThreads, 0, s>>>(w, mu, v, C, D, P, g, stop);
    return g_gerr.launch_ok("gmm_prepare_kernel");
}

int run_lse(const FrameArgs& fa, bool f32, const double* P, const double* g, int C, int D, double* lse, const int32_t* stop, hipStream_t s) {
    if (fa.n_total == 0) return XVEC_OK;
    const unsigned grid = (unsigned)frame_tiles(fa.n_total);
    if (f32) gmm_lse_kernel<float><<<grid, kThreads, 0, s>>>(fa, P, g, C, D, lse, stop);
    else gmm_lse_kernel<double><<<grid, kThreads, 0, s>>>(fa, P, g, C, D, lse, stop);
    return g_gerr.launch_ok("gmm_lse_kernel");
}

int clear_bad(int64_t* n_bad, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(n_bad, 0, sizeof(int64_t), s);
    return e == hipSuccess ? XVEC_OK : g_gerr.fail(XVEC_ERR_HIP, "clearing n_bad failed: %s", hipGetErrorString(e));
}

// E-step of the global form on a prepared model: lse, the sums, the statistics into n, f, s
int run_global(const FrameArgs& fa, bool f32, void* ws, const Layout& l, int C, int D, double* n, double* f, double* sq, double* llsum,
               int64_t* n_frames, int64_t* n_bad, const int32_t* stop, hipStream_t s) {
    const double* P = part<double>(ws, l.P);
    const double* g = part<double>(ws, l.g);
    double* lse = part<double>(ws, l.lse);
    int rc;
    if ((rc = run_lse(fa, f32, P, g, C, D, lse, stop, s))) return rc;
    gmm_sums_kernel<<<1, kThreads, 0, s>>>(lse, fa.off, fa.n_total, 1, llsum, n_frames, reinterpret_cast<unsigned long long*>(n_bad), stop);
    if ((rc = g_gerr.launch_ok("gmm_sums_kernel"))) return rc;
    StatArgs a{};
    a.fa = fa;
    a.P = P;
    a.g = g;
    a.lse = lse;
    a.slab = part<double>(ws, l.slab);
    a.slice_frames = slice_frames(fa.n_total, l.slices);
    a.C = C;
    a.D = D;
    a.ctiles = comp_tiles(C);
    a.ytiles = y_tiles(D, false);
    a.stop = stop;
    const dim3 grid((unsigned)l.slices, (unsigned)a.ctiles, (unsigned)a.ytiles);
    if (f32) gmm_stats_kernel<float, false><<<grid, kThreads, 0, s>>>(a);
    else gmm_stats_kernel<double, false><<<grid, kThreads, 0, s>>>(a);
    if ((rc = g_gerr.launch_ok("gmm_stats_kernel"))) return rc;
    gmm_reduce_kernel<<<blocks_for((int64_t)C * (1 + 2 * D)), kThreads, 0, s>>>(a.slab, l.slices, a.ctiles, a.ytiles, C, D, n, f, sq, stop);
    return g_gerr.launch_ok("gmm_reduce_kernel");
}

int run_mstep(const double* n, const double* f, const double* sq, const int64_t* n_frames, int C, int D, const xvec_gmm_mstep_options& o,
              double* w, double* mu, double* v, const int32_t* stop, hipStream_t s) {
    gmm_mstep_weights_kernel<<<1, kThreads, 0, s>>>(n, n_frames, C, w, stop);
    if (const int rc = g_gerr.launch_ok("gmm_mstep_weights_kernel")) return rc;
    gmm_mstep_moments_kernel<<<blocks_for((int64_t)C * D), kThreads, 0, s>>>(n, f, sq, C, D, o.reg_covar, o.var_floor, o.min_count, mu, v, stop);
    return g_gerr.launch_ok("gmm_mstep_moments_kernel");
}

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_gmm_last_error(void) { return g_gerr.c_str(); }

int xvec_gmm_plan_host(int64_t n_total, int64_t n_utts, int32_t C, int32_t D, int32_t per_utt, int32_t n_slices, int64_t* out) {
    Refusal why;
    if (check_plan_query(n_total, n_utts, C, D, per_utt, n_slices, out, why)) return refused(why);
    const int32_t slices = per_utt ? 0 : slices_of(n_total, C, D, n_slices);
    out[0] = kFT;
    out[1] = kCT;
    out[2] = comp_tiles(C);
    out[3] = y_tiles(D, per_utt != 0);
    out[4] = slices;
    out[5] = per_utt ? 0 : slice_frames(n_total, slices);
    out[6] = k_pad(D);
    out[7] = k_chunks(D);
    out[8] = per_utt ? 0 : (int64_t)slab_doubles(C, D, slices);
    out[9] = (per_utt ? n_utts : (int64_t)slices) * out[2] * out[3];
    return XVEC_OK;
}

size_t xvec_gmm_loglik_workspace_bytes(int64_t n_utts, int32_t C, int32_t D) { return loglik_layout(n_utts, C, D).total; }

size_t xvec_gmm_accumulate_workspace_bytes(int64_t n_total, int64_t n_utts, int32_t C, int32_t D, int32_t per_utt, int32_t n_slices) {
    return accumulate_layout(n_total, n_utts, C, D, per_utt, n_slices).total;
}

size_t xvec_gmm_em_workspace_bytes(int64_t n_total, int64_t n_utts, int32_t C, int32_t D, int32_t n_slices) {
    return em_layout(n_total, n_utts, C, D, n_slices).total;
}

size_t xvec_gmm_linear_scores_workspace_bytes(int64_t M, int64_t U, int32_t C, int32_t D) { return score_layout(M, U, C, D).total; }

int xvec_gmm_prepare(const double* w, const double* mu, const double* v, const double* mu_override, int32_t C, int32_t D, double* P,
                     double* g, xvec_stream stream) {
    Refusal why;
    if (check_model(C, D, why)) return refused(why);
    if (!w || !mu || !v || !P || !g) return g_gerr.fail(XVEC_ERR_ARG, "null pointer: w / mu / v / P / g");
    return prepare(w, mu_override ? mu_override : mu, v, C, D, P, g, nullptr, static_cast<hipStream_t>(stream));
}

int xvec_gmm_loglik(const xvec_gmm_frames* frames, const double* w, const double* mu, const double* v, const double* mu_override,
                    int32_t C, int32_t D, double* lse, double* utt_llsum, int64_t* utt_frames, int64_t* n_bad, double* gamma,
                    void* workspace, size_t workspace_bytes, xvec_stream stream) {
    Refusal why;
    int64_t n_total = 0;
    if (check_model(C, D, why) || check_frames(frames, D, &n_total, why)) return refused(why);
    if (!w || !mu || !v) return g_gerr.fail(XVEC_ERR_ARG, "null pointer: w / mu / v");
    if (!lse || !utt_llsum || !utt_frames || !n_bad) return g_gerr.fail(XVEC_ERR_ARG, "null pointer: lse / utt_llsum / utt_frames / n_bad");
    const Layout l = loglik_layout(frames->n_utts, C, D);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, l.total, g_gerr))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    FrameArgs fa{};
    if ((rc = put_frames(frames, n_total, workspace, l, fa, s))) return rc;
    double* P = part<double>(workspace, l.P);
    double* g = part<double>(workspace, l.g);
    const bool f32 = frames->x_type == XVEC_GMM_X_F32;
    if ((rc = prepare(w, mu_override ? mu_override : mu, v, C, D, P, g, nullptr, s))) return rc;
    if ((rc = run_lse(fa, f32, P, g, C, D, lse, nullptr, s))) return rc;
    if ((rc = clear_bad(n_bad, s))) return rc;
    gmm_sums_kernel<<<(unsigned)fa.n_utts, kThreads, 0, s>>>(lse, fa.off, n_total, 0, utt_llsum, utt_frames,
                                                             reinterpret_cast<unsigned long long*>(n_bad), nullptr);
    if ((rc = g_gerr.launch_ok("gmm_sums_kernel"))) return rc;
    if (gamma && n_total) {
        const dim3 grid((unsigned)frame_tiles(n_total), (unsigned)comp_tiles(C));
        if (f32) gmm_gamma_kernel<float><<<grid, kThreads, 0, s>>>(fa, P, g, C, D, lse, gamma);
        else gmm_gamma_kernel<double><<<grid, kThreads, 0, s>>>(fa, P, g, C, D, lse, gamma);
        if ((rc = g_gerr.launch_ok("gmm_gamma_kernel"))) return rc;
    }
    return XVEC_OK;
}

int xvec_gmm_accumulate(const xvec_gmm_frames* frames, const double* w, const double* mu, const double* v, int32_t C, int32_t D,
                        int32_t per_utt, int32_t n_slices, double* n, double* f, double* sq, double* llsum, int64_t* n_frames,
                        int64_t* n_bad, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    Refusal why;
    int64_t n_total = 0;
    if (check_model(C, D, why) || check_frames(frames, D, &n_total, why) || check_slices(per_utt, n_slices, why)) return refused(why);
    if (!w || !mu || !v) return g_gerr.fail(XVEC_ERR_ARG, "null pointer: w / mu / v");
    if (!n || !f || (!per_utt && !sq)) return g_gerr.fail(XVEC_ERR_ARG, "null pointer: n / f / s");
    if (!llsum || !n_frames || !n_bad) return g_gerr.fail(XVEC_ERR_ARG, "null pointer: llsum / n_frames / n_bad");
    const Layout l = accumulate_layout(n_total, frames->n_utts, C, D, per_utt, n_slices);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, l.total, g_gerr))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    FrameArgs fa{};
    if ((rc = put_frames(frames, n_total, workspace, l, fa, s))) return rc;
    double* P = part<double>(workspace, l.P);
    double* g = part<double>(workspace, l.g);
    const bool f32 = frames->x_type == XVEC_GMM_X_F32;
    if ((rc = prepare(w, mu, v, C, D, P, g, nullptr, s))) return rc;
    if (!per_utt) return run_global(fa, f32, workspace, l, C, D, n, f, sq, llsum, n_frames, n_bad, nullptr, s);
    double* lse = part<double>(workspace, l.lse);
    if ((rc = run_lse(fa, f32, P, g, C, D, lse, nullptr, s))) return rc;
    if ((rc = clear_bad(n_bad, s))) return rc;
    gmm_sums_kernel<<<(unsigned)fa.n_utts, kThreads, 0, s>>>(lse, fa.off, n_total, 0, llsum, n_frames,
                                                             reinterpret_cast<unsigned long long*>(n_bad), nullptr);
    if ((rc = g_gerr.launch_ok("gmm_sums_kernel"))) return rc;
    StatArgs a{};
    a.fa = fa;
    a.P = P;
    a.g = g;
    a.lse = lse;
    a.n = n;
    a.f = f;
    a.C = C;
    a.D = D;
    a.ctiles = comp_tiles(C);
    a.ytiles = y_tiles(D, true);
    const dim3 grid((unsigned)fa.n_utts, (unsigned)a.ctiles, (unsigned)a.ytiles);
    if (f32) gmm_stats_kernel<float, true><<<grid, kThreads, 0, s>>>(a);
    else gmm_stats_kernel<double, true><<<grid, kThreads, 0, s>>>(a);
    return g_gerr.launch_ok("gmm_stats_kernel");
}

int xvec_gmm_mstep(const double* n, const double* f, const double* sq, const int64_t* n_frames, int32_t C, int32_t D,
                   const xvec_gmm_mstep_options* options, double* w, double* mu, double* v, xvec_stream stream) {
    Refusal why;
    if (check_model(C, D, why) || check_options(options, why)) return refused(why);
    if (!n || !f || !sq || !n_frames || !w || !mu || !v) return g_gerr.fail(XVEC_ERR_ARG, "null pointer: n / f / s / n_frames / w / mu / v");
    return run_mstep(n, f, sq, n_frames, C, D, *options, w, mu, v, nullptr, static_cast<hipStream_t>(stream));
}

int xvec_gmm_em(const xvec_gmm_frames* frames, int32_t C, int32_t D, int32_t max_iter, double tol,
                const xvec_gmm_mstep_options* options, int32_t n_slices, double* w, double* mu, double* v, double* lower_bound,
                int32_t* n_iter_done, int64_t* n_bad, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    Refusal why;
    int64_t n_total = 0;
    if (check_model(C, D, why) || check_frames(frames, D, &n_total, why) || check_slices(0, n_slices, why) ||
        check_em(max_iter, tol, why) || check_options(options, why))
        return refused(why);
    if (!w || !mu || !v) return g_gerr.fail(XVEC_ERR_ARG, "null pointer: w / mu / v");
    if (!lower_bound || !n_iter_done || !n_bad) return g_gerr.fail(XVEC_ERR_ARG, "null pointer: lower_bound / n_iter_done / n_bad");
    if (n_total == 0) return g_gerr.fail(XVEC_ERR_ARG, "the utterances hold no frame");
    const Layout l = em_layout(n_total, frames->n_utts, C, D, n_slices);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, l.total, g_gerr))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    FrameArgs fa{};
    if ((rc = put_frames(frames, n_total, workspace, l, fa, s))) return rc;
    const bool f32 = frames->x_type == XVEC_GMM_X_F32;
    double* P = part<double>(workspace, l.P);
    double* g = part<double>(workspace, l.g);
    double* n = part<double>(workspace, l.n);
    double* f = part<double>(workspace, l.f);
    double* sq = part<double>(workspace, l.s);
    double* llsum = part<double>(workspace, l.sums);
    int64_t* n_frames = part<int64_t>(workspace, l.sums) + 1;
    EmState* st = part<EmState>(workspace, l.state);
    const int32_t* stop = &st->stop;
    gmm_em_init_kernel<<<blocks_for(max_iter), kThreads, 0, s>>>(st, lower_bound, max_iter, n_iter_done);
    if ((rc = g_gerr.launch_ok("gmm_em_init_kernel"))) return rc;
    if ((rc = clear_bad(n_bad, s))) return rc;
    for (int it = 0; it < max_iter; ++it) {
        if ((rc = prepare(w, mu, v, C, D, P, g, stop, s))) return rc;
        if ((rc = run_global(fa, f32, workspace, l, C, D, n, f, sq, llsum, n_frames, n_bad, stop, s))) return rc;
        if ((rc = run_mstep(n, f, sq, n_frames, C, D, *options, w, mu, v, stop, s))) return rc;
        gmm_em_check_kernel<<<1, 1, 0, s>>>(st, llsum, n_frames, it, tol, lower_bound, n_iter_done);
        if ((rc = g_gerr.launch_ok("gmm_em_check_kernel"))) return rc;
    }
    return XVEC_OK;
}

int xvec_gmm_map_means(const double* n, const double* f, const double* mu, int64_t M, int32_t C, int32_t D, double relevance,
                       double* mu_hat, xvec_stream stream) {
    Refusal why;
    if (check_model(C, D, why) || check_map(M, relevance, why)) return refused(why);
    if (!n || !f || !mu || !mu_hat) return g_gerr.fail(XVEC_ERR_ARG, "null pointer: n / f / mu / mu_hat");
    const int64_t total = M * C * D;
    if (total > kMaxLaunch) return g_gerr.fail(XVEC_ERR_TOO_LARGE, "M C D = %lld elements exceed one launch", (long long)total);
    gmm_map_kernel<<<blocks_for(total), kThreads, 0, static_cast<hipStream_t>(stream)>>>(n, f, mu, total, C, D, relevance, mu_hat);
    return g_gerr.launch_ok("gmm_map_kernel");
}

int xvec_gmm_linear_scores(const double* mu_hat, int64_t M, const double* n, const double* f, int64_t U, const double* mu,
                           const double* v, int32_t C, int32_t D, double* S, int64_t ld_s, void* workspace, size_t workspace_bytes,
                           xvec_stream stream) {
    Refusal why;
    if (check_model(C, D, why) || check_scores(M, U, ld_s, why)) return refused(why);
    if (!mu_hat || !n || !f || !mu || !v || !S) return g_gerr.fail(XVEC_ERR_ARG, "null pointer: mu_hat / n / f / mu / v / S");
    const ScoreLayout l = score_layout(M, U, C, D);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, l.total, g_gerr))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t CD = (int64_t)C * D;
    double* model = part<double>(workspace, l.model);
    double* test = part<double>(workspace, l.test);
    if (M * CD > kMaxLaunch) return g_gerr.fail(XVEC_ERR_TOO_LARGE, "M C D = %lld elements exceed one launch", (long long)(M * CD));
    gmm_super_model_kernel<<<blocks_for(M * CD), kThreads, 0, s>>>(mu_hat, mu, v, M * CD, CD, model);
    if ((rc = g_gerr.launch_ok("gmm_super_model_kernel"))) return rc;
    gmm_super_test_kernel<<<(unsigned)U, kThreads, 0, s>>>(n, f, mu, C, D, test);
    if ((rc = g_gerr.launch_ok("gmm_super_test_kernel"))) return rc;
    const int64_t tiles = ((U + kCT - 1) / kCT) * ((M + kFT - 1) / kFT);
    if (tiles > kMaxFrames) return g_gerr.fail(XVEC_ERR_TOO_LARGE, "M = %lld by U = %lld scores exceed 2^31 - 1 tiles of 64 x 64", (long long)M, (long long)U);
    gmm_scores_kernel<<<(unsigned)tiles, kThreads, 0, s>>>(model, test, M, U, CD, S, ld_s);
    if ((rc = g_gerr.launch_ok("gmm_scores_kernel"))) return rc;
    return XVEC_OK;
}

}  // extern "C"
