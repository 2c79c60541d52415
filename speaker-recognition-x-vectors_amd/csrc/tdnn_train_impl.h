// One TDNN layer in training mode, forward and backward, fp32 (reference tdnn_layer.py:26-41 under model.train()).
// C ABI: include/xvec_train.h.  Three matrix products on v_mfma_f32_32x32x2_f32, all through ONE tiled kernel
// (train_gemm_kernel) whose operand loaders differ per product:
//   FWD  z  [N, Cout]          = ReLU(x_ctx [N, K] W^T + bias)     the context gather happens in the A loader
//   DW   dW [Cout, K]          = dz^T x_ctx                        reduction over the N rows, split into slices: every
//                                                                  slice writes its partial product to a slab, a second
//                                                                  launch sums the slabs in slice order
//   DX   dx [B*T, Cin]         = dz_ctx [B*T, taps*Cout] W_taps    row q of an utterance gathers dz rows q - off(tap),
//                                                                  zero where that leaves the utterance
// and column reductions over the rows (BatchNorm statistics, dbeta, dgamma, dbias) in 256-row chunks: one partial per
// chunk and column, summed in chunk order by a second launch.  No float atomics anywhere: results are bit-identical per call.
//
// Every kernel that sees rows has a compile-time RAGGED variant (xvec_tdnn_train_*_ragged): the padded layout stays, a row
// (b, p) takes part iff p < len[b] - span.  Invalid rows are masked by SELECTION -- their operands are never loaded, their
// outputs are written as 0 -- so nothing depends on what the padding holds.  The unmasked variant carries an empty Lengths
// argument and none of the masking code.  This header holds the kernels and both calls' host code as templates over RAGGED;
// tdnn_train.hip instantiates the unmasked form, tdnn_train_ragged.hip the masked one (each translation unit gets only its
// own kernels).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/xvec_hip.h"
#include "../../include/xvec_train.h"
#include "dropout_mask.h"
#include "host_support.h"
#include "tdnn_common.h"

namespace xvec {
namespace {

constexpr int kMaxTaps = 8;
constexpr int kBM = 128, kBN = 128, kBK = 16;   // block tile; 4 waves as 2 x 2, each 64 x 64 = 2 x 2 MFMA tiles of 32 x 32
// LDS images are [k][row] with a row stride of 132 floats: the two lane halves of an MFMA operand read the k rows kk and
// kk + 8, 8 * 132 = 32 banks apart (one conflict-free ds_read_b32); the transposing stores of the k-contiguous operands
// (thread = 4 k of one row; a wave = 16 rows x 4 k-quads) land on (4 q + j) * 132 + row = 64 different banks.
constexpr int kLD = 132;
constexpr int kChunk = 256;                     // rows per partial of the column reductions
constexpr int kDwMinRows = 256;                 // a dW slice is at least this many rows ...
constexpr int kDwBlocks = 1024;                 // ... and slices x tiles aim at this many blocks (fixed: device-independent results)

// (a NAMED enumeration: the kernels' parameter list depends on OP == OP_FWD_DROPOUT, which is part of their mangled names, and
// the host and the device compilation number unnamed types differently)
enum Op : int { OP_FWD = 0, OP_DW = 1, OP_DX = 2, OP_FWD_DROPOUT = 3 };

// The valid INPUT frames per utterance of a ragged call, device int32 [B]; empty in the unmasked kernels.
template <bool RAGGED>
struct Lengths {};
template <>
struct Lengths<true> {
    const int32_t* len;
    int B, T, span;
};

// Dropout after the ReLU (the *_dropout calls): threshold and scale of dropout_mask.h for the call's p, and the (seed, stream)
// that name its mask; empty in the kernels without it.  The backward carries the scale only.
template <bool DROPOUT>
struct Dropout {};
template <>
struct Dropout<true> {
    uint32_t thr;
    float scale;
    uint64_t seed, stream;
};

// valid output rows of utterance b: len[b] - span for a length in [span + 1, T]; a length outside that range, which the host
// cannot see, gives the utterance no rows at all
__device__ __forceinline__ int valid_rows(const Lengths<true>& L, int b) {
    if (b >= L.B) return 0;
    const int l = L.len[b];
    return l > L.span && l <= L.T ? l - L.span : 0;
}

// valid rows among the rows [r0, r1) of the padded [B * Tp] row space, and the first of them (-1: none)
__device__ __forceinline__ int valid_in_range(const Lengths<true>& L, int Tp, int r0, int r1, int& first) {
    int cnt = 0;
    first = -1;
    for (int b = r0 / Tp; b < L.B && b * Tp < r1; ++b) {
        const int lo = max(r0, b * Tp), hi = min(r1, b * Tp + valid_rows(L, b));
        if (hi > lo) {
            if (first < 0) first = lo;
            cnt += hi - lo;
        }
    }
    return cnt;
}

// all valid rows of the call, in every thread of the block (integer sum: any order gives the same)
__device__ __forceinline__ int valid_total(const Lengths<true>& L, int* sh) {
    int s = 0;
    for (int b = threadIdx.x; b < L.B; b += blockDim.x) s += valid_rows(L, b);
    if (threadIdx.x == 0) *sh = 0;
    __syncthreads();
    if (s) atomicAdd(sh, s);
    __syncthreads();
    return *sh;
}

// (utterance, frame, valid rows of the utterance) of a row that moves forward through the padded row space
struct RowWalk {
    int b, p, v;
    __device__ __forceinline__ RowWalk(const Lengths<true>& L, int Tp, int r) : b(r / Tp), p(r - (r / Tp) * Tp), v(valid_rows(L, r / Tp)) {}
    __device__ __forceinline__ bool valid() const { return p < v; }
    __device__ __forceinline__ void step(const Lengths<true>& L, int Tp, int n) {
        p += n;
        if (p < Tp) return;
        while (p >= Tp) {
            p -= Tp;
            ++b;
        }
        v = valid_rows(L, b);
    }
};

struct GemmArgs {
    const float* a;      // FWD: x    DW: dz   DX: dz
    const float* b;      // FWD: W    DW: x    DX: W
    const float* bias;   // FWD
    float* c;            // FWD: z    DW: slab (or dW itself with one slice)    DX: dx
    int M, N, K;         // product dimensions; K is the whole reduction length
    int k_per_slice;     // DW: rows per slice (a multiple of kBK); otherwise K
    int tiles_m, tiles_n;
    int T, Tp, Cin, Cout, Kw;   // Kw = taps * Cin, the row length of W
    int off[kMaxTaps];          // context[i] - context[0]
};

// off[tap] without a dynamically indexed copy of the argument block (which would live in scratch)
__device__ __forceinline__ int tap_off(const GemmArgs& g, int tap) {
    int o = g.off[0];
#pragma unroll
    for (int i = 1; i < kMaxTaps; ++i) o = tap == i ? g.off[i] : o;
    return o;
}

// (tap, c) + step along a [taps][width] axis
__device__ __forceinline__ void advance(int& tap, int& c, int step, int width) {
    c += step;
    while (c >= width) {
        c -= width;
        ++tap;
    }
}

// OP_FWD_DROPOUT is OP_FWD with the dropout mask in the epilogue: z = keep ? max(acc + bias, 0) * scale : 0, the mask from
// dropout_mask.h.  Only csrc/tdnn_train_dropout.hip instantiates it; D is empty in every other product.
template <int OP, bool VEC, bool RAGGED>
__global__ __launch_bounds__(256, 2) void train_gemm_kernel(const GemmArgs g, const Lengths<RAGGED> L,
                                                            const Dropout<OP == OP_FWD_DROPOUT> D) {
    constexpr bool FWD = OP == OP_FWD || OP == OP_FWD_DROPOUT, DROPOUT = OP == OP_FWD_DROPOUT;
    __shared__ __attribute__((aligned(16))) float sA[2][kBK][kLD];
    __shared__ __attribute__((aligned(16))) float sB[2][kBK][kLD];
    const int per_slice = g.tiles_m * g.tiles_n;
    const int logical = xcd_remap(blockIdx.x, gridDim.x);       // the column tiles of one row tile share an XCD's L2
    const int slice = logical / per_slice, tile = logical - slice * per_slice;
    const int tm = tile / g.tiles_n, tn = tile - tm * g.tiles_n;
    const int m0 = tm * kBM, n0 = tn * kBN;
    const int kbeg = slice * g.k_per_slice;
    const int kend = min(g.K, kbeg + g.k_per_slice);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l31 = lane & 31, lh = lane >> 5;

    // ---- loaders.  k-contiguous operands (FWD A, FWD B, DX A): pass i = row (tid >> 2) + 64 i, four k from (tid & 3) * 4.
    // row-contiguous operands (DW A, DW B, DX B): pass i = k row (tid >> 5) + 8 i, four rows/columns from (tid & 31) * 4.
    const int kc_row = tid >> 2, kc_k = (tid & 3) * 4;
    const int mc_k = tid >> 5, mc_col = (tid & 31) * 4;
    float ra[2][4], rb[2][4];

    // per-thread state of the A operand
    int a_base[2] = {0, 0}, a_q[2] = {0, 0};       // FWD: frame b*T + p      DX: b*Tp and q
    int a_v[2] = {0, 0};                           // RAGGED DX: valid dz rows of the utterance
    bool a_ok[2] = {false, false};
    int a_tap = 0, a_c = 0;                        // FWD / DX: (tap, channel) of k = kcur + kc_k
    if constexpr (FWD) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + kc_row + 64 * i;
            a_ok[i] = m < g.M;
            const int b = m / g.Tp;
            a_base[i] = b * g.T + (m - b * g.Tp);
            if constexpr (RAGGED) a_ok[i] = a_ok[i] && m - b * g.Tp < valid_rows(L, b);     // an invalid row loads nothing
        }
        a_tap = kc_k / g.Cin;
        a_c = kc_k - a_tap * g.Cin;
    } else if constexpr (OP == OP_DX) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + kc_row + 64 * i;
            a_ok[i] = m < g.M;
            const int b = m / g.T;
            a_base[i] = b * g.Tp;
            a_q[i] = m - b * g.T;
            if constexpr (RAGGED) a_v[i] = a_ok[i] ? valid_rows(L, b) : 0;
        }
        a_tap = kc_k / g.Cout;
        a_c = kc_k - a_tap * g.Cout;
    }
    // per-thread state of the B operand
    int b_row[2] = {0, 0}, b_p[2] = {0, 0};        // DW: utterance b and frame p of row k     DX: (tap, co) of k
    int b_v[2] = {0, 0};                           // RAGGED DW: valid rows of utterance b_row
    if constexpr (OP == OP_DW) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = kbeg + mc_k + 8 * i;
            b_row[i] = r / g.Tp;
            b_p[i] = r - b_row[i] * g.Tp;
            if constexpr (RAGGED) b_v[i] = valid_rows(L, b_row[i]);
        }
    } else if constexpr (OP == OP_DX) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int k = mc_k + 8 * i;
            b_row[i] = k / g.Cout;
            b_p[i] = k - b_row[i] * g.Cout;
        }
    }

    auto load4 = [&](const float* p, float (&v)[4]) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    };

    auto gload = [&](int kcur) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ra[i][j] = 0.f;
                rb[i][j] = 0.f;
            }
        // ---------------- A
        if constexpr (FWD || OP == OP_DX) {
            const int k = kcur + kc_k;
            const int width = FWD ? g.Cin : g.Cout;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (!a_ok[i]) continue;
                if constexpr (VEC) {
                    if (k < kend) {
                        const int o = tap_off(g, a_tap);
                        if constexpr (FWD) {
                            load4(g.a + (int64_t)(a_base[i] + o) * g.Cin + a_c, ra[i]);
                        } else {
                            const int p = a_q[i] - o;
                            if (p >= 0 && p < (RAGGED ? a_v[i] : g.Tp)) load4(g.a + (int64_t)(a_base[i] + p) * g.Cout + a_c, ra[i]);
                        }
                    }
                } else {
                    int tj = a_tap, cj = a_c;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (k + j < kend) {
                            const int o = tap_off(g, tj);
                            if constexpr (FWD) {
                                ra[i][j] = g.a[(int64_t)(a_base[i] + o) * g.Cin + cj];
                            } else {
                                const int p = a_q[i] - o;
                                if (p >= 0 && p < (RAGGED ? a_v[i] : g.Tp)) ra[i][j] = g.a[(int64_t)(a_base[i] + p) * g.Cout + cj];
                            }
                        }
                        advance(tj, cj, 1, width);
                    }
                }
            }
            advance(a_tap, a_c, kBK, width);
        } else {                                   // DW: dz[k, m]
            const int m = m0 + mc_col;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int k = kcur + mc_k + 8 * i;
                if (k >= kend) continue;
                const float* p = g.a + (int64_t)k * g.Cout + m;
                if constexpr (VEC) {
                    if (m < g.M) load4(p, ra[i]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (m + j < g.M) ra[i][j] = p[j];
                }
            }
        }
        // ---------------- B
        if constexpr (FWD) {              // W[n, k]
            const int k = kcur + kc_k;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int n = n0 + kc_row + 64 * i;
                if (n >= g.N) continue;
                const float* p = g.b + (int64_t)n * g.Kw + k;
                if constexpr (VEC) {
                    if (k < kend) load4(p, rb[i]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (k + j < kend) rb[i][j] = p[j];
                }
            }
        } else if constexpr (OP == OP_DW) {        // x_ctx[k, n]: frame (b, p + off(tap of n)), channel of n
            const int n = n0 + mc_col;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int k = kcur + mc_k + 8 * i;
                if (k < kend && (!RAGGED || b_p[i] < b_v[i])) {        // RAGGED: the x rows of an invalid dz row stay 0 (0 * NaN)
                    const int frame = b_row[i] * g.T + b_p[i];
                    if constexpr (VEC) {
                        if (n < g.N) {
                            const int tap = n / g.Cin;
                            load4(g.b + (int64_t)(frame + tap_off(g, tap)) * g.Cin + (n - tap * g.Cin), rb[i]);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (n + j < g.N) {
                                const int tap = (n + j) / g.Cin;
                                rb[i][j] = g.b[(int64_t)(frame + tap_off(g, tap)) * g.Cin + (n + j - tap * g.Cin)];
                            }
                    }
                }
                if constexpr (RAGGED) {
                    const int before = b_row[i];
                    advance(b_row[i], b_p[i], kBK, g.Tp);
                    if (b_row[i] != before) b_v[i] = valid_rows(L, b_row[i]);
                } else {
                    advance(b_row[i], b_p[i], kBK, g.Tp);
                }
            }
        } else {                                   // DX: W[co, tap * Cin + n] at k = tap * Cout + co
            const int n = n0 + mc_col;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int k = kcur + mc_k + 8 * i;
                if (k < kend) {
                    const float* p = g.b + (int64_t)b_p[i] * g.Kw + b_row[i] * g.Cin + n;
                    if constexpr (VEC) {
                        if (n < g.N) load4(p, rb[i]);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (n + j < g.N) rb[i][j] = p[j];
                    }
                }
                advance(b_row[i], b_p[i], kBK, g.Cout);
            }
        }
    };

    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if constexpr (OP == OP_DW) {
                *reinterpret_cast<f32x4*>(&sA[buf][mc_k + 8 * i][mc_col]) = f32x4{ra[i][0], ra[i][1], ra[i][2], ra[i][3]};
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) sA[buf][kc_k + j][kc_row + 64 * i] = ra[i][j];
            }
            if constexpr (FWD) {
#pragma unroll
                for (int j = 0; j < 4; ++j) sB[buf][kc_k + j][kc_row + 64 * i] = rb[i][j];
            } else {
                *reinterpret_cast<f32x4*>(&sB[buf][mc_k + 8 * i][mc_col]) = f32x4{rb[i][0], rb[i][1], rb[i][2], rb[i][3]};
            }
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int n_it = kend > kbeg ? (kend - kbeg + kBK - 1) / kBK : 0;
    if (n_it > 0) {
        gload(kbeg);
        lstore(0);
        __syncthreads();
    }
    for (int it = 0; it < n_it; ++it) {
        const int buf = it & 1;
        if (it + 1 < n_it) gload(kbeg + (it + 1) * kBK);     // in flight while this chunk's 32 MFMAs per wave run
#pragma unroll
        for (int kk = 0; kk < kBK / 2; ++kk) {
            const int k = kk + 8 * lh;
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = sA[buf][k][wr * 64 + i * 32 + l31];
                b[i] = sB[buf][k][wc * 64 + i * 32 + l31];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (it + 1 < n_it) lstore(buf ^ 1);
        __syncthreads();
    }

    // RAGGED forward: which of the tile's rows are valid, once per row, in the first words of sA (the K loop ended on a barrier:
    // nobody reads the operands any more)
    int* const s_valid = reinterpret_cast<int*>(&sA[0][0][0]);
    if constexpr (FWD && RAGGED) {
        if (tid < kBM) {
            const int m = m0 + tid, b = m / g.Tp;
            s_valid[tid] = m < g.M && m - b * g.Tp < valid_rows(L, b);
        }
        __syncthreads();
    }

    // C/D of the 32 x 32 MFMA: column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int ldc = g.N;
    float* out = g.c + (OP == OP_DW ? (size_t)slice * g.M * g.N : (size_t)0);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + wc * 64 + j * 32 + l31;
        if (col >= g.N) continue;
        float bias = 0.f;
        if constexpr (FWD) bias = g.bias[col];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            [[maybe_unused]] dropout::Words words{};
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                // DROPOUT: the accumulators r & 3 are four consecutive rows from a multiple of 4 -- the four words of one call
                if constexpr (DROPOUT)
                    if ((r & 3) == 0 && row < g.M) words = dropout::row_quad_words((uint32_t)col, (uint32_t)row >> 2, D.seed, D.stream);
                if (row >= g.M) continue;
                float v = acc[i][j][r];
                if constexpr (FWD) v = fmaxf(v + bias, 0.f);
                if constexpr (DROPOUT) v = words.w[r & 3] >= D.thr ? v * D.scale : 0.f;
                if constexpr (FWD && RAGGED) v = s_valid[row - m0] ? v : 0.f;      // an invalid row of z is exactly 0
                out[(size_t)row * ldc + col] = v;
            }
        }
    }
}


// out[i] = sum over slices, in slice order, of slab[s][i]
__global__ __launch_bounds__(256) void train_slab_reduce_kernel(const float* __restrict__ slab, int slices, size_t count,
                                                                float* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= count) return;
    float s = 0.f;
    for (int sl = 0; sl < slices; ++sl) s += slab[sl * count + i];
    out[i] = s;
}

// ---------------------------------------------------------------- column reductions over the rows
// A block takes 64 columns of one 256-row chunk: thread (column tid & 63, row group tid >> 6) walks the rows
// group, group + 4, ... of the chunk; the four groups are then added in group order.
struct ColCtx {
    int col, grp, r0, r1;
    bool ok;
};
__device__ __forceinline__ ColCtx col_ctx(int N, int Cout) {
    ColCtx c;
    c.col = blockIdx.x * 64 + (threadIdx.x & 63);
    c.grp = threadIdx.x >> 6;
    c.r0 = blockIdx.y * kChunk;
    c.r1 = min(N, c.r0 + kChunk);
    c.ok = c.col < Cout;
    return c;
}
// sum of the four row groups' values of every column, in group order, in all four threads of the column
__device__ __forceinline__ float group_sum(float v, float (*sh)[64]) {
    __syncthreads();                     // (the previous use of sh is over)
    sh[threadIdx.x >> 6][threadIdx.x & 63] = v;
    __syncthreads();
    const int c = threadIdx.x & 63;
    return ((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c];
}

// chunk mean and sum of squared deviations about it: part[chunk][0][col] = mean, part[chunk][1][col] = M2.  The mean is
// formed about a pivot (the chunk's first row), the deviations in a second pass over the chunk (it sits in the cache).
// RAGGED: over the chunk's valid rows only, about its first valid row; a chunk without one writes (0, 0), which the merge skips.
template <bool RAGGED>
__global__ __launch_bounds__(256) void train_stats_kernel(const float* __restrict__ z, int N, int Cout, int Tp, float* __restrict__ part,
                                                          const Lengths<RAGGED> L) {
    __shared__ float sh[4][64];
    ColCtx c = col_ctx(N, Cout);
    int first = c.r0, n_valid = c.r1 - c.r0;
    if constexpr (RAGGED) {
        c.grp = __builtin_amdgcn_readfirstlane(c.grp);      // a wave walks one row group: its row bookkeeping is scalar
        n_valid = valid_in_range(L, Tp, c.r0, c.r1, first);
    }
    const float cnt = (float)n_valid;
    float pivot = 0.f, s = 0.f;
    if (c.ok && (!RAGGED || n_valid > 0)) {
        pivot = z[(size_t)first * Cout + c.col];
        if constexpr (RAGGED) {
            RowWalk w(L, Tp, c.r0 + c.grp);
            for (int r = c.r0 + c.grp; r < c.r1; r += 4, w.step(L, Tp, 4))
                if (w.valid()) s += z[(size_t)r * Cout + c.col] - pivot;
        } else {
            for (int r = c.r0 + c.grp; r < c.r1; r += 4) s += z[(size_t)r * Cout + c.col] - pivot;
        }
    }
    const float gs = group_sum(s, sh);
    const float mean = RAGGED && n_valid == 0 ? 0.f : pivot + gs / cnt;
    float q = 0.f;
    if (c.ok && (!RAGGED || n_valid > 0)) {
        if constexpr (RAGGED) {
            RowWalk w(L, Tp, c.r0 + c.grp);
            for (int r = c.r0 + c.grp; r < c.r1; r += 4, w.step(L, Tp, 4))
                if (w.valid()) {
                    const float d = z[(size_t)r * Cout + c.col] - mean;
                    q = fmaf(d, d, q);
                }
        } else {
            for (int r = c.r0 + c.grp; r < c.r1; r += 4) {
                const float d = z[(size_t)r * Cout + c.col] - mean;
                q = fmaf(d, d, q);
            }
        }
    }
    q = group_sum(q, sh);
    if (c.ok && c.grp == 0) {
        part[((size_t)blockIdx.y * 2 + 0) * Cout + c.col] = mean;
        part[((size_t)blockIdx.y * 2 + 1) * Cout + c.col] = q;
    }
}

// the chunks' (mean, M2) merged in chunk order (Chan et al.): batch mean and BIASED variance
// RAGGED: a chunk counts its valid rows (none: skipped; the first that has some starts the merge), the variance divides by
// the call's valid rows.
template <bool RAGGED>
__global__ __launch_bounds__(64) void train_stats_merge_kernel(const float* __restrict__ part, int chunks, int N, int Cout, int Tp,
                                                               float* __restrict__ mean_out, float* __restrict__ var_out,
                                                               const Lengths<RAGGED> L) {
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= Cout) return;
    float mean = 0.f, m2 = 0.f, n = 0.f;
    int total = N;
    if constexpr (RAGGED) {
        total = 0;
    } else {
        mean = part[col];
        m2 = part[Cout + col];
        n = (float)min(N, kChunk);
    }
    for (int ch = RAGGED ? 0 : 1; ch < chunks; ++ch) {
        float nc = (float)(min(N, (ch + 1) * kChunk) - ch * kChunk);
        const float mc = part[((size_t)ch * 2 + 0) * Cout + col], qc = part[((size_t)ch * 2 + 1) * Cout + col];
        if constexpr (RAGGED) {
            int first;
            const int cnt = valid_in_range(L, Tp, ch * kChunk, min(N, (ch + 1) * kChunk), first);
            if (cnt == 0) continue;
            nc = (float)cnt;
            if (total == 0) {
                mean = mc;
                m2 = qc;
                n = nc;
                total = cnt;
                continue;
            }
            total += cnt;
        }
        const float tot = n + nc, delta = mc - mean;
        mean += delta * (nc / tot);
        m2 += qc + delta * delta * (n * nc / tot);
        n = tot;
    }
    mean_out[col] = mean;
    var_out[col] = m2 / (float)total;
}

// RAGGED: an invalid row of y is exactly 0.
template <bool RAGGED>
__global__ __launch_bounds__(256) void train_norm_kernel(const float* __restrict__ z, int N, int Cout, int Tp,
                                                         const float* __restrict__ mean, const float* __restrict__ var,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float eps, float* __restrict__ y, const Lengths<RAGGED> L) {
    ColCtx c = col_ctx(N, Cout);
    if (!c.ok) return;
    const float mu = mean[c.col], scale = gamma[c.col] * (1.0f / sqrtf(var[c.col] + eps)), shift = beta[c.col];
    if constexpr (RAGGED) {
        c.grp = __builtin_amdgcn_readfirstlane(c.grp);
        RowWalk w(L, Tp, c.r0 + c.grp);
        for (int r = c.r0 + c.grp; r < c.r1; r += 4, w.step(L, Tp, 4)) {
            const size_t i = (size_t)r * Cout + c.col;
            y[i] = w.valid() ? fmaf(z[i] - mu, scale, shift) : 0.f;
        }
    } else {
        for (int r = c.r0 + c.grp; r < c.r1; r += 4) {
            const size_t i = (size_t)r * Cout + c.col;
            y[i] = fmaf(z[i] - mu, scale, shift);
        }
    }
}

// part[chunk][0][col] = sum of dy, part[chunk][1][col] = sum of dy x^ over the chunk's rows
// RAGGED: dy of an invalid row is not read.
template <bool RAGGED>
__global__ __launch_bounds__(256) void train_bn_sums_kernel(const float* __restrict__ dy, const float* __restrict__ z, int N,
                                                            int Cout, int Tp, const float* __restrict__ mean,
                                                            const float* __restrict__ var, float eps, float* __restrict__ part,
                                                            const Lengths<RAGGED> L) {
    __shared__ float sh[4][64];
    ColCtx c = col_ctx(N, Cout);
    if constexpr (RAGGED) c.grp = __builtin_amdgcn_readfirstlane(c.grp);
    float s1 = 0.f, s2 = 0.f;
    if (c.ok) {
        const float mu = mean[c.col], invstd = 1.0f / sqrtf(var[c.col] + eps);
        if constexpr (RAGGED) {
            RowWalk w(L, Tp, c.r0 + c.grp);
            for (int r = c.r0 + c.grp; r < c.r1; r += 4, w.step(L, Tp, 4)) {
                if (!w.valid()) continue;
                const size_t i = (size_t)r * Cout + c.col;
                const float d = dy[i];
                s1 += d;
                s2 = fmaf(d, (z[i] - mu) * invstd, s2);
            }
        } else {
            for (int r = c.r0 + c.grp; r < c.r1; r += 4) {
                const size_t i = (size_t)r * Cout + c.col;
                const float d = dy[i];
                s1 += d;
                s2 = fmaf(d, (z[i] - mu) * invstd, s2);
            }
        }
    }
    s1 = group_sum(s1, sh);
    s2 = group_sum(s2, sh);
    if (c.ok && c.grp == 0) {
        part[((size_t)blockIdx.y * 2 + 0) * Cout + c.col] = s1;
        part[((size_t)blockIdx.y * 2 + 1) * Cout + c.col] = s2;
    }
}

// out_p[col] = sum over chunks, in chunk order, of part[chunk][p][col], p < planes (blockIdx.y = p)
__global__ __launch_bounds__(64) void train_col_reduce_kernel(const float* __restrict__ part, int chunks, int planes, int Cout,
                                                              float* __restrict__ out0, float* __restrict__ out1) {
    const int col = blockIdx.x * 64 + threadIdx.x, p = blockIdx.y;
    if (col >= Cout) return;
    float s = 0.f;
    for (int ch = 0; ch < chunks; ++ch) s += part[((size_t)ch * planes + p) * Cout + col];
    (p == 0 ? out0 : out1)[col] = s;
}

// dz = [z > 0] gamma invstd (dy - dbeta / N - x^ dgamma / N), or [z > 0] dy without BatchNorm; part[chunk][col] = sum of dz
// over the chunk's rows.  The mask is a SELECT: a channel that is never on gets exact zeros.
// RAGGED: the 1 / N is over the call's valid rows; an invalid row of dz is exactly 0 and its dy is not read.
// DROPOUT: z is the post-dropout value, so [z > 0] is "kept and on" (scale >= 1); dz is the value above times the scale.
template <bool RAGGED, bool DROPOUT>
__device__ __forceinline__ void dz_chunk(const float* __restrict__ dy, const float* __restrict__ z, int N, int Cout, int Tp,
                                         const float* __restrict__ gamma, const float* __restrict__ mean,
                                         const float* __restrict__ var, const float* __restrict__ dgamma,
                                         const float* __restrict__ dbeta, float eps, float* __restrict__ dz,
                                         float* __restrict__ part, const Lengths<RAGGED>& L, [[maybe_unused]] float keep_scale) {
    __shared__ float sh[4][64];
    ColCtx c = col_ctx(N, Cout);
    int rows = N;
    if constexpr (RAGGED) {
        __shared__ int sh_total;
        c.grp = __builtin_amdgcn_readfirstlane(c.grp);
        rows = valid_total(L, &sh_total);
    }
    float s = 0.f;
    if (c.ok) {
        float mu = 0.f, invstd = 1.f, scale = 1.f, kb = 0.f, kg = 0.f;
        if (gamma) {
            const float inv_n = 1.0f / (float)rows;
            mu = mean[c.col];
            invstd = 1.0f / sqrtf(var[c.col] + eps);
            scale = gamma[c.col] * invstd;
            kb = dbeta[c.col] * inv_n;
            kg = dgamma[c.col] * inv_n;
        }
        auto one = [&](int r) {
            const size_t i = (size_t)r * Cout + c.col;
            const float zv = z[i];
            float v = dy[i];
            if (gamma) v = scale * ((v - kb) - (zv - mu) * invstd * kg);
            if constexpr (DROPOUT) v *= keep_scale;
            v = zv > 0.f ? v : 0.f;
            dz[i] = v;
            s += v;
        };
        if constexpr (RAGGED) {
            RowWalk w(L, Tp, c.r0 + c.grp);
            for (int r = c.r0 + c.grp; r < c.r1; r += 4, w.step(L, Tp, 4)) {
                if (w.valid()) one(r);
                else dz[(size_t)r * Cout + c.col] = 0.f;
            }
        } else {
            for (int r = c.r0 + c.grp; r < c.r1; r += 4) one(r);
        }
    }
    s = group_sum(s, sh);
    if (c.ok && c.grp == 0) part[(size_t)blockIdx.y * Cout + c.col] = s;
}

template <bool RAGGED>
__global__ __launch_bounds__(256) void train_dz_kernel(const float* __restrict__ dy, const float* __restrict__ z, int N, int Cout, int Tp,
                                                       const float* __restrict__ gamma, const float* __restrict__ mean,
                                                       const float* __restrict__ var, const float* __restrict__ dgamma,
                                                       const float* __restrict__ dbeta, float eps, float* __restrict__ dz,
                                                       float* __restrict__ part, const Lengths<RAGGED> L) {
    dz_chunk<RAGGED, false>(dy, z, N, Cout, Tp, gamma, mean, var, dgamma, dbeta, eps, dz, part, L, 1.0f);
}

// Only csrc/tdnn_train_dropout.hip instantiates it.
template <bool RAGGED>
__global__ __launch_bounds__(256) void train_dz_dropout_kernel(const float* __restrict__ dy, const float* __restrict__ z, int N, int Cout,
                                                               int Tp, const float* __restrict__ gamma, const float* __restrict__ mean,
                                                               const float* __restrict__ var, const float* __restrict__ dgamma,
                                                               const float* __restrict__ dbeta, float eps, float* __restrict__ dz,
                                                               float* __restrict__ part, const Lengths<RAGGED> L, float keep_scale) {
    dz_chunk<RAGGED, true>(dy, z, N, Cout, Tp, gamma, mean, var, dgamma, dbeta, eps, dz, part, L, keep_scale);
}

// ---------------------------------------------------------------- host side

inline ErrorChannel& terr() { return train_error_channel(); }

struct Shape {
    int B, T, Cin, Cout, taps, span, Tp, N, Kw, chunks;
    int off[kMaxTaps];
};

struct Plan {
    int dw_tiles_m, dw_tiles_n, slices, rows_per_slice;
    float* part;       // column-reduction partials, 2 planes
    float* dz;         // [N, Cout]
    float* slab;       // dW partial products, one [Cout, Kw] per slice (slices > 1)
    size_t total;
};

// XVEC_OK, or the code with the message set
inline int make_shape(int B, int T, int Cin, int Cout, const int32_t* context_host, int n_ctx, Shape& s) {
    if (!context_host) return terr().fail(XVEC_ERR_ARG, "null pointer: context_host");
    if (B < 1 || T < 1 || Cin < 1 || Cout < 1)
        return terr().fail(XVEC_ERR_ARG, "B = %d, T = %d, Cin = %d and Cout = %d must be >= 1", B, T, Cin, Cout);
    if (n_ctx < 1 || n_ctx > kMaxTaps) return terr().fail(XVEC_ERR_ARG, "n_ctx = %d: 1 .. %d context offsets", n_ctx, kMaxTaps);
    for (int i = 1; i < n_ctx; ++i)
        if (context_host[i] <= context_host[i - 1])
            return terr().fail(XVEC_ERR_ARG, "context is not strictly increasing at entry %d (%d after %d)", i, context_host[i],
                               context_host[i - 1]);
    const int64_t span = (int64_t)context_host[n_ctx - 1] - context_host[0];
    if (T <= span) return terr().fail(XVEC_ERR_ARG, "T = %d is not longer than the context span %lld", T, (long long)span);
    if ((int64_t)B * T > 0x7fffffff)
        return terr().fail(XVEC_ERR_TOO_LARGE, "B * T = %lld frames: row indices are int32", (long long)B * T);
    if ((int64_t)n_ctx * std::max(Cin, Cout) > 0x7fffffff)
        return terr().fail(XVEC_ERR_TOO_LARGE, "n_ctx * max(Cin, Cout) = %lld: column indices are int32",
                           (long long)n_ctx * std::max(Cin, Cout));
    s.B = B; s.T = T; s.Cin = Cin; s.Cout = Cout; s.taps = n_ctx;
    s.span = (int)span;
    s.Tp = T - s.span;
    s.N = B * s.Tp;
    s.Kw = n_ctx * Cin;
    s.chunks = (s.N + kChunk - 1) / kChunk;
    if (s.chunks > 65535) return terr().fail(XVEC_ERR_TOO_LARGE, "N = %d rows: more than 65535 chunks of %d", s.N, kChunk);
    for (int i = 0; i < kMaxTaps; ++i) s.off[i] = i < n_ctx ? context_host[i] - context_host[0] : 0;
    return XVEC_OK;
}

inline Plan make_plan(void* ws, const Shape& s) {
    Plan p{};
    p.dw_tiles_m = (s.Cout + kBM - 1) / kBM;
    p.dw_tiles_n = (s.Kw + kBN - 1) / kBN;
    const int64_t tiles = (int64_t)p.dw_tiles_m * p.dw_tiles_n;
    const int64_t by_blocks = std::max<int64_t>(1, kDwBlocks / tiles);
    const int64_t by_rows = std::max<int64_t>(1, (s.N + kDwMinRows - 1) / kDwMinRows);
    p.slices = (int)std::min(by_blocks, by_rows);
    p.rows_per_slice = ((s.N + p.slices - 1) / p.slices + kBK - 1) / kBK * kBK;
    Carver c(ws);
    p.part = c.take<float>((size_t)2 * s.chunks * s.Cout);
    p.dz = c.take<float>((size_t)s.N * s.Cout);
    p.slab = c.take<float>(p.slices > 1 ? (size_t)p.slices * s.Cout * s.Kw : 0);
    p.total = c.total();
    return p;
}

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

template <int OP, bool RAGGED>
int launch_gemm(const GemmArgs& g, const Lengths<RAGGED>& L, int slices, bool vec, hipStream_t s, const char* what,
                const Dropout<OP == OP_FWD_DROPOUT>& D = {}) {
    const int64_t blocks = (int64_t)g.tiles_m * g.tiles_n * slices;
    if (blocks > 0x7fffffff) return terr().fail(XVEC_ERR_TOO_LARGE, "%s: %lld blocks", what, (long long)blocks);
    if (vec) train_gemm_kernel<OP, true, RAGGED><<<(unsigned)blocks, 256, 0, s>>>(g, L, D);
    else train_gemm_kernel<OP, false, RAGGED><<<(unsigned)blocks, 256, 0, s>>>(g, L, D);
    return terr().launch_ok(what);
}

// XVEC_OK and the call's Dropout block, or the code with the message set: 0 <= p < 1, NaN refused
inline int make_dropout(float p, uint64_t seed, uint64_t stream, Dropout<true>& D) {
    if (!dropout::valid_p(p)) return terr().fail(XVEC_ERR_ARG, "dropout p = %g: 0 <= p < 1", (double)p);
    D = Dropout<true>{dropout::threshold(p), dropout::keep_scale(p), seed, stream};
    return XVEC_OK;
}

inline GemmArgs gemm_args(const Shape& s) {
    GemmArgs g{};
    g.T = s.T; g.Tp = s.Tp; g.Cin = s.Cin; g.Cout = s.Cout; g.Kw = s.Kw;
    for (int i = 0; i < kMaxTaps; ++i) g.off[i] = s.off[i];
    return g;
}

inline dim3 col_grid(const Shape& s) { return dim3((s.Cout + 63) / 64, s.chunks); }

template <bool RAGGED>
Lengths<RAGGED> make_lengths(const Shape& s, const int32_t* lengths_dev) {
    if constexpr (RAGGED) return Lengths<true>{lengths_dev, s.B, s.T, s.span};
    else return Lengths<false>{};
}

// Launches: the product (+ bias, ReLU) into z; with BatchNorm the chunk statistics, their merge, the normalisation.
// DROPOUT: the product's epilogue applies the mask, everything after it sees the post-dropout z.
template <bool RAGGED, bool DROPOUT = false>
int train_forward(const float* x, int32_t B, int32_t T, int32_t Cin, const float* W, const float* bias, int32_t Cout,
                  const int32_t* context_host, int32_t n_ctx, const float* gamma, const float* beta, float eps, float* z,
                  float* batch_mean, float* batch_var, float* y, const int32_t* lengths_dev, void* workspace,
                  size_t workspace_bytes, xvec_stream stream, const Dropout<DROPOUT>& D = {}) {
    if (!x || !W || !bias || !z) return terr().fail(XVEC_ERR_ARG, "null pointer: x, W, bias and z are required");
    if (gamma && (!beta || !batch_mean || !batch_var || !y))
        return terr().fail(XVEC_ERR_ARG, "null pointer: with gamma, beta, batch_mean, batch_var and y are required");
    if (RAGGED && !lengths_dev) return terr().fail(XVEC_ERR_ARG, "null pointer: lengths_dev");
    Shape s;
    int rc;
    if ((rc = make_shape(B, T, Cin, Cout, context_host, n_ctx, s))) return rc;
    const Plan p = make_plan(workspace, s);
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, p.total, terr(), XVEC_ERR_ARG))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Lengths<RAGGED> L = make_lengths<RAGGED>(s, lengths_dev);

    GemmArgs g = gemm_args(s);
    g.a = x; g.b = W; g.bias = bias; g.c = z;
    g.M = s.N; g.N = Cout; g.K = s.Kw; g.k_per_slice = s.Kw;
    g.tiles_m = (g.M + kBM - 1) / kBM;
    g.tiles_n = (g.N + kBN - 1) / kBN;
    if ((rc = launch_gemm<DROPOUT ? OP_FWD_DROPOUT : OP_FWD>(g, L, 1, Cin % 4 == 0 && aligned16(x) && aligned16(W), st,
                                                             "train_gemm_kernel (forward)", D)))
        return rc;
    if (!gamma) return XVEC_OK;
    train_stats_kernel<RAGGED><<<col_grid(s), 256, 0, st>>>(z, s.N, Cout, s.Tp, p.part, L);
    if ((rc = terr().launch_ok("train_stats_kernel"))) return rc;
    train_stats_merge_kernel<RAGGED><<<(Cout + 63) / 64, 64, 0, st>>>(p.part, s.chunks, s.N, Cout, s.Tp, batch_mean, batch_var, L);
    if ((rc = terr().launch_ok("train_stats_merge_kernel"))) return rc;
    train_norm_kernel<RAGGED><<<col_grid(s), 256, 0, st>>>(z, s.N, Cout, s.Tp, batch_mean, batch_var, gamma, beta, eps, y, L);
    return terr().launch_ok("train_norm_kernel");
}

// Launches: with BatchNorm the chunk sums of dy and dy x^ and their reduction (dbeta, dgamma); dz and its chunk sums, their
// reduction (dbias); the dW product over row slices and, with more than one slice, the slab sum; the dx product.
// DROPOUT: z is the post-dropout value and dz carries the scale of the kept elements; nothing else differs.
template <bool RAGGED, bool DROPOUT = false>
int train_backward(const float* dy, const float* x, const float* z, int32_t B, int32_t T, int32_t Cin, const float* W,
                   int32_t Cout, const int32_t* context_host, int32_t n_ctx, const float* gamma, const float* batch_mean,
                   const float* batch_var, float eps, float* dx, float* dW, float* dbias, float* dgamma, float* dbeta,
                   const int32_t* lengths_dev, void* workspace, size_t workspace_bytes, xvec_stream stream,
                   [[maybe_unused]] const Dropout<DROPOUT>& D = {}) {
    if (!dy || !x || !z || !W || !dW || !dbias)
        return terr().fail(XVEC_ERR_ARG, "null pointer: dy, x, z, W, dW and dbias are required");
    if (gamma && (!batch_mean || !batch_var || !dgamma || !dbeta))
        return terr().fail(XVEC_ERR_ARG, "null pointer: with gamma, batch_mean, batch_var, dgamma and dbeta are required");
    if (RAGGED && !lengths_dev) return terr().fail(XVEC_ERR_ARG, "null pointer: lengths_dev");
    Shape s;
    int rc;
    if ((rc = make_shape(B, T, Cin, Cout, context_host, n_ctx, s))) return rc;
    const Plan p = make_plan(workspace, s);
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, p.total, terr(), XVEC_ERR_ARG))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Lengths<RAGGED> L = make_lengths<RAGGED>(s, lengths_dev);
    const dim3 cols((Cout + 63) / 64);

    if (gamma) {
        train_bn_sums_kernel<RAGGED><<<col_grid(s), 256, 0, st>>>(dy, z, s.N, Cout, s.Tp, batch_mean, batch_var, eps, p.part, L);
        if ((rc = terr().launch_ok("train_bn_sums_kernel"))) return rc;
        train_col_reduce_kernel<<<dim3(cols.x, 2), 64, 0, st>>>(p.part, s.chunks, 2, Cout, dbeta, dgamma);
        if ((rc = terr().launch_ok("train_col_reduce_kernel"))) return rc;
    }
    if constexpr (DROPOUT) {
        train_dz_dropout_kernel<RAGGED><<<col_grid(s), 256, 0, st>>>(dy, z, s.N, Cout, s.Tp, gamma, batch_mean, batch_var, dgamma, dbeta,
                                                                    eps, p.dz, p.part, L, D.scale);
    } else {
        train_dz_kernel<RAGGED><<<col_grid(s), 256, 0, st>>>(dy, z, s.N, Cout, s.Tp, gamma, batch_mean, batch_var, dgamma, dbeta, eps, p.dz,
                                                            p.part, L);
    }
    if ((rc = terr().launch_ok(DROPOUT ? "train_dz_dropout_kernel" : "train_dz_kernel"))) return rc;
    train_col_reduce_kernel<<<dim3(cols.x, 1), 64, 0, st>>>(p.part, s.chunks, 1, Cout, dbias, nullptr);
    if ((rc = terr().launch_ok("train_col_reduce_kernel"))) return rc;

    const bool vec = Cin % 4 == 0 && Cout % 4 == 0 && aligned16(x) && aligned16(W);
    GemmArgs g = gemm_args(s);
    g.a = p.dz; g.b = x; g.c = p.slices > 1 ? p.slab : dW;
    g.M = Cout; g.N = s.Kw; g.K = s.N; g.k_per_slice = p.rows_per_slice;
    g.tiles_m = p.dw_tiles_m;
    g.tiles_n = p.dw_tiles_n;
    if ((rc = launch_gemm<OP_DW>(g, L, p.slices, vec, st, "train_gemm_kernel (dW)"))) return rc;
    if (p.slices > 1) {
        const size_t count = (size_t)Cout * s.Kw;
        train_slab_reduce_kernel<<<(unsigned)((count + 255) / 256), 256, 0, st>>>(p.slab, p.slices, count, dW);
        if ((rc = terr().launch_ok("train_slab_reduce_kernel"))) return rc;
    }
    if (!dx) return XVEC_OK;
    g = gemm_args(s);
    g.a = p.dz; g.b = W; g.c = dx;
    g.M = B * T; g.N = Cin; g.K = s.taps * Cout; g.k_per_slice = g.K;
    g.tiles_m = (g.M + kBM - 1) / kBM;
    g.tiles_n = (g.N + kBN - 1) / kBN;
    return launch_gemm<OP_DX>(g, L, 1, vec, st, "train_gemm_kernel (dx)");
}

}  // namespace
}  // namespace xvec
