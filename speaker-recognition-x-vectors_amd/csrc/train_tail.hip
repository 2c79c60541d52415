// The tail of a training step, forward and backward, fp32 (reference main.py:72-75, 99-100, 148): statistics pooling, the three
// segment-level Linear layers, the cross-entropy loss, and Adam.  C ABI: include/xvec_train.h.
//   pooling    one pass over y5: sums of deviations about the utterance's first frame, four row groups added in group order
//              (train_tail_pool.h; its length-masked form is what train_tail_ragged.hip passes in -- the only kernels of the
//              tail that see frames; everything after the pooling is per utterance)
//   products   ONE tiled kernel on v_mfma_f32_32x32x2_f32 (tail_gemm_kernel) over 64 x 64 tiles with the reduction split into
//              slices; every slice writes its partial product to a slab and tail_epilogue_kernel sums the slabs in slice order
//              and applies the bias, the ReLU or the ReLU mask.  With M = batch a product has few tiles: the slices are what
//              fills the chip.  The slice count depends on the shape alone (device-independent results).
//   loss       one block per row (maximum, sum of exponentials: fixed trees), then the rows in index order
//   Adam       one launch per 32 tensors, the pointer table in the argument block
// No atomics anywhere: results are bit-identical per call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/xvec_hip.h"
#include "../../include/xvec_train.h"
#include "host_support.h"
#include "tdnn_common.h"
#include "train_tail_pool.h"

namespace xvec {
namespace {

constexpr int kTM = 64, kTN = 64, kTK = 16;     // block tile; 4 waves as 2 x 2, each one 32 x 32 MFMA tile
// LDS images are [k][row] with a row stride of 68 floats: the two lane halves of an MFMA operand read the k rows kk and kk + 8,
// 8 * 68 = 32 banks apart; the transposing stores of a k-contiguous operand (a wave = 16 rows x 4 k-quads) land on
// (4 q + j) * 68 + row = 64 different banks.
constexpr int kTLD = 68;
constexpr int kSliceMinK = 64;                  // a slice of the reduction is at least this long ...
constexpr int kSliceBlocks = 512;               // ... and slices x tiles aim at this many blocks

enum { EPI_SUM = 0, EPI_BIAS = 1, EPI_BIAS_RELU = 2, EPI_MASK = 3 };

struct TailGemm {
    const float* a;      // A_KC: [M][K]   otherwise [K][M]
    const float* b;      // B_KC: [N][K]   otherwise [K][N]
    float* c;            // slab [slices][M][N]
    int M, N, K;
    int k_per_slice;     // a multiple of kTK
    int tiles_m, tiles_n, slices;
};

__device__ __forceinline__ void load4(const float* p, float (&v)[4]) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}

// four values of one operand tile: KC (rows x k, k contiguous): row (tid >> 2), k from (tid & 3) * 4; otherwise (k x rows,
// rows contiguous): k row (tid >> 4), rows from (tid & 15) * 4.  Out-of-range elements are 0.
template <bool KC, bool VEC>
__device__ __forceinline__ void tile_load(const float* __restrict__ base, int R, int K, int r0, int kcur, int kend, float (&v)[4]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = 0.f;
    if constexpr (KC) {
        const int r = r0 + (tid >> 2), k = kcur + (tid & 3) * 4;
        if (r >= R) return;
        const float* p = base + (size_t)r * K + k;
        if constexpr (VEC) {
            if (k < kend) load4(p, v);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k + j < kend) v[j] = p[j];
        }
    } else {
        const int k = kcur + (tid >> 4), r = r0 + (tid & 15) * 4;
        if (k >= kend) return;
        const float* p = base + (size_t)k * R + r;
        if constexpr (VEC) {
            if (r < R) load4(p, v);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (r + j < R) v[j] = p[j];
        }
    }
}

template <bool KC>
__device__ __forceinline__ void tile_store(float (*s)[kTLD], const float (&v)[4]) {
    const int tid = threadIdx.x;
    if constexpr (KC) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[(tid & 3) * 4 + j][tid >> 2] = v[j];
    } else {
        *reinterpret_cast<f32x4*>(&s[tid >> 4][(tid & 15) * 4]) = f32x4{v[0], v[1], v[2], v[3]};
    }
}

// slab[slice] = A B over the slice's part of the reduction
template <bool A_KC, bool B_KC, bool VEC>
__global__ __launch_bounds__(256) void tail_gemm_kernel(const TailGemm g) {
    __shared__ __attribute__((aligned(16))) float sA[2][kTK][kTLD];
    __shared__ __attribute__((aligned(16))) float sB[2][kTK][kTLD];
    const int per_slice = g.tiles_m * g.tiles_n;
    const int slice = blockIdx.x / per_slice, tile = blockIdx.x - slice * per_slice;
    const int tm = tile / g.tiles_n, tn = tile - tm * g.tiles_n;
    const int m0 = tm * kTM, n0 = tn * kTN;
    const int kbeg = slice * g.k_per_slice;
    const int kend = min(g.K, kbeg + g.k_per_slice);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l31 = lane & 31, lh = lane >> 5;

    float ra[4], rb[4];
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    const int n_it = kend > kbeg ? (kend - kbeg + kTK - 1) / kTK : 0;
    if (n_it > 0) {
        tile_load<A_KC, VEC>(g.a, g.M, g.K, m0, kbeg, kend, ra);
        tile_load<B_KC, VEC>(g.b, g.N, g.K, n0, kbeg, kend, rb);
        tile_store<A_KC>(sA[0], ra);
        tile_store<B_KC>(sB[0], rb);
        __syncthreads();
    }
    for (int it = 0; it < n_it; ++it) {
        const int buf = it & 1;
        if (it + 1 < n_it) {                                 // in flight while this chunk's MFMAs run
            tile_load<A_KC, VEC>(g.a, g.M, g.K, m0, kbeg + (it + 1) * kTK, kend, ra);
            tile_load<B_KC, VEC>(g.b, g.N, g.K, n0, kbeg + (it + 1) * kTK, kend, rb);
        }
#pragma unroll
        for (int kk = 0; kk < kTK / 2; ++kk) {
            const int k = kk + 8 * lh;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[buf][k][wr * 32 + l31], sB[buf][k][wc * 32 + l31], acc, 0, 0, 0);
        }
        if (it + 1 < n_it) {
            tile_store<A_KC>(sA[buf ^ 1], ra);
            tile_store<B_KC>(sB[buf ^ 1], rb);
        }
        __syncthreads();
    }

    // C/D of the 32 x 32 MFMA: column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    float* out = g.c + (size_t)slice * g.M * g.N;
    const int col = n0 + wc * 32 + l31;
    if (col >= g.N) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (row < g.M) out[(size_t)row * g.N + col] = acc[r];
    }
}

// out[i] = f(sum over slices, in slice order, of slab[s][i]): plus bias[column], ReLU, or the select [act[i] > 0]
__global__ __launch_bounds__(256) void tail_epilogue_kernel(const float* __restrict__ slab, int slices, size_t count, int N, int mode,
                                                            const float* __restrict__ bias, const float* __restrict__ act,
                                                            float* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= count) return;
    float s = 0.f;
#pragma unroll 8
    for (int sl = 0; sl < slices; ++sl) s += slab[sl * count + i];
    if (mode == EPI_BIAS || mode == EPI_BIAS_RELU) s += bias[i % N];
    if (mode == EPI_BIAS_RELU) s = fmaxf(s, 0.f);
    if (mode == EPI_MASK) s = act[i] > 0.f ? s : 0.f;
    out[i] = s;
}

// out[col] = sum over the rows of src[row][col].  A block takes 64 columns: thread (column tid & 63, row group tid >> 6) adds the
// rows grp, grp + 4, ... in row order, the four groups are then added in group order.
__global__ __launch_bounds__(256) void tail_colsum_kernel(const float* __restrict__ src, int rows, int cols, float* __restrict__ out) {
    __shared__ float sh[4][64];
    const int c = threadIdx.x & 63, grp = threadIdx.x >> 6, col = blockIdx.x * 64 + c;
    float s = 0.f;
    if (col < cols) {
#pragma unroll 8
        for (int r = grp; r < rows; r += 4) s += src[(size_t)r * cols + col];
    }
    sh[grp][c] = s;
    __syncthreads();
    if (grp == 0 && col < cols) out[col] = ((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c];
}

// ---------------------------------------------------------------- the loss
// all 256 threads' values combined by a fixed tree; the result in every thread
template <bool MAX>
__device__ __forceinline__ float block_tree(float v, float* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sh[tid] = MAX ? fmaxf(sh[tid], sh[tid + s]) : sh[tid] + sh[tid + s];
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

// row maximum and the sum of exp(x - maximum) of one row of K logits
__device__ __forceinline__ void row_softmax_terms(const float* __restrict__ x, int K, float* sh, float& mx, float& sum) {
    float m = -INFINITY;
    for (int k = threadIdx.x; k < K; k += 256) m = fmaxf(m, x[k]);
    mx = block_tree<true>(m, sh);
    float s = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) s += expf(x[k] - mx);
    sum = block_tree<false>(s, sh);
}

// rowloss[b] = logsumexp(logits[b]) - logits[b][label[b]]; NaN for a label outside [0, K) (nothing is read through it)
__global__ __launch_bounds__(256) void tail_rowloss_kernel(const float* __restrict__ logits, int K, const long long* __restrict__ labels,
                                                           float* __restrict__ rowloss) {
    __shared__ float sh[256];
    const float* x = logits + (size_t)blockIdx.x * K;
    float mx, sum;
    row_softmax_terms(x, K, sh, mx, sum);
    if (threadIdx.x != 0) return;
    const long long label = labels[blockIdx.x];
    rowloss[blockIdx.x] = label >= 0 && label < K ? (mx + logf(sum)) - x[label] : NAN;
}

// loss = (sum over the rows, in index order) / B: the block stages 256 rows at a time, thread 0 adds them
__global__ __launch_bounds__(256) void tail_loss_mean_kernel(const float* __restrict__ rowloss, int B, float* __restrict__ loss) {
    __shared__ float sh[256];
    float s = 0.f;
    for (int b0 = 0; b0 < B; b0 += 256) {
        if (b0 + (int)threadIdx.x < B) sh[threadIdx.x] = rowloss[b0 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int j = 0; j < min(256, B - b0); ++j) s += sh[j];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = s / (float)B;
}

// dlogits = dloss (softmax(logits) - onehot(label)) / B; a label outside [0, K) has no onehot entry
__global__ __launch_bounds__(256) void tail_dlogits_kernel(const float* __restrict__ logits, int K, int B, const long long* __restrict__ labels,
                                                           const float* __restrict__ dloss, float* __restrict__ dlogits) {
    __shared__ float sh[256];
    const float* x = logits + (size_t)blockIdx.x * K;
    float mx, sum;
    row_softmax_terms(x, K, sh, mx, sum);
    const long long label = labels[blockIdx.x];
    const float scale = dloss[0] / (float)B;
    for (int k = threadIdx.x; k < K; k += 256) {
        const float p = expf(x[k] - mx) / sum;
        dlogits[(size_t)blockIdx.x * K + k] = scale * (p - (k == label ? 1.0f : 0.f));
    }
}

// ---------------------------------------------------------------- Adam
constexpr int kAdamMax = 32;                    // tensors per launch
constexpr int kAdamPerBlock = 4096;             // elements per block: 256 threads x 4 quads

struct AdamTable {
    float* p[kAdamMax];
    const float* g[kAdamMax];
    float* m[kAdamMax];
    float* v[kAdamMax];
    long long n[kAdamMax];
    int first_block[kAdamMax];   // ascending; INT_MAX past the last tensor
    int shift[kAdamMax];         // floats between the 16-byte boundary below and the base, the same for p, g, m, v; -1 where they
                                 // differ: that tensor goes element by element
    float b1, omb1, b2, omb2;    // beta1, 1 - beta1, beta2, 1 - beta2
    float step_size;             // lr / (1 - beta1^t)
    float bc2_sqrt;              // sqrt(1 - beta2^t)
    float eps;
};

__device__ __forceinline__ void adam_update(const AdamTable& t, float g, float& m, float& v, float& p) {
    m = fmaf(t.b1, m, t.omb1 * g);
    v = fmaf(t.b2, v, t.omb2 * g * g);
    p -= t.step_size * (m / (sqrtf(v) / t.bc2_sqrt + t.eps));
}

// A block takes 4096 consecutive elements of one tensor, counted from the 16-byte boundary below its base: thread quads that
// lie inside the tensor move as 16 bytes, the ragged ends element by element.  The block's tensor is looked up in the argument
// block where it lies, in the kernel-argument segment (scalar loads at a uniform index; indexing the by-value copy
// dynamically would put it in scratch).  INVARIANT: the table is the kernel's FIRST AND ONLY argument, so it starts at
// offset 0 of the kernel-argument segment (explicit arguments are laid out in order from offset 0, each at its natural
// alignment; hidden arguments follow them).  Another argument in front of it would need its offset added here.
typedef const AdamTable __attribute__((address_space(4))) * AdamTablePtr;

__global__ __launch_bounds__(256) void adam_step_kernel(const AdamTable t) {
    const AdamTablePtr tab = (AdamTablePtr)__builtin_amdgcn_kernarg_segment_ptr();   // t, at offset 0: see above
    const int blk = blockIdx.x;
    int idx = 0;
#pragma unroll
    for (int i = 1; i < kAdamMax; ++i) idx += blk >= t.first_block[i] ? 1 : 0;
    float* p = tab->p[idx];
    const float* g = tab->g[idx];
    float* m = tab->m[idx];
    float* v = tab->v[idx];
    const long long n = tab->n[idx];
    const int first = tab->first_block[idx], shift = tab->shift[idx];
    const bool vec = shift >= 0;
    const long long origin = (long long)(blk - first) * kAdamPerBlock - (vec ? shift : 0);
#pragma unroll
    for (int it = 0; it < kAdamPerBlock / 1024; ++it) {
        const long long i0 = origin + (it * 256 + (int)threadIdx.x) * 4;
        if (i0 >= n || i0 + 3 < 0) continue;
        if (vec && i0 >= 0 && i0 + 3 < n) {
            float gg[4], mm[4], vv[4], pp[4];
            load4(g + i0, gg);
            load4(m + i0, mm);
            load4(v + i0, vv);
            load4(p + i0, pp);
#pragma unroll
            for (int j = 0; j < 4; ++j) adam_update(t, gg[j], mm[j], vv[j], pp[j]);
            *reinterpret_cast<f32x4*>(m + i0) = f32x4{mm[0], mm[1], mm[2], mm[3]};
            *reinterpret_cast<f32x4*>(v + i0) = f32x4{vv[0], vv[1], vv[2], vv[3]};
            *reinterpret_cast<f32x4*>(p + i0) = f32x4{pp[0], pp[1], pp[2], pp[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long i = i0 + j;
                if (i < 0 || i >= n) continue;
                float mm = m[i], vv = v[i], pp = p[i];
                adam_update(t, g[i], mm, vv, pp);
                m[i] = mm;
                v[i] = vv;
                p[i] = pp;
            }
        }
    }
}

// ---------------------------------------------------------------- host side

ErrorChannel& terr() { return train_error_channel(); }

struct Product {
    int M, N, K, tiles_m, tiles_n, slices, k_per_slice;
    size_t slab_floats() const { return (size_t)slices * M * N; }
};

// the slices of one product: from the shape alone
Product make_product(int M, int N, int K) {
    Product p{};
    p.M = M; p.N = N; p.K = K;
    p.tiles_m = (M + kTM - 1) / kTM;
    p.tiles_n = (N + kTN - 1) / kTN;
    const int64_t tiles = (int64_t)p.tiles_m * p.tiles_n;
    const int64_t by_blocks = std::max<int64_t>(1, kSliceBlocks / tiles);
    const int64_t by_k = std::max<int64_t>(1, (K + kSliceMinK - 1) / kSliceMinK);
    const int want = (int)std::min(by_blocks, by_k);
    p.k_per_slice = ((K + want - 1) / want + kTK - 1) / kTK * kTK;
    p.slices = (K + p.k_per_slice - 1) / p.k_per_slice;
    return p;
}

struct Shape {
    int B, Tp, C, H, K;
};

struct Plan {
    Product pre6, pre7, out;                  // forward:  [B, H] over 2C, [B, H] over H, [B, K] over H
    Product dWo, da7, dW7, da6, dW6, dpool;   // backward: [K, H] over B, [B, H] over K, [H, H] over B, [B, H] over H,
                                              //           [H, 2C] over B, [B, 2C] over H
    float* rowloss;    // [B]
    float* dlogits;    // [B, K]
    float* dz7;        // [B, H]
    float* dz6;        // [B, H]
    float* dpooled;    // [B, 2C]
    float* slab;       // the largest product's slices
    size_t total;
};

int make_shape(int B, int Tp, int C, int H, int K, Shape& s) {
    if (B < 1 || C < 1 || H < 1 || K < 1)
        return terr().fail(XVEC_ERR_ARG, "B = %d, C = %d, H = %d and K = %d must be >= 1", B, C, H, K);
    if (Tp < 2) return terr().fail(XVEC_ERR_ARG, "Tp = %d: the unbiased std needs at least 2 pooled frames", Tp);
    if (B > 65535) return terr().fail(XVEC_ERR_TOO_LARGE, "B = %d utterances: more than 65535", B);
    if ((int64_t)B * Tp > 0x7fffffff)
        return terr().fail(XVEC_ERR_TOO_LARGE, "B * Tp = %lld frames: row indices are int32", (long long)B * Tp);
    if (2 * (int64_t)C > 0x3fffffff || H > 0x3fffffff || K > 0x3fffffff)
        return terr().fail(XVEC_ERR_TOO_LARGE, "2 C = %lld, H = %d, K = %d: column indices are int32", 2 * (long long)C, H, K);
    s.B = B; s.Tp = Tp; s.C = C; s.H = H; s.K = K;
    return XVEC_OK;
}

Plan make_plan(void* ws, const Shape& s) {
    Plan p{};
    const int C2 = 2 * s.C;
    p.pre6 = make_product(s.B, s.H, C2);
    p.pre7 = make_product(s.B, s.H, s.H);
    p.out = make_product(s.B, s.K, s.H);
    p.dWo = make_product(s.K, s.H, s.B);
    p.da7 = make_product(s.B, s.H, s.K);
    p.dW7 = make_product(s.H, s.H, s.B);
    p.da6 = make_product(s.B, s.H, s.H);
    p.dW6 = make_product(s.H, C2, s.B);
    p.dpool = make_product(s.B, C2, s.H);
    size_t slab = 0;
    for (const Product* q : {&p.pre6, &p.pre7, &p.out, &p.dWo, &p.da7, &p.dW7, &p.da6, &p.dW6, &p.dpool})
        slab = std::max(slab, q->slab_floats());
    Carver c(ws);
    p.rowloss = c.take<float>(s.B);
    p.dlogits = c.take<float>((size_t)s.B * s.K);
    p.dz7 = c.take<float>((size_t)s.B * s.H);
    p.dz6 = c.take<float>((size_t)s.B * s.H);
    p.dpooled = c.take<float>((size_t)s.B * C2);
    p.slab = c.take<float>(slab);
    p.total = c.total();
    return p;
}

// out = f(A B): the sliced product into the slab, then the epilogue
template <bool A_KC, bool B_KC>
int product(const Product& q, const float* a, const float* b, float* slab, int mode, const float* bias, const float* act,
            float* out, hipStream_t st, const char* what) {
    TailGemm g{};
    g.a = a; g.b = b; g.c = slab;
    g.M = q.M; g.N = q.N; g.K = q.K;
    g.k_per_slice = q.k_per_slice;
    g.tiles_m = q.tiles_m; g.tiles_n = q.tiles_n; g.slices = q.slices;
    const int64_t blocks = (int64_t)q.tiles_m * q.tiles_n * q.slices;
    if (blocks > 0x7fffffff) return terr().fail(XVEC_ERR_TOO_LARGE, "%s: %lld blocks", what, (long long)blocks);
    const bool vec = aligned16(a) && aligned16(b) && (A_KC ? q.K : q.M) % 4 == 0 && (B_KC ? q.K : q.N) % 4 == 0;
    if (vec) tail_gemm_kernel<A_KC, B_KC, true><<<(unsigned)blocks, 256, 0, st>>>(g);
    else tail_gemm_kernel<A_KC, B_KC, false><<<(unsigned)blocks, 256, 0, st>>>(g);
    int rc;
    if ((rc = terr().launch_ok(what))) return rc;
    const size_t count = (size_t)q.M * q.N;
    tail_epilogue_kernel<<<(unsigned)((count + 255) / 256), 256, 0, st>>>(slab, q.slices, count, q.N, mode, bias, act, out);
    return terr().launch_ok("tail_epilogue_kernel");
}

int colsum(const float* src, int rows, int cols, float* out, hipStream_t st) {
    tail_colsum_kernel<<<(cols + 63) / 64, 256, 0, st>>>(src, rows, cols, out);
    return terr().launch_ok("tail_colsum_kernel");
}

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

size_t xvec_train_tail_workspace_bytes(int32_t B, int32_t Tp, int32_t C, int32_t H, int32_t K) {
    Shape s;
    if (make_shape(B, Tp, C, H, K, s)) return 0;
    return make_plan(nullptr, s).total;
}

}  // extern "C"

namespace xvec {

// Launches: the pooling; three times product + epilogue; the row losses and their mean.
int train_tail_forward(const float* y5, int32_t B, int32_t Tp, int32_t C, const float* W6, const float* b6, int32_t H,
                       const float* W7, const float* b7, const float* Wo, const float* bo, int32_t K, const int64_t* labels,
                       float* pooled, float* a6, float* a7, float* logits, float* loss, void* workspace, size_t workspace_bytes,
                       xvec_stream stream, TailPoolFn pool, const int32_t* lengths_dev) {
    if (!y5 || !W6 || !b6 || !W7 || !b7 || !Wo || !bo || !labels)
        return terr().fail(XVEC_ERR_ARG, "null pointer: y5, the six segment parameters and labels are required");
    if (!pooled || !a6 || !a7 || !logits || !loss)
        return terr().fail(XVEC_ERR_ARG, "null pointer: pooled, a6, a7, logits and loss are required");
    Shape s;
    int rc;
    if ((rc = make_shape(B, Tp, C, H, K, s))) return rc;
    const Plan p = make_plan(workspace, s);
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, p.total, terr(), XVEC_ERR_ARG))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);

    if ((rc = pool(y5, B, Tp, C, lengths_dev, pooled, st))) return rc;
    if ((rc = product<true, true>(p.pre6, pooled, W6, p.slab, EPI_BIAS_RELU, b6, nullptr, a6, st, "tail_gemm_kernel (layer 6)"))) return rc;
    if ((rc = product<true, true>(p.pre7, a6, W7, p.slab, EPI_BIAS_RELU, b7, nullptr, a7, st, "tail_gemm_kernel (layer 7)"))) return rc;
    if ((rc = product<true, true>(p.out, a7, Wo, p.slab, EPI_BIAS, bo, nullptr, logits, st, "tail_gemm_kernel (output)"))) return rc;
    tail_rowloss_kernel<<<B, 256, 0, st>>>(logits, K, reinterpret_cast<const long long*>(labels), p.rowloss);
    if ((rc = terr().launch_ok("tail_rowloss_kernel"))) return rc;
    tail_loss_mean_kernel<<<1, 256, 0, st>>>(p.rowloss, B, loss);
    return terr().launch_ok("tail_loss_mean_kernel");
}

// Launches: dlogits and dbo; per layer from the output down the weight gradient, the gradient of its input under the ReLU
// mask of the layer below, and that layer's bias gradient; the gradient of pooled; dy5.
int train_tail_backward(const float* dloss, const float* y5, int32_t B, int32_t Tp, int32_t C, const float* W6, int32_t H,
                        const float* W7, const float* Wo, int32_t K, const int64_t* labels, const float* pooled, const float* a6,
                        const float* a7, const float* logits, float* dy5, float* dW6, float* db6, float* dW7, float* db7,
                        float* dWo, float* dbo, void* workspace, size_t workspace_bytes, xvec_stream stream, TailPoolBwdFn pool_bwd,
                        const int32_t* lengths_dev) {
    if (!dloss || !y5 || !W6 || !W7 || !Wo || !labels || !pooled || !a6 || !a7 || !logits)
        return terr().fail(XVEC_ERR_ARG, "null pointer: dloss, y5, W6, W7, Wo, labels, pooled, a6, a7 and logits are required");
    if (!dW6 || !db6 || !dW7 || !db7 || !dWo || !dbo)
        return terr().fail(XVEC_ERR_ARG, "null pointer: the six parameter gradients are required (only dy5 may be null)");
    Shape s;
    int rc;
    if ((rc = make_shape(B, Tp, C, H, K, s))) return rc;
    const Plan p = make_plan(workspace, s);
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, p.total, terr(), XVEC_ERR_ARG))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);

    tail_dlogits_kernel<<<B, 256, 0, st>>>(logits, K, B, reinterpret_cast<const long long*>(labels), dloss, p.dlogits);
    if ((rc = terr().launch_ok("tail_dlogits_kernel"))) return rc;
    if ((rc = colsum(p.dlogits, B, K, dbo, st))) return rc;
    if ((rc = product<false, false>(p.dWo, p.dlogits, a7, p.slab, EPI_SUM, nullptr, nullptr, dWo, st, "tail_gemm_kernel (dWo)"))) return rc;
    if ((rc = product<true, false>(p.da7, p.dlogits, Wo, p.slab, EPI_MASK, nullptr, a7, p.dz7, st, "tail_gemm_kernel (da7)"))) return rc;
    if ((rc = colsum(p.dz7, B, H, db7, st))) return rc;
    if ((rc = product<false, false>(p.dW7, p.dz7, a6, p.slab, EPI_SUM, nullptr, nullptr, dW7, st, "tail_gemm_kernel (dW7)"))) return rc;
    if ((rc = product<true, false>(p.da6, p.dz7, W7, p.slab, EPI_MASK, nullptr, a6, p.dz6, st, "tail_gemm_kernel (da6)"))) return rc;
    if ((rc = colsum(p.dz6, B, H, db6, st))) return rc;
    if ((rc = product<false, false>(p.dW6, p.dz6, pooled, p.slab, EPI_SUM, nullptr, nullptr, dW6, st, "tail_gemm_kernel (dW6)"))) return rc;
    if (!dy5) return XVEC_OK;
    if ((rc = product<true, false>(p.dpool, p.dz6, W6, p.slab, EPI_SUM, nullptr, nullptr, p.dpooled, st, "tail_gemm_kernel (dpooled)"))) return rc;
    return pool_bwd(y5, B, Tp, C, lengths_dev, pooled, p.dpooled, dy5, st);
}

}  // namespace xvec

extern "C" {

int xvec_train_tail_forward(const float* y5, int32_t B, int32_t Tp, int32_t C, const float* W6, const float* b6, int32_t H,
                            const float* W7, const float* b7, const float* Wo, const float* bo, int32_t K,
                            const int64_t* labels, float* pooled, float* a6, float* a7, float* logits, float* loss,
                            void* workspace, size_t workspace_bytes, xvec_stream stream) {
    return train_tail_forward(y5, B, Tp, C, W6, b6, H, W7, b7, Wo, bo, K, labels, pooled, a6, a7, logits, loss, workspace,
                              workspace_bytes, stream, launch_tail_pool<false>, nullptr);
}

int xvec_train_tail_backward(const float* dloss, const float* y5, int32_t B, int32_t Tp, int32_t C, const float* W6, int32_t H,
                             const float* W7, const float* Wo, int32_t K, const int64_t* labels, const float* pooled,
                             const float* a6, const float* a7, const float* logits, float* dy5, float* dW6, float* db6,
                             float* dW7, float* db7, float* dWo, float* dbo, void* workspace, size_t workspace_bytes,
                             xvec_stream stream) {
    return train_tail_backward(dloss, y5, B, Tp, C, W6, H, W7, Wo, K, labels, pooled, a6, a7, logits, dy5, dW6, db6, dW7, db7, dWo,
                               dbo, workspace, workspace_bytes, stream, launch_tail_pool_bwd<false>, nullptr);
}

// Launches: one per 32 tensors.
int xvec_adam_step(float* const* params_host, const float* const* grads_host, float* const* exp_avg_host,
                   float* const* exp_avg_sq_host, const int64_t* lengths_host, int32_t n_tensors, double lr, double beta1,
                   double beta2, double eps, int64_t t, xvec_stream stream) {
    if (!params_host || !grads_host || !exp_avg_host || !exp_avg_sq_host || !lengths_host)
        return terr().fail(XVEC_ERR_ARG, "null pointer: the four pointer tables and lengths_host are required");
    if (n_tensors < 0) return terr().fail(XVEC_ERR_ARG, "n_tensors = %d must be >= 0", n_tensors);
    if (t < 1) return terr().fail(XVEC_ERR_ARG, "t = %lld: the step count starts at 1", (long long)t);
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0))
        return terr().fail(XVEC_ERR_ARG, "beta1 = %g and beta2 = %g must lie in [0, 1)", beta1, beta2);
    for (int i = 0; i < n_tensors; ++i) {
        if (lengths_host[i] < 0) return terr().fail(XVEC_ERR_ARG, "tensor %d: length %lld", i, (long long)lengths_host[i]);
        if (lengths_host[i] && (!params_host[i] || !grads_host[i] || !exp_avg_host[i] || !exp_avg_sq_host[i]))
            return terr().fail(XVEC_ERR_ARG, "tensor %d: null pointer", i);
        for (const void* q : {(const void*)params_host[i], (const void*)grads_host[i], (const void*)exp_avg_host[i], (const void*)exp_avg_sq_host[i]})
            if (reinterpret_cast<uintptr_t>(q) % 4) return terr().fail(XVEC_ERR_ARG, "tensor %d: a pointer is not 4-byte aligned", i);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    AdamTable tab{};
    tab.b1 = (float)beta1; tab.omb1 = (float)(1.0 - beta1);
    tab.b2 = (float)beta2; tab.omb2 = (float)(1.0 - beta2);
    tab.step_size = (float)(lr / (1.0 - std::pow(beta1, (double)t)));
    tab.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(beta2, (double)t));
    tab.eps = (float)eps;
    int i = 0;
    while (i < n_tensors) {
        int used = 0;
        int64_t blocks = 0;
        for (; i < n_tensors && used < kAdamMax; ++i) {
            if (lengths_host[i] == 0) continue;
            const uintptr_t mis = reinterpret_cast<uintptr_t>(params_host[i]) % 16;
            const bool same = reinterpret_cast<uintptr_t>(grads_host[i]) % 16 == mis &&
                              reinterpret_cast<uintptr_t>(exp_avg_host[i]) % 16 == mis &&
                              reinterpret_cast<uintptr_t>(exp_avg_sq_host[i]) % 16 == mis;
            const int shift = same ? (int)(mis / 4) : -1;
            const int64_t nb = (lengths_host[i] + (same ? shift : 0) + kAdamPerBlock - 1) / kAdamPerBlock;
            if (blocks + nb > 0x7fffffff) return terr().fail(XVEC_ERR_TOO_LARGE, "tensor %d: %lld elements", i, (long long)lengths_host[i]);
            tab.p[used] = params_host[i]; tab.g[used] = grads_host[i];
            tab.m[used] = exp_avg_host[i]; tab.v[used] = exp_avg_sq_host[i];
            tab.n[used] = lengths_host[i];
            tab.first_block[used] = (int)blocks;
            tab.shift[used] = shift;
            blocks += nb;
            ++used;
        }
        if (!used) break;
        for (int k = used; k < kAdamMax; ++k) {
            tab.p[k] = nullptr; tab.g[k] = nullptr; tab.m[k] = nullptr; tab.v[k] = nullptr;
            tab.n[k] = 0; tab.first_block[k] = INT_MAX; tab.shift[k] = -1;
        }
        adam_step_kernel<<<(unsigned)blocks, 256, 0, st>>>(tab);
        int rc;
        if ((rc = terr().launch_ok("adam_step_kernel"))) return rc;
    }
    return XVEC_OK;
}

}  // extern "C"
