// Waveform augmentation in front of the MFCC front end: SNR mixing, reverberation, min-max scaling.
//   reference: dataset.py:185-396 (augment_data, add_with_certain_snr, augment_musan_*, augment_rir) and :217-219
// C ABI and the arithmetic: include/xvec_augment.h.  Kernels:
//   aug_mix_kernel<I16>      one block per utterance: fp64 working signal in the workspace, its ops in list order; per op one
//                            pass for the two integer sums of squares and one that applies the gain
//   aug_reverb_conv_kernel   the full convolution as a Toeplitz product on v_mfma_f32_32x32x2_f32 (below); keeps c[:n] and
//                            the block's max|c|
//   aug_reverb_apply_kernel  one block per utterance: max|x|, the maximum of the block maxima, out = x + c * (max|x| / max|c|)
//   aug_normalize_kernel     one block per row: min and max, then (x - min) / (max - min)
// Nothing goes through a float atomic: the sums of squares are 64-bit integer sums, maxima do not depend on the order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

#include "../../include/xvec_augment.h"
#include "../../include/xvec_hip.h"
#include "host_support.h"

namespace xvec {
namespace {

typedef float f32x16v __attribute__((ext_vector_type(16)));

constexpr int kRowThreads = 1024;             // the one-block-per-row kernels
constexpr int kRowWaves = kRowThreads / 64;

// ---------------------------------------------------------------- block reductions (every thread of the block calls them)

__device__ __forceinline__ float block_max(float v, float* sh, int waves) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    __syncthreads();      // sh may still be read from the call before
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = sh[0];
    for (int w = 1; w < waves; ++w) m = fmaxf(m, sh[w]);
    return m;
}

// ---------------------------------------------------------------- mix

struct MixArgs {
    float* waves;
    int64_t ld, n;
    const void* pool;
    int32_t n_rows;
    int64_t m_max;
    const int32_t* src_len;
    const xvec_aug_op* ops;      // device copy, checked by the host
    int32_t n_ops;
    const xvec_aug_src* srcs;
    double* work;                // [batch, n]
    double* gains;
    unsigned long long* n_bad_source;
};

// The op's noise at sample i, truncated: the sum in list order of the sources that reach that far
template <bool I16>
__device__ __forceinline__ long long noise_at(const MixArgs& g, const xvec_aug_op& op, int i) {
    double z = 0.0;
    for (int k = 0; k < op.n_src; ++k) {
        const xvec_aug_src s = g.srcs[op.first_src + k];
        if (s.row < 0 || s.row >= g.n_rows || s.start < 0) continue;      // counted once per op by thread 0
        const int64_t len = min((int64_t)max(g.src_len[s.row], 0), g.m_max);
        const int64_t p = (int64_t)s.start + i;
        if (p >= len) continue;
        const int64_t at = (int64_t)s.row * g.m_max + p;
        z += I16 ? (double)static_cast<const int16_t*>(g.pool)[at] : (double)static_cast<const float*>(g.pool)[at];
    }
    return (long long)z;      // toward zero
}

template <bool I16>
__global__ __launch_bounds__(kRowThreads) void aug_mix_kernel(const MixArgs g) {
#pragma clang fp contract(off)
    __shared__ int first_op, op_count;
    __shared__ unsigned long long sums[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        first_op = g.n_ops;
        op_count = 0;
    }
    __syncthreads();
    for (int o = tid; o < g.n_ops; o += kRowThreads) {      // the ops are sorted by utterance: mine are consecutive
        if (g.ops[o].utt == b) {
            atomicMin(&first_op, o);
            atomicAdd(&op_count, 1);
        }
    }
    __syncthreads();
    const int o_lo = first_op, o_hi = first_op + op_count;
    if (op_count == 0) return;      // a row without ops is not touched
    float* row = g.waves + (int64_t)b * g.ld;
    double* w = g.work + (int64_t)b * g.n;
    for (int64_t i = tid; i < g.n; i += kRowThreads) w[i] = (double)row[i];
    for (int o = o_lo; o < o_hi; ++o) {
        const xvec_aug_op op = g.ops[o];
        __syncthreads();      // the working signal of the op before is written; sums[] is free
        if (tid < 2) sums[tid] = 0;
        if (tid == 0) {
            unsigned long long bad = 0;
            for (int k = 0; k < op.n_src; ++k) {
                const xvec_aug_src s = g.srcs[op.first_src + k];
                bad += s.row < 0 || s.row >= g.n_rows || s.start < 0;
            }
            if (bad) atomicAdd(g.n_bad_source, bad);
        }
        __syncthreads();
        unsigned long long ss = 0, zz = 0;      // wrap like the reference's int64 squares
        for (int i = tid; i < op.length; i += kRowThreads) {
            const long long s = (long long)w[op.offset + i];
            const long long z = noise_at<I16>(g, op, i);
            ss += (unsigned long long)s * (unsigned long long)s;
            zz += (unsigned long long)z * (unsigned long long)z;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            ss += __shfl_xor(ss, off);
            zz += __shfl_xor(zz, off);
        }
        if ((tid & 63) == 0) {      // integer sums: the order does not matter
            atomicAdd(&sums[0], ss);
            atomicAdd(&sums[1], zz);
        }
        __syncthreads();
        const double s_rms = sqrt((double)(long long)sums[0] / (double)op.length);
        const double z_rms = sqrt((double)(long long)sums[1] / (double)op.length);
        const double wanted = sqrt(s_rms * s_rms / op.snr_ratio);
        const double den = z_rms + 1e-20;
        if (tid == 0) g.gains[o] = wanted / den;
        for (int i = tid; i < op.length; i += kRowThreads) {
            const long long s = (long long)w[op.offset + i];
            const long long z = noise_at<I16>(g, op, i);
            w[op.offset + i] = (double)s + ((double)z * wanted) / den;
        }
    }
    __syncthreads();
    for (int64_t i = tid; i < g.n; i += kRowThreads) row[i] = (float)w[i];
}

// ---------------------------------------------------------------- reverb: the convolution
//
// With t = 32 a + i the output index and the taps cut into blocks of 32,
//   c[32 a + i] = sum_{cb, j} x[32 (a - cb) + j] * h[32 cb + i - j]        (x and h zero outside their ranges)
// which is, per tap block cb, a [a-blocks, 32] x [32, 32] product: A = x seen as rows of 32 samples, shifted by cb rows,
// B = the Toeplitz block T_cb[j, i] = h[32 cb + i - j].  T is never stored: a lane reads its element straight out of h in LDS.
// A block of four waves owns 256 a-blocks (8192 outputs) of one utterance, wave w the a-blocks [64 w, 64 w + 64) as two 32 x 32
// accumulators that share every B operand.  The taps go by in chunks of kKc blocks (512 taps): a chunk stages the 271 rows of
// x it touches (row stride 33 floats: the lanes of an A operand are 32 rows apart) and 544 values of h, then runs 16 x 16 x 2
// MFMAs per wave with one LDS read per operand.  Tap blocks that only meet the zeros in front of x or behind it are skipped.

constexpr int kKc = 16;                           // tap blocks per chunk
constexpr int kConvThreads = 256;
constexpr int kMt = 2;                            // accumulators per wave
constexpr int kAb = 4 * kMt * 32;                 // a-blocks per block: 256
constexpr int kConvOut = 32 * kAb;                // outputs per block: 8192
constexpr int kXsRows = kAb + kKc - 1;            // 271
constexpr int kXsLd = 33;
constexpr int kHs = 32 * kKc + 32;                // hs[u] = h[32 c0 - 32 + u]

struct ReverbArgs {
    float* waves;
    int64_t ld, n;
    const float* rirs;
    int32_t n_rirs;
    int64_t l_max;
    const int32_t* rir_len;
    const int32_t* rir_of_utt;
    float* conv;                 // [batch, n]
    float* part_max;             // [batch, blocks_per_utt]
    int32_t blocks_per_utt;
    unsigned long long* n_bad_rir;
};

// the utterance's response length, 0 when the row is to be left alone (no rir, or one that is out of range)
__device__ __forceinline__ int rir_taps(const ReverbArgs& g, int b, int* rir_out) {
    const int r = g.rir_of_utt[b];
    if (r < 0 || r >= g.n_rirs) return 0;
    const int L = g.rir_len[r];
    if (L < 1 || (int64_t)L > g.l_max) return 0;
    *rir_out = r;
    return L;
}

__global__ __launch_bounds__(kConvThreads) void aug_reverb_conv_kernel(const ReverbArgs g) {
    __shared__ float xs[kXsRows * kXsLd];
    __shared__ float hs[kHs];
    __shared__ float red[kConvThreads / 64];
    const int b = blockIdx.y, blk = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, kh = lane >> 5;
    int rir = 0;
    const int L = rir_taps(g, b, &rir);
    if (L == 0) return;                                     // the apply kernel returns too: nothing of this row is read
    const int n = (int)g.n;
    const int64_t n_out = (int64_t)n + L - 1;
    const int a0 = blk * kAb;
    if ((int64_t)a0 * 32 >= n_out) {                        // past this utterance's outputs
        if (tid == 0) g.part_max[(int64_t)b * g.blocks_per_utt + blk] = 0.f;
        return;
    }
    const float* x = g.waves + (int64_t)b * g.ld;
    const float* h = g.rirs + (int64_t)rir * g.l_max;
    const int c_tot = (L + 30) / 32 + 1;                    // tap blocks that hold a tap: 32 cb + i - j <= L - 1, i - j >= -31
    const int c_lo = max(0, a0 - (n - 1) / 32);             // below it every row a - cb lies behind x
    const int c_hi = min(c_tot, a0 + kAb);                  // from it on every row a - cb lies in front of x

    f32x16v acc[kMt];
#pragma unroll
    for (int m = 0; m < kMt; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[m][e] = 0.f;
    const float* xa = xs + (kMt * 32 * wave + i + kKc - 1) * kXsLd + kh;      // + (32 m - cc) * kXsLd + 2 jj
    const float* hb = hs + 32 + i - kh;                                        // + 32 cc - 2 jj

    for (int c0 = c_lo; c0 < c_hi; c0 += kKc) {
        __syncthreads();                                    // the chunk before is consumed
        const int q0 = a0 - c0 - kKc + 1;                   // the x row that lands in xs row 0
        for (int idx = tid; idx < kXsRows * 32; idx += kConvThreads) {
            const int q = idx >> 5, j = idx & 31;
            const int64_t at = (int64_t)(q0 + q) * 32 + j;
            xs[q * kXsLd + j] = at >= 0 && at < n ? x[at] : 0.f;
        }
        for (int u = tid; u < kHs; u += kConvThreads) {
            const int k = 32 * c0 - 32 + u;
            hs[u] = k >= 0 && k < L ? h[k] : 0.f;
        }
        __syncthreads();
#pragma unroll 2
        for (int cc = 0; cc < kKc; ++cc) {
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) {
                const float bv = hb[32 * cc - 2 * jj];
#pragma unroll
                for (int m = 0; m < kMt; ++m)
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[(32 * m - cc) * kXsLd + 2 * jj], bv, acc[m], 0, 0, 0);
            }
        }
    }
    // accumulator element e of lane (i, kh): row = (e & 3) + 8 (e >> 2) + 4 kh, col = i
    float* conv = g.conv + (int64_t)b * g.n;
    float peak = 0.f;
#pragma unroll
    for (int m = 0; m < kMt; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int a = a0 + kMt * 32 * wave + 32 * m + (e & 3) + 8 * (e >> 2) + 4 * kh;
            const int64_t t = (int64_t)a * 32 + i;
            if (t < n_out) peak = fmaxf(peak, fabsf(acc[m][e]));
            if (t < n) conv[t] = acc[m][e];
        }
    peak = block_max(peak, red, kConvThreads / 64);
    if (tid == 0) g.part_max[(int64_t)b * g.blocks_per_utt + blk] = peak;
}

__global__ __launch_bounds__(kRowThreads) void aug_reverb_apply_kernel(const ReverbArgs g) {
    __shared__ float red[kRowWaves];
    const int b = blockIdx.x, tid = threadIdx.x;
    int rir = 0;
    const int L = rir_taps(g, b, &rir);
    if (L == 0) {
        if (tid == 0 && g.rir_of_utt[b] >= 0) atomicAdd(g.n_bad_rir, 1ull);
        return;
    }
    float* x = g.waves + (int64_t)b * g.ld;
    const float* conv = g.conv + (int64_t)b * g.n;
    float mx = 0.f, mc = 0.f;
    for (int64_t t = tid; t < g.n; t += kRowThreads) mx = fmaxf(mx, fabsf(x[t]));
    for (int k = tid; k < g.blocks_per_utt; k += kRowThreads) mc = fmaxf(mc, g.part_max[(int64_t)b * g.blocks_per_utt + k]);
    mx = block_max(mx, red, kRowWaves);
    mc = block_max(mc, red, kRowWaves);
    const float scale = mx / mc;      // 0 / 0 = NaN for an all-zero utterance or response, as the reference
    for (int64_t t = tid; t < g.n; t += kRowThreads) x[t] = x[t] + conv[t] * scale;
}

// ---------------------------------------------------------------- normalize

__global__ __launch_bounds__(kRowThreads) void aug_normalize_kernel(float* waves, int64_t ld, int64_t n) {
    __shared__ float red[kRowWaves];
    float* x = waves + (int64_t)blockIdx.x * ld;
    const int tid = threadIdx.x;
    float hi = -INFINITY, neg_lo = -INFINITY;      // the minimum as the maximum of -x
    for (int64_t t = tid; t < n; t += kRowThreads) {
        const float v = x[t];
        hi = fmaxf(hi, v);
        neg_lo = fmaxf(neg_lo, -v);
    }
    hi = block_max(hi, red, kRowWaves);
    const float lo = -block_max(neg_lo, red, kRowWaves);
    const float range = hi - lo;                   // = max(x - min): the rounding is monotonic
    for (int64_t t = tid; t < n; t += kRowThreads) x[t] = (x[t] - lo) / range;      // 0 / 0 = NaN for a constant row
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_aerr;

constexpr int64_t kMaxN = (int64_t)1 << 28, kMaxTaps = (int64_t)1 << 24, kMaxOps = (int64_t)1 << 24;

int check_waves(const float* waves, int64_t ld, int32_t batch, int64_t n) {
    if (!waves) return g_aerr.fail(XVEC_ERR_ARG, "null pointer: waves");
    if (batch < 1 || batch > 65535) return g_aerr.fail(XVEC_ERR_ARG, "batch = %d: must be in 1 .. 65535", batch);
    if (n < 1) return g_aerr.fail(XVEC_ERR_ARG, "n = %lld: need at least one sample", (long long)n);
    if (n > kMaxN) return g_aerr.fail(XVEC_ERR_TOO_LARGE, "n = %lld exceeds 2^28", (long long)n);
    if (ld < n) return g_aerr.fail(XVEC_ERR_ARG, "ld = %lld is smaller than n = %lld", (long long)ld, (long long)n);
    return XVEC_OK;
}

struct MixPlan {
    double* work;
    xvec_aug_op* ops;
    size_t total;
};

MixPlan make_mix_plan(void* workspace, int32_t batch, int64_t n, int64_t n_ops) {
    MixPlan p{};
    Carver c(workspace);
    p.work = c.take<double>((size_t)batch * (size_t)n);
    p.ops = c.take<xvec_aug_op>((size_t)std::max<int64_t>(n_ops, 1));
    p.total = c.total();
    return p;
}

struct ReverbPlan {
    float* conv;
    float* part_max;
    int32_t blocks_per_utt;
    size_t total;
};

ReverbPlan make_reverb_plan(void* workspace, int32_t batch, int64_t n, int64_t l_max) {
    ReverbPlan p{};
    p.blocks_per_utt = (int32_t)((n + l_max - 1 + kConvOut - 1) / kConvOut);
    Carver c(workspace);
    p.conv = c.take<float>((size_t)batch * (size_t)n);
    p.part_max = c.take<float>((size_t)batch * (size_t)p.blocks_per_utt);
    p.total = c.total();
    return p;
}

bool sizes_ok(int32_t batch, int64_t n) { return batch >= 1 && batch <= 65535 && n >= 1 && n <= kMaxN; }

int check_ops(const xvec_aug_op* ops, int64_t n_ops, int32_t batch, int64_t n, int64_t n_srcs) {
    for (int64_t o = 0; o < n_ops; ++o) {
        const xvec_aug_op& op = ops[o];
        if (op.utt < 0 || op.utt >= batch)
            return g_aerr.fail(XVEC_ERR_ARG, "op %lld: utt = %d is outside the batch of %d", (long long)o, op.utt, batch);
        if (o > 0 && op.utt < ops[o - 1].utt)
            return g_aerr.fail(XVEC_ERR_ARG, "op %lld: the ops are not sorted by utterance (utt %d after %d)", (long long)o, op.utt,
                               ops[o - 1].utt);
        if (op.length < 1 || op.offset < 0 || (int64_t)op.offset + op.length > n)
            return g_aerr.fail(XVEC_ERR_ARG, "op %lld: the slice [%d, %lld) leaves the row of %lld samples", (long long)o, op.offset,
                               (long long)op.offset + op.length, (long long)n);
        if (op.n_src < 0 || op.first_src < 0 || (int64_t)op.first_src + op.n_src > n_srcs)
            return g_aerr.fail(XVEC_ERR_ARG, "op %lld: sources [%d, %lld) lie outside the source list of %lld", (long long)o,
                               op.first_src, (long long)op.first_src + op.n_src, (long long)n_srcs);
        if (!(op.snr_ratio > 0.0) || op.snr_ratio > 1e300)
            return g_aerr.fail(XVEC_ERR_ARG, "op %lld: snr_ratio = %g must be positive and finite", (long long)o, op.snr_ratio);
    }
    return XVEC_OK;
}

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_aug_last_error(void) { return g_aerr.c_str(); }

size_t xvec_aug_mix_workspace_bytes(int32_t batch, int64_t n, int64_t n_ops) {
    if (!sizes_ok(batch, n) || n_ops < 0 || n_ops > kMaxOps) return 0;
    return make_mix_plan(nullptr, batch, n, n_ops).total;
}

int xvec_aug_mix(float* waves, int64_t ld, int32_t batch, int64_t n, const void* pool, int32_t pool_dtype, int32_t n_rows,
                 int64_t m_max, const int32_t* src_len, const xvec_aug_op* ops, int64_t n_ops, const xvec_aug_src* srcs,
                 int64_t n_srcs, double* gains_out, xvec_aug_status* status, void* workspace, size_t workspace_bytes,
                 xvec_stream stream) {
    int rc;
    if ((rc = check_waves(waves, ld, batch, n))) return rc;
    if (!pool || !src_len || !status || !workspace) return g_aerr.fail(XVEC_ERR_ARG, "null pointer: pool / src_len / status / workspace");
    if (pool_dtype != XVEC_AUG_POOL_F32 && pool_dtype != XVEC_AUG_POOL_I16)
        return g_aerr.fail(XVEC_ERR_ARG, "pool_dtype = %d: XVEC_AUG_POOL_F32 or XVEC_AUG_POOL_I16", pool_dtype);
    if (n_rows < 1 || m_max < 1 || m_max > 0x7fffffff)
        return g_aerr.fail(XVEC_ERR_ARG, "pool [%d, %lld]: both sizes must be at least 1", n_rows, (long long)m_max);
    if (n_ops < 0 || n_srcs < 0) return g_aerr.fail(XVEC_ERR_ARG, "n_ops = %lld, n_srcs = %lld: negative", (long long)n_ops, (long long)n_srcs);
    if (n_ops > kMaxOps) return g_aerr.fail(XVEC_ERR_TOO_LARGE, "n_ops = %lld exceeds 2^24", (long long)n_ops);
    if (n_ops > 0 && (!ops || !gains_out)) return g_aerr.fail(XVEC_ERR_ARG, "null pointer: ops / gains_out");
    if (n_srcs > 0 && !srcs) return g_aerr.fail(XVEC_ERR_ARG, "null pointer: srcs");
    if ((rc = check_ops(ops, n_ops, batch, n, n_srcs))) return rc;
    const MixPlan p = make_mix_plan(workspace, batch, n, n_ops);
    if ((rc = workspace_ok(workspace_bytes, p.total, g_aerr))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(&status->n_bad_source, 0, sizeof(int64_t), s);
    if (e != hipSuccess) return g_aerr.fail(XVEC_ERR_HIP, "clearing the status failed: %s", hipGetErrorString(e));
    if (n_ops == 0) return XVEC_OK;
    e = hipMemcpyAsync(p.ops, ops, (size_t)n_ops * sizeof(xvec_aug_op), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return g_aerr.fail(XVEC_ERR_HIP, "copying the op list failed: %s", hipGetErrorString(e));
    MixArgs g{};
    g.waves = waves;
    g.ld = ld;
    g.n = n;
    g.pool = pool;
    g.n_rows = n_rows;
    g.m_max = m_max;
    g.src_len = src_len;
    g.ops = p.ops;
    g.n_ops = (int32_t)n_ops;
    g.srcs = srcs;
    g.work = p.work;
    g.gains = gains_out;
    g.n_bad_source = reinterpret_cast<unsigned long long*>(&status->n_bad_source);
    if (pool_dtype == XVEC_AUG_POOL_I16) aug_mix_kernel<true><<<(unsigned)batch, kRowThreads, 0, s>>>(g);
    else aug_mix_kernel<false><<<(unsigned)batch, kRowThreads, 0, s>>>(g);
    return g_aerr.launch_ok("aug_mix_kernel");
}

size_t xvec_aug_reverb_workspace_bytes(int32_t batch, int64_t n, int64_t l_max) {
    if (!sizes_ok(batch, n) || l_max < 1 || l_max > kMaxTaps) return 0;
    return make_reverb_plan(nullptr, batch, n, l_max).total;
}

int xvec_aug_reverb(float* waves, int64_t ld, int32_t batch, int64_t n, const float* rirs, int32_t n_rirs, int64_t l_max,
                    const int32_t* rir_len, const int32_t* rir_of_utt, xvec_aug_status* status, void* workspace,
                    size_t workspace_bytes, xvec_stream stream) {
    int rc;
    if ((rc = check_waves(waves, ld, batch, n))) return rc;
    if (!rirs || !rir_len || !rir_of_utt || !status || !workspace)
        return g_aerr.fail(XVEC_ERR_ARG, "null pointer: rirs / rir_len / rir_of_utt / status / workspace");
    if (n_rirs < 1 || l_max < 1)
        return g_aerr.fail(XVEC_ERR_ARG, "rirs [%d, %lld]: both sizes must be at least 1", n_rirs, (long long)l_max);
    if (l_max > kMaxTaps) return g_aerr.fail(XVEC_ERR_TOO_LARGE, "l_max = %lld exceeds 2^24", (long long)l_max);
    const ReverbPlan p = make_reverb_plan(workspace, batch, n, l_max);
    if ((rc = workspace_ok(workspace_bytes, p.total, g_aerr))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = hipMemsetAsync(&status->n_bad_rir, 0, sizeof(int64_t), s);
    if (e != hipSuccess) return g_aerr.fail(XVEC_ERR_HIP, "clearing the status failed: %s", hipGetErrorString(e));
    ReverbArgs g{};
    g.waves = waves;
    g.ld = ld;
    g.n = n;
    g.rirs = rirs;
    g.n_rirs = n_rirs;
    g.l_max = l_max;
    g.rir_len = rir_len;
    g.rir_of_utt = rir_of_utt;
    g.conv = p.conv;
    g.part_max = p.part_max;
    g.blocks_per_utt = p.blocks_per_utt;
    g.n_bad_rir = reinterpret_cast<unsigned long long*>(&status->n_bad_rir);
    aug_reverb_conv_kernel<<<dim3((unsigned)p.blocks_per_utt, (unsigned)batch), kConvThreads, 0, s>>>(g);
    if ((rc = g_aerr.launch_ok("aug_reverb_conv_kernel"))) return rc;
    aug_reverb_apply_kernel<<<(unsigned)batch, kRowThreads, 0, s>>>(g);
    return g_aerr.launch_ok("aug_reverb_apply_kernel");
}

int xvec_aug_normalize(float* waves, int64_t ld, int32_t batch, int64_t n, xvec_stream stream) {
    int rc;
    if ((rc = check_waves(waves, ld, batch, n))) return rc;
    aug_normalize_kernel<<<(unsigned)batch, kRowThreads, 0, static_cast<hipStream_t>(stream)>>>(waves, ld, n);
    return g_aerr.launch_ok("aug_normalize_kernel");
}

}  // extern "C"
