// Statistics pooling of the training step's tail, forward and backward (C ABI: include/xvec_train.h), and what train_tail.hip
// shares with train_tail_ragged.hip.  Both kernels have a compile-time RAGGED variant over per-utterance valid-frame counts on
// the padded layout y5 [B, Tp, C]: the frames t >= len[b] are never read and their dy5 is written as 0.  The launchers are
// templates: a translation unit gets the kernels of the variant it names.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/xvec_hip.h"
#include "../../include/xvec_train.h"
#include "host_support.h"
#include "tdnn_common.h"

namespace xvec {

// The pooling step of a tail call: XVEC_OK or the code, with the message in the training calls' channel.
using TailPoolFn = int (*)(const float* y5, int B, int Tp, int C, const int32_t* lengths_dev, float* pooled, hipStream_t st);
using TailPoolBwdFn = int (*)(const float* y5, int B, int Tp, int C, const int32_t* lengths_dev, const float* pooled,
                              const float* dpooled, float* dy5, hipStream_t st);

// xvec_train_tail_forward / _backward with the pooling passed in (train_tail.hip); `lengths_dev` goes to it untouched.
int train_tail_forward(const float* y5, int32_t B, int32_t Tp, int32_t C, const float* W6, const float* b6, int32_t H,
                       const float* W7, const float* b7, const float* Wo, const float* bo, int32_t K, const int64_t* labels,
                       float* pooled, float* a6, float* a7, float* logits, float* loss, void* workspace, size_t workspace_bytes,
                       xvec_stream stream, TailPoolFn pool, const int32_t* lengths_dev);
int train_tail_backward(const float* dloss, const float* y5, int32_t B, int32_t Tp, int32_t C, const float* W6, int32_t H,
                        const float* W7, const float* Wo, int32_t K, const int64_t* labels, const float* pooled, const float* a6,
                        const float* a7, const float* logits, float* dy5, float* dW6, float* db6, float* dW7, float* db7,
                        float* dWo, float* dbo, void* workspace, size_t workspace_bytes, xvec_stream stream, TailPoolBwdFn pool_bwd,
                        const int32_t* lengths_dev);

namespace {

constexpr int kPoolRows = 32;                   // frames per block of the pooling backward

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// valid frames of utterance b: len[b] for a length in [2, Tp]; a length outside that range, which the host cannot see, gives the
// utterance no frames: its pooled row and its dy5 are 0
__device__ __forceinline__ int pooled_frames(const int32_t* __restrict__ len, int b, int Tp) {
    const int l = len[b];
    return l >= 2 && l <= Tp ? l : 0;
}

// A block takes 64 groups of W channels of one utterance: thread (group tid & 63, row group tid >> 6) walks the frames
// grp, grp + 4, ...; W = 4 reads 16 bytes per lane (C % 4 == 0, y5 16-byte aligned), W = 1 is the element-wise form.
template <int W>
__device__ __forceinline__ void load_w(const float* p, float (&v)[W]) {
    if constexpr (W == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}

// pooled[b][c] = mean, pooled[b][C + c] = unbiased std over the n frames, from s1 = sum (y - pivot) and s2 = sum (y - pivot)^2
// about the pivot y[b][0][c]: a channel that is constant over the utterance has s1 = s2 = 0 and an std of exactly 0.
// n = Tp, or with RAGGED the utterance's valid frames.
template <int W, bool RAGGED>
__global__ __launch_bounds__(256) void tail_pool_kernel(const float* __restrict__ y, int Tp, int C, float* __restrict__ pooled,
                                                        const int32_t* __restrict__ len) {
    __shared__ float sh[2][4][64 * W];
    const int tid = threadIdx.x, cg = tid & 63, grp = tid >> 6, b = blockIdx.y;
    const int c0 = (blockIdx.x * 64 + cg) * W;
    const bool ok = c0 < C;
    const int frames = RAGGED ? pooled_frames(len, b, Tp) : Tp;
    float piv[W], s1[W], s2[W];
#pragma unroll
    for (int j = 0; j < W; ++j) piv[j] = s1[j] = s2[j] = 0.f;
    if (ok && (!RAGGED || frames > 0)) {
        const float* base = y + (size_t)b * Tp * C + c0;
        load_w<W>(base, piv);
#pragma unroll 4
        for (int t = grp; t < frames; t += 4) {
            float v[W];
            load_w<W>(base + (size_t)t * C, v);
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const float d = v[j] - piv[j];
                s1[j] += d;
                s2[j] = fmaf(d, d, s2[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
        sh[0][grp][cg * W + j] = s1[j];
        sh[1][grp][cg * W + j] = s2[j];
    }
    __syncthreads();
    if (!ok || grp != 0) return;
    const float n = (float)frames;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const int i = cg * W + j;
        const float a1 = ((sh[0][0][i] + sh[0][1][i]) + sh[0][2][i]) + sh[0][3][i];
        const float a2 = ((sh[1][0][i] + sh[1][1][i]) + sh[1][2][i]) + sh[1][3][i];
        const float var = fmaxf(a2 - a1 * a1 / n, 0.f) / (n - 1.0f);
        const bool none = RAGGED && frames == 0;
        pooled[(size_t)b * 2 * C + c0 + j] = none ? 0.f : piv[j] + a1 / n;
        pooled[(size_t)b * 2 * C + C + c0 + j] = none ? 0.f : sqrtf(var);
    }
}

// dy5[b][t][c] = dmean / n + dstd (y5 - mean) / ((n - 1) std), the second term 0 where std == 0 (a SELECT on the factor);
// n = Tp, or with RAGGED the utterance's valid frames, and dy5 = 0 on the frames past them.
template <int W, bool RAGGED>
__global__ __launch_bounds__(256) void tail_pool_bwd_kernel(const float* __restrict__ y, int Tp, int C, const float* __restrict__ pooled,
                                                            const float* __restrict__ dpooled, float* __restrict__ dy,
                                                            const int32_t* __restrict__ len) {
    const int tid = threadIdx.x, cg = tid & 63, grp = tid >> 6, b = blockIdx.z;
    const int c0 = (blockIdx.x * 64 + cg) * W;
    if (c0 >= C) return;
    const int t0 = blockIdx.y * kPoolRows, t1 = min(Tp, t0 + kPoolRows);
    const int frames = RAGGED ? pooled_frames(len, b, Tp) : Tp;
    float mean[W], add[W], fac[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const size_t i = (size_t)b * 2 * C + c0 + j;
        const float sd = pooled[i + C];
        mean[j] = pooled[i];
        add[j] = dpooled[i] / (float)frames;
        fac[j] = sd > 0.f ? dpooled[i + C] / ((float)(frames - 1) * sd) : 0.f;
    }
    const size_t base = (size_t)b * Tp * C + c0;
#pragma unroll 4
    for (int t = t0 + grp; t < t1; t += 4) {
        float v[W];
        if (!RAGGED || t < frames) {
            load_w<W>(y + base + (size_t)t * C, v);
#pragma unroll
            for (int j = 0; j < W; ++j) v[j] = fmaf(fac[j], v[j] - mean[j], add[j]);
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) v[j] = 0.f;
        }
        if constexpr (W == 4) {
            *reinterpret_cast<f32x4*>(dy + base + (size_t)t * C) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
            dy[base + (size_t)t * C] = v[0];
        }
    }
}

template <bool RAGGED>
int launch_tail_pool(const float* y5, int B, int Tp, int C, const int32_t* lengths_dev, float* pooled, hipStream_t st) {
    if (C % 4 == 0 && aligned16(y5)) tail_pool_kernel<4, RAGGED><<<dim3((C / 4 + 63) / 64, B), 256, 0, st>>>(y5, Tp, C, pooled, lengths_dev);
    else tail_pool_kernel<1, RAGGED><<<dim3((C + 63) / 64, B), 256, 0, st>>>(y5, Tp, C, pooled, lengths_dev);
    return train_error_channel().launch_ok("tail_pool_kernel");
}

template <bool RAGGED>
int launch_tail_pool_bwd(const float* y5, int B, int Tp, int C, const int32_t* lengths_dev, const float* pooled, const float* dpooled,
                         float* dy5, hipStream_t st) {
    const int row_blocks = (Tp + kPoolRows - 1) / kPoolRows;
    if (row_blocks > 65535)
        return train_error_channel().fail(XVEC_ERR_TOO_LARGE, "Tp = %d frames: more than 65535 blocks of %d", Tp, kPoolRows);
    if (C % 4 == 0 && aligned16(y5) && aligned16(dy5))
        tail_pool_bwd_kernel<4, RAGGED><<<dim3((C / 4 + 63) / 64, row_blocks, B), 256, 0, st>>>(y5, Tp, C, pooled, dpooled, dy5, lengths_dev);
    else
        tail_pool_bwd_kernel<1, RAGGED><<<dim3((C + 63) / 64, row_blocks, B), 256, 0, st>>>(y5, Tp, C, pooled, dpooled, dy5, lengths_dev);
    return train_error_channel().launch_ok("tail_pool_bwd_kernel");
}

}  // namespace
}  // namespace xvec
