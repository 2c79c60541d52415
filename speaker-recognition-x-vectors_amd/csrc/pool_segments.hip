// Statistics pooling over arbitrary row ranges ("segments") of a row matrix: per segment and channel, the mean and the
// UNBIASED standard deviation of rows [row0, row0 + n) of y[rows][ldy]; out[i] = mean[0..C) ‖ std[0..C).  It pools sliding
// windows and speech segments out of ONE run of the frame-level stack over a whole recording (xvec_forward_segments): the valid
// convolutions make the layer-5 rows of a crop x[s : s + L] rows s .. s + L - 15 of the recording's, element for element.
//
//  * pool_segments_kernel -- one block of four waves per (segment, group of 64 lanes' channels).  One pass over the
//                            segment's rows with the segment's OWN first row as the pivot K (sums of (x-K), (x-K)^2, as
//                            stat_pool_kernel, pool.hip): a channel constant over the segment has every deviation exactly 0,
//                            so std == 0 and mean == the constant whatever the rows outside the segment hold.  Wave w takes
//                            rows w, w + 4, ..., four of them in flight; the four waves' sums meet in LDS in a fixed order:
//                            no atomics, repeat calls are bit-identical, and a segment's result depends on nothing but its
//                            rows.  fp32 or bf16 rows (bf16: widened in registers, no pass over the rows), 16-byte loads or
//                            element-wise.  An optional per-channel affine map of the rows (a deferred BatchNorm) is applied
//                            to the statistics.
//  * segment_rows_kernel  -- (utt, start, len) in input frames -> (row0, n) in layer 5's compact row layout.
//
// n == 1 gives a NaN std exactly like torch.std (0/0).  A segment that is empty or leaves [0, rows) reads nothing and gets NaN.
#include "pool_segments.h"

namespace xvec {

namespace {

template <bool BF, int VEC>
__device__ __forceinline__ void ld_row(const void* p, float (&v)[VEC]) {
    if constexpr (!BF && VEC == 4) {
        const float4 t = *static_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else if constexpr (BF && VEC == 8) {
        const uint4 t = *static_cast<const uint4*>(p);
        const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = __uint_as_float(w[j] << 16);
            v[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
        }
    } else if constexpr (BF) {
        v[0] = __uint_as_float((uint32_t)*static_cast<const uint16_t*>(p) << 16);
    } else {
        v[0] = *static_cast<const float*>(p);
    }
}

template <bool BF, int VEC>
__global__ __launch_bounds__(256) void pool_segments_kernel(const PoolSegArgs a) {
    __shared__ float red[2][3][64 * VEC];          // the sums of waves 1..3, for wave 0
    constexpr int ES = BF ? 2 : 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t seg = blockIdx.x;
    const int ch = (blockIdx.y * 64 + lane) * VEC;
    const bool active = ch < a.C;                  // (a vector's tail past C lies in the row's padding: read, never stored)
    const int64_t r0 = a.row0[seg];
    const int n = a.n[seg];
    float* o = a.out + seg * 2 * (int64_t)a.C;
    if (n <= 0 || r0 < 0 || r0 > a.rows - n) {     // block-uniform: nothing is read
        if (wave == 0 && active) {
#pragma unroll
            for (int k = 0; k < VEC; ++k)
                if (ch + k < a.C) o[ch + k] = o[a.C + ch + k] = __builtin_nanf("");
        }
        return;
    }
    float K[VEC], s1[VEC], s2[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { K[k] = 0.f; s1[k] = 0.f; s2[k] = 0.f; }
    if (active) {
        const char* base = static_cast<const char*>(a.y) + (r0 * a.ldy + ch) * ES;
        const int64_t rb = (int64_t)a.ldy * ES;    // row stride in bytes
        ld_row<BF, VEC>(base, K);
        int f = wave;
        for (; f + 12 < n; f += 16) {              // 4 independent rows in flight per wave
            float v0[VEC], v1[VEC], v2[VEC], v3[VEC];
            ld_row<BF, VEC>(base + f * rb, v0);
            ld_row<BF, VEC>(base + (f + 4) * rb, v1);
            ld_row<BF, VEC>(base + (f + 8) * rb, v2);
            ld_row<BF, VEC>(base + (f + 12) * rb, v3);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float d0 = v0[k] - K[k], d1 = v1[k] - K[k], d2 = v2[k] - K[k], d3 = v3[k] - K[k];
                s1[k] += (d0 + d1) + (d2 + d3);
                s2[k] += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
            }
        }
        for (; f < n; f += 4) {
            float v0[VEC];
            ld_row<BF, VEC>(base + f * rb, v0);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float d0 = v0[k] - K[k];
                s1[k] += d0;
                s2[k] += d0 * d0;
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            red[0][wave - 1][lane * VEC + k] = s1[k];
            red[1][wave - 1][lane * VEC + k] = s2[k];
        }
    }
    __syncthreads();
    if (wave == 0 && active) {
        const double dn = (double)n;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if (ch + k >= a.C) break;
            const int i = lane * VEC + k;
            const float t1 = (s1[k] + red[0][0][i]) + (red[0][1][i] + red[0][2][i]);
            const float t2 = (s2[k] + red[1][0][i]) + (red[1][1][i] + red[1][2][i]);
            // the merge in fp64, as pool_finalize_kernel: mean of (x - K), then the variance about it
            const double md = (double)t1 / dn;
            double var = ((double)t2 - (double)t1 * md) / (dn - 1.0);
            var = var > 0.0 ? var : 0.0;
            double mean = (double)K[k] + md, sd = sqrt(var);
            if (a.scale) {
                const double sc = (double)a.scale[ch + k], sh = (double)a.shift[ch + k];
                mean = sh + sc * mean;
                sd *= sc < 0.0 ? -sc : sc;
            }
            o[ch + k] = (float)mean;
            o[a.C + ch + k] = n > 1 ? (float)sd : __builtin_nanf("");
        }
    }
}

__global__ __launch_bounds__(256) void segment_rows_kernel(const int32_t* utt, const int32_t* start, const int32_t* len,
                                                           int64_t n_segments, const int64_t* offsets, int n_utts, int cum,
                                                           int64_t* row0, int32_t* n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_segments) return;
    const int u = utt[i];
    const int64_t st = start[i], ln = len[i];
    int64_t r = 0;
    int32_t cnt = 0;
    if (u >= 0 && u < n_utts && st >= 0 && ln > cum) {
        const int64_t lo = offsets[u], hi = offsets[u + 1];
        if (lo + st + ln <= hi) {
            r = lo - (int64_t)cum * u + st;
            cnt = (int32_t)(ln - cum);
        }
    }
    row0[i] = r;
    n[i] = cnt;
}

template <bool BF, int VEC>
hipError_t launch_one(const PoolSegArgs& a, hipStream_t s) {
    dim3 grid((unsigned)a.n_segments, (unsigned)((a.C + 64 * VEC - 1) / (64 * VEC)));
    pool_segments_kernel<BF, VEC><<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace

bool pool_segments_vector(const void* y, int elem, int ldy, int C) {
    const int es = elem ? 2 : 4, vec = 16 / es;
    return (reinterpret_cast<uintptr_t>(y) & 15) == 0 && ((int64_t)ldy * es) % 16 == 0 && ((int64_t)C + vec - 1) / vec * vec <= ldy;
}

hipError_t launch_pool_segments(const PoolSegArgs& a, hipStream_t s) {
    if (a.n_segments <= 0 || a.C <= 0) return hipSuccess;
    if (a.n_segments > 0x7fffffff || a.ldy < a.C) return hipErrorInvalidValue;
    const bool v16 = pool_segments_vector(a.y, a.elem, a.ldy, a.C);
    if (a.elem) return v16 ? launch_one<true, 8>(a, s) : launch_one<true, 1>(a, s);
    return v16 ? launch_one<false, 4>(a, s) : launch_one<false, 1>(a, s);
}

hipError_t launch_segment_rows(const int32_t* utt, const int32_t* start, const int32_t* len, int64_t n_segments,
                               const int64_t* offsets, int n_utts, int cum, int64_t* row0, int32_t* n, hipStream_t s) {
    if (n_segments <= 0) return hipSuccess;
    segment_rows_kernel<<<(unsigned)((n_segments + 255) / 256), 256, 0, s>>>(utt, start, len, n_segments, offsets, n_utts, cum,
                                                                            row0, n);
    return hipGetLastError();
}

}  // namespace xvec
