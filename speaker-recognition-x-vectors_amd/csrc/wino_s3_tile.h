// What the two Winograd F(2,3) kernels on bf16_split3 operands share (tdnn_wino_s3.hip: 64 pairs x 128 channels on four waves;
// tdnn_wino_s3w.hip: 64 pairs x 256 channels on eight): the load stream's step, the staging of a chunk (input rows -> V planes
// in the LDS image of wino_s3_lds_map.h), the fragment registers and the pinned product schedule of a wave's K loop.  The
// WS3_* macros stay defined behind this header; the kernels #undef them at their end.
#pragma once
#include "tdnn_wino_rows.h"
#include "wino_s3_lds_map.h"

namespace xvec {
namespace wino {

// Step the load stream to the next chunk; after a tile's last chunk, to chunk 0 of the block's next tile.  Past the block's
// last chunk it stays put (the look-ahead re-reads that chunk; the data is never used).
// STEP = 2 (n_chunks even): a stream over the chunks of one parity (tdnn_wino_s3w.hip: two wave sets stage alternate chunks).
template <int STEP = 1>
__device__ __forceinline__ void s3_advance(const TdnnArgs& a, Ctx& cx, const Lane& ln, int* tbl, int64_t* tblh, int n_chunks) {
    if (cx.kc + STEP < n_chunks) {
        cx.kc += STEP;
    } else {
        const int64_t g_rem = cx.g_end - cx.g_s;
        const int64_t g_next = cx.g_s + (g_rem < 2 ? g_rem : 2);
        if (g_next < cx.g_end) {
            cx.g_s = g_next;
            cx.q0 = g_next * 32;
            cx.lp ^= 1;
            set_rows(a, cx, ln, tbl, tblh);
            cx.kc &= STEP - 1;
        }
    }
}

struct S3Stage {
    float4 x0, x1, x2, x3;
};

// the four input rows of this thread's pair (group `grp`: 0 -> set_rows' pair q0 + r0, 1 -> q0 + r0 + 32) at the chunk cx
// points at.  Rows x1, x2 are x0 + d, x0 + 2d: the scalar offset carries the shift; x3 has a lane offset of its own.
__device__ __forceinline__ void s3_gld(const Ctx& cx, bool grp, S3Stage& s) {
    const int xo0 = grp ? cx.x01 : cx.x00, xo3 = grp ? cx.x31 : cx.x30;
    const int so = cx.kc * (kS3K * 4);
    s.x0 = buf_load16(cx.xrsrc, xo0, so);
    s.x1 = buf_load16(cx.xrsrc, xo0, so + cx.drb);
    s.x2 = buf_load16(cx.xrsrc, xo0, so + 2 * cx.drb);
    s.x3 = buf_load16(cx.xrsrc, xo3, so);
}

// V_k = x0-x2 | x1+x2 | x2-x1 | x1-x3 in fp32, each split into hi | mid | lo -> LDS buffer B (st: this thread's 8 bytes)
__device__ __forceinline__ void s3_vstore(char* B, int st, const S3Stage& s) {
    const float4 v[4] = {
        make_float4(s.x0.x - s.x2.x, s.x0.y - s.x2.y, s.x0.z - s.x2.z, s.x0.w - s.x2.w),
        make_float4(s.x1.x + s.x2.x, s.x1.y + s.x2.y, s.x1.z + s.x2.z, s.x1.w + s.x2.w),
        make_float4(s.x2.x - s.x1.x, s.x2.y - s.x1.y, s.x2.z - s.x1.z, s.x2.w - s.x1.w),
        make_float4(s.x1.x - s.x3.x, s.x1.y - s.x3.y, s.x1.z - s.x3.z, s.x1.w - s.x3.w)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        u32x2 hi, mid, lo;
        split3(v[k], hi, mid, lo);
        *reinterpret_cast<u32x2*>(B + (3 * k + 0) * kS3Plane + st) = hi;
        *reinterpret_cast<u32x2*>(B + (3 * k + 1) * kS3Plane + st) = mid;
        *reinterpret_cast<u32x2*>(B + (3 * k + 2) * kS3Plane + st) = lo;
    }
}

// The U-plane fragments (hi | mid | lo) of the four products of a chunk, this wave's column, and the A fragments of one product
// (a: pair group 0, b: pair group 1).  Named members, not arrays: the K loop below is pinned with scheduling barriers.
struct S3U {
    float4 w00, w01, w02, w10, w11, w12, w20, w21, w22, w30, w31, w32;
};
struct S3Frag {
    float4 a0, a1, a2, b0, b1, b2;
};

// one MFMA of s3_mfma6's six (tdnn_common.h: the same products in the same order into the same accumulator)
#define WS3_MF(acc_, x_, w_) \
    acc_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x_), __builtin_bit_cast(bf16x8, w_), acc_, 0, 0, 0);
// one A fragment of product kn_ of the chunk in buffer B_: plane pl_ of pair group g_ (0: ln.a_rd, 1: a_rd1)
#define WS3_RD(dst_, B_, kn_, pl_, g_) \
    dst_ = *reinterpret_cast<const float4*>((B_) + (3 * (kn_) + (pl_)) * kS3Plane + ((g_) ? a_rd1 : ln.a_rd));
// the three U fragments of product K_ of chunk it + 1; the stream wraps to chunk 0 past the tile's last chunk (the next tile
// of the block is in the same channel column)
#define WS3_ULD(K_)                                                                   \
    {                                                                                 \
        int c_ = it + 1;                                                              \
        if (c_ >= n_chunks) c_ -= n_chunks;                                           \
        u.w##K_##0 = buf_load16(ursrc, ln.b_rd, ((4 * c_ + K_) * 3 + 0) * 1024);      \
        u.w##K_##1 = buf_load16(ursrc, ln.b_rd, ((4 * c_ + K_) * 3 + 1) * 1024);      \
        u.w##K_##2 = buf_load16(ursrc, ln.b_rd, ((4 * c_ + K_) * 3 + 2) * 1024);      \
    }
// Product K_ of a tile of two pair groups.  The two fragment sets roll: pair group 1's fragments of this product are read
// from S behind the first MFMAs of pair group 0, pair group 0's of product kn_ (of the chunk in buffer NB_) behind the first
// MFMAs of pair group 1 -- each into registers whose last MFMA has just issued, ONE ds_read_b128 per MFMA gap (MI355X: up to
// two per gap are free), in the order the MFMAs take them (lo | mid | hi: the waits are counted), each five MFMAs ahead of
// its use.  24 fragment registers, as without look-ahead.
// BAR_: the chunk's barrier, between the two pair groups of product 3 (see the loop).
#define WS3_PRODUCT2(K_, NB_, kn_, BAR_)                                                                   \
    {                                                                                                      \
        WS3_MF(acc##K_##_0, f.a2, u.w##K_##0) WS3_RD(f.b2, S, K_, 2, 1) SB();                              \
        WS3_MF(acc##K_##_0, f.a1, u.w##K_##1) WS3_RD(f.b1, S, K_, 1, 1) SB();                              \
        WS3_MF(acc##K_##_0, f.a0, u.w##K_##2) WS3_RD(f.b0, S, K_, 0, 1) SB();                              \
        WS3_MF(acc##K_##_0, f.a1, u.w##K_##0) WS3_MF(acc##K_##_0, f.a0, u.w##K_##1) WS3_MF(acc##K_##_0, f.a0, u.w##K_##0) SB(); \
        BAR_                                                                                               \
        WS3_MF(acc##K_##_1, f.b2, u.w##K_##0) WS3_RD(f.a2, NB_, kn_, 2, 0) SB();                           \
        WS3_MF(acc##K_##_1, f.b1, u.w##K_##1) WS3_RD(f.a1, NB_, kn_, 1, 0) SB();                           \
        WS3_MF(acc##K_##_1, f.b0, u.w##K_##2) WS3_RD(f.a0, NB_, kn_, 0, 0) SB();                           \
        WS3_MF(acc##K_##_1, f.b1, u.w##K_##0) WS3_MF(acc##K_##_1, f.b0, u.w##K_##1) WS3_MF(acc##K_##_1, f.b0, u.w##K_##0) SB(); \
        WS3_ULD(K_)                                                                                        \
        SB();                                                                                              \
    }
// Product K_ of a tile of one pair group (a block's odd last tile): the second set's registers are free, so the fragments of
// product kn_ go to set N_ while this product runs on set C_ (a | b, alternating; product 0 runs on a).  BAR_ comes first:
// product 3's own fragments were read a product ago, and the next chunk's must be read behind it.
#define WS3_PRODUCT1(K_, C_, N_, NB_, kn_, BAR_)                                                           \
    {                                                                                                      \
        BAR_                                                                                               \
        WS3_MF(acc##K_##_0, f.C_##2, u.w##K_##0) WS3_RD(f.N_##2, NB_, kn_, 2, 0) SB();                     \
        WS3_MF(acc##K_##_0, f.C_##1, u.w##K_##1) WS3_RD(f.N_##1, NB_, kn_, 1, 0) SB();                     \
        WS3_MF(acc##K_##_0, f.C_##0, u.w##K_##2) WS3_RD(f.N_##0, NB_, kn_, 0, 0) SB();                     \
        WS3_MF(acc##K_##_0, f.C_##1, u.w##K_##0) WS3_MF(acc##K_##_0, f.C_##0, u.w##K_##1) WS3_MF(acc##K_##_0, f.C_##0, u.w##K_##0) SB(); \
        WS3_ULD(K_)                                                                                        \
        SB();                                                                                              \
    }

// Chunk `it` of a tile's K loop (s3_tile: the schedule).  head: the staged chunk, it + 1, -> the other buffer (free: every wave
// passed the barrier behind its last read of chunk it - 1), then the load stream steps STEP_ chunks on and the staging
// registers receive the chunk it points at.  HEAD_ false: a chunk without a head -- the other wave set stages it
// (tdnn_wino_s3w.hip, STEP_ 2), or a knock-out build; with STEP_ 1 the stream still steps.
#define WS3_CHUNK(HEAD_, STEP_) \
{ \
    const char* S = lds + (it & 1) * kS3Stage; \
    char* Sn = lds + ((it & 1) ^ 1) * kS3Stage; \
    if constexpr ((HEAD_)) s3_vstore(Sn, ln.st_off, st); \
    if constexpr ((HEAD_) || (STEP_) == 1) s3_advance<STEP_>(a, cx, ln, tbl, tblh, n_chunks); \
    if constexpr ((HEAD_)) s3_gld(cx, grp, st); \
    SB(); \
    if constexpr (G > 1) { \
        WS3_PRODUCT2(0, S, 1, ) \
        WS3_PRODUCT2(1, S, 2, ) \
        WS3_PRODUCT2(2, S, 3, ) \
        WS3_PRODUCT2(3, Sn, 0, __syncthreads(); SB();) \
    } else { \
        WS3_PRODUCT1(0, a, b, S, 1, ) \
        WS3_PRODUCT1(1, b, a, S, 2, ) \
        WS3_PRODUCT1(2, a, b, S, 3, ) \
        WS3_PRODUCT1(3, b, a, Sn, 0, __syncthreads(); SB();) \
    } \
}

}  // namespace wino
}  // namespace xvec
