// Device code of the 128x128 frame-level kernel family (tdnn_layer.hip: header comment there), shared by the translation
// units that instantiate it: tdnn_layer.hip (tdnn_kernel, fp32 / bf16 / bf16x3), tdnn_split3.hip (tdnn_split3_kernel) and
// tdnn_split3w.hip (tdnn_split3w_kernel: the pooling S3 body on 384-channel tiles, template parameter WS = the wave set).
#pragma once
#include <cstdlib>

#include "tdnn_common.h"

namespace xvec {

constexpr int kBM = 128, kBN = 128;
constexpr int kStageFloats = (kBM + kBN) * kBK;   // one LDS buffer: A tile then B tile
constexpr int kConstFloats = 3 * kBN;             // bias | scale | shift of the block's 128 channels (pooling: bias | bias - K | -K)
constexpr int kLdsBytes = (2 * kStageFloats + kConstFloats) * 4;

#ifdef XVEC_DIAG
// Diagnostic build only (make DIAG=1): s_memtime stamps of wave 0 of every block (one copy per translation unit; xvec_diag_read
// reads tdnn_layer.hip's)
static __device__ unsigned long long g_diag[8 * 8192];
#endif

// Per-thread state of one tile walk.  Global reads go through raw buffer loads: a block-uniform
// descriptor per operand (rebased at the tile origin), a uniform scalar byte offset (tap row
// shift, row group, chunk column) and ONE 32-bit per-thread byte offset per operand, so no
// per-load 64-bit address is ever computed or kept in VGPRs.
struct Ctx {
    __amdgpu_buffer_rsrc_t xrsrc;   // X + m0*ldx  (tile the load stream is in)
    __amdgpu_buffer_rsrc_t wrsrc;   // W + n0*k_pad
    int x_base;          // r0*ldx*ES + c*16 bytes    (per thread)
    int ur0, ur1, ur2, ur3;   // u(row r0+32j of the tile)*span: rows to add to re-base into the input layout
    int xo0, xo1, xo2, xo3;   // x_base + ur_j*ldx*ES
    int w_toff;          // r0*k_pad*ES + c*16 bytes
    __amdgpu_buffer_rsrc_t wfrsrc;   // bf16: fragment-major weights of this wave's 32-channel column tile
    int wf_voff;         // lane*16
    int r0;
    int u_tile;          // utterance holding row m0 (block-uniform), and the first row of the next one
    int64_t off_next;
    int64_t m0;          // first flat row of the tile the load stream is in
    int64_t g_s, g_end;  // that tile's first row group; end of this block's row range
    PoolCur pool;        // compute side: pooling cursor (POOL variants)
    bool pivot_set;      // POOL: the block's pooling pivots are in LDS (false until its first tile's epilogue)
    int tap, kc, itl;    // next chunk to fetch: (tap, kc) and its linear index within the tile
    int es;              // bytes per input element (4: fp32, 2: bf16)
};

// eight fp32 values -> eight bf16 in the 16 bytes of a staging register (round to nearest even, as pack_rows)
__device__ __forceinline__ float4 cvt8_bf16(const float4& lo, const float4& hi) {
    typedef __bf16 bf16x8v __attribute__((ext_vector_type(8)));
    typedef float f32x8v __attribute__((ext_vector_type(8)));
    const f32x8v f8 = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const f32x4 b4 = __builtin_bit_cast(f32x4, __builtin_convertvector(f8, bf16x8v));
    return make_float4(b4.x, b4.y, b4.z, b4.w);
}

// per-thread input offsets of the four staging rows (r0 + 32j) of the tile the stream is in: the
// compact output row p of utterance u reads input rows p + u*span (+ tap shift).  The utterance of
// the tile's first row is tracked incrementally (cx.u_tile / cx.off_next: tiles only move
// forward); the few utterance boundaries inside the tile are walked with block-uniform values
// (scalar loads of the offsets for ragged batches) and each lane just counts how many of them its
// rows have passed -- no division, and no vector-memory load whose wait would drain the
// staging loads in flight.
// The fixed-length and the ragged case are two separate code paths on purpose: sharing one loop made
// hipcc put the ragged path's s_waitcnt vmcnt(0) (for the offsets load) on the fixed path too,
// draining the 16 staging loads in flight at every tile change.
template <bool RAGGED>
__device__ __forceinline__ void set_tile_rows_impl(const TdnnArgs& a, Ctx& cx) {
    const int n_last = a.out_map.n_utts - 1;
    const int64_t t_out = a.out_map.fixed_T - a.out_map.cum;          // fixed-length: rows per utterance
    auto next_off = [&](int u) -> int64_t {                            // first row of utterance u+1
        if (RAGGED) return a.out_map.offsets[u + 1] - (int64_t)(u + 1) * a.out_map.cum;
        return (int64_t)(u + 1) * t_out;
    };
    while (cx.m0 >= cx.off_next && cx.u_tile < n_last) {
        cx.u_tile = __builtin_amdgcn_readfirstlane(cx.u_tile + 1);
        cx.off_next = next_off(cx.u_tile);
    }
    const int64_t p = cx.m0 + cx.r0;
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    int u = cx.u_tile;
    int64_t nxt = cx.off_next;
    while (nxt < cx.m0 + 128 && u < n_last) {       // block-uniform walk over the boundaries in the tile
        c0 += (p >= nxt) ? 1 : 0;
        c1 += (p + 32 >= nxt) ? 1 : 0;
        c2 += (p + 64 >= nxt) ? 1 : 0;
        c3 += (p + 96 >= nxt) ? 1 : 0;
        u = __builtin_amdgcn_readfirstlane(u + 1);
        nxt = next_off(u);
    }
    const int rb = a.ldx * cx.es;
    cx.ur0 = (cx.u_tile + c0) * a.span;
    cx.ur1 = (cx.u_tile + c1) * a.span;
    cx.ur2 = (cx.u_tile + c2) * a.span;
    cx.ur3 = (cx.u_tile + c3) * a.span;
    cx.xo0 = cx.x_base + cx.ur0 * rb;
    cx.xo1 = cx.x_base + cx.ur1 * rb;
    cx.xo2 = cx.x_base + cx.ur2 * rb;
    cx.xo3 = cx.x_base + cx.ur3 * rb;
}

__device__ __forceinline__ void set_tile_rows(const TdnnArgs& a, Ctx& cx) {
    if (a.span == 0) {
        cx.ur0 = cx.ur1 = cx.ur2 = cx.ur3 = 0;
        cx.xo0 = cx.xo1 = cx.xo2 = cx.xo3 = cx.x_base;
        return;
    }
    if (a.out_map.offsets == nullptr) set_tile_rows_impl<false>(a, cx);
    else set_tile_rows_impl<true>(a, cx);
}

// Step the load stream to the next K-chunk.  The stream is continuous over the block's tiles:
// after the last chunk of a tile it moves to chunk 0 of the next tile (same channel column, next
// <=4 row groups), so a tile's first chunks are already in flight / in LDS when its MFMAs start
// and only the first tile of a block pays a prologue.  Past the block's last chunk it stays put
// (the look-ahead of the final chunks re-reads that chunk; the data is never used).
// Activation descriptor of the tile at row cx.m0.  GUARD (first layer): X is the caller's tensor,
// not a padded workspace buffer, so the descriptor ends with it and rows past the end read as 0.
template <int GUARD>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t x_rsrc(const TdnnArgs& a, const Ctx& cx) {
    // GUARD == 2: the caller's rows are fp32 and are rounded to bf16 on their way into the staging registers
    // (the separate pack_rows pass of the bf16 path: 7.4 MB read + 3.7 MB written + a launch per batch)
    const int src_es = GUARD == 2 ? 4 : cx.es;
    const int64_t off = cx.m0 * (int64_t)a.ldx * src_es;
    if (GUARD) return make_rsrc_bounded(a.X, off, a.x_bytes ? a.x_bytes : a.x_rows * (int64_t)a.ldx * src_es);
    return make_rsrc(static_cast<const char*>(a.X) + off);
}

template <int GUARD, bool X3>
__device__ __forceinline__ void advance(const TdnnArgs& a, Ctx& cx, int n_chunks) {
    if (cx.itl + 1 < n_chunks) {
        // taps innermost: consecutive chunks re-read the same 128-byte slab of activation rows,
        // shifted by the dilation, while it is still in L2 (the packed weights follow this order)
        ++cx.itl;
        if (++cx.tap == a.n_taps) {
            cx.tap = 0;
            ++cx.kc;
        }
    } else {
        const int64_t g_rem = cx.g_end - cx.g_s;
        const int64_t g_next = cx.g_s + (g_rem < 4 ? g_rem : 4);
        if (g_next < cx.g_end) {
            cx.g_s = g_next;
            cx.m0 = g_next * 32;
            cx.xrsrc = x_rsrc<GUARD>(a, cx);
            set_tile_rows(a, cx);
            cx.itl = 0;
            cx.kc = 0;
            cx.tap = 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The main loop is written with token-pasting macros over NAMED registers (sA<i>_<set>,
// fa<i>_<fset>, acc<i>): register arrays, even with compile-time indices through inlined
// lambdas, were left in scratch memory by hipcc (ROCm 7.2) once scheduling barriers were present.
// G (row groups of the tile, 1..4) is a template parameter; ops of absent groups vanish.
// ---------------------------------------------------------------------------------------------
#define XV_KO(q_) ((((2 * (q_)) + h) ^ sw) << 2)
// fragment reads (LDS -> VGPR) of k-group q_ into fragment set f_ from buffer base S_
#define XV_FRG_A(i_, q_, f_, S_) \
    if constexpr (G > i_) { rg.fa##i_##_##f_ = *reinterpret_cast<const float4*>((S_) + a_rd + i_ * 32 * kBK + XV_KO(q_)); }
// fp32: B fragment from the LDS image.  bf16: B fragments never touch LDS (see XV_GLB below).
#define XV_FRG_B(q_, f_, S_) \
    if constexpr (!INBF) { rg.fb_##f_ = *reinterpret_cast<const float4*>((S_) + b_rd + XV_KO(q_)); }
// LDS stores of staging set n_ into LDS buffer n_
#define XV_LST_A(i_, n_) \
    if constexpr (G > i_) { *reinterpret_cast<float4*>(smem + n_ * kStageFloats + st_off + i_ * 32 * kBK) = rg.sA##i_##_##n_; }
// the second half of an LDS buffer: fp32 -> the weight tile; bf16x3 -> the lo plane of the
// activation tile (same rows, x_plane_bytes further on in global memory); plain bf16 -> unused
#define XV_LST_B(j_, n_)                                                                                  \
    if constexpr (X3) {                                                                                   \
        if constexpr (G > j_) *reinterpret_cast<float4*>(smem + n_ * kStageFloats + st_off + kBM * kBK + j_ * 32 * kBK) = rg.sB##j_##_##n_; \
    } else if constexpr (!INBF) {                                                                         \
        *reinterpret_cast<float4*>(smem + n_ * kStageFloats + st_off + kBM * kBK + j_ * 32 * kBK) = rg.sB##j_##_##n_; \
    }
// bf16x3 keeps ONE staging set (its chunks are three times as long, so one chunk of lead hides the
// loads, and the registers are needed for the lo-plane fragments): set 0 -> LDS buffer b_
#define XV_LST3(i_, b_)                                                                                   \
    if constexpr (G > i_) {                                                                               \
        *reinterpret_cast<float4*>(smem + b_ * kStageFloats + st_off + i_ * 32 * kBK) = rg.sA##i_##_0;      \
        *reinterpret_cast<float4*>(smem + b_ * kStageFloats + st_off + kBM * kBK + i_ * 32 * kBK) = rg.sB##i_##_0; \
    }
// global loads of the chunk cx points at into staging set n_ (P_OFF: byte offset of the plane)
#define XV_GLD_X(dst_, i_, P_OFF)                                                                         \
    {                                                                                                     \
        const int row_shift = cx.tap * a.tap_rows;                                                        \
        const int soff = ((row_shift + 32 * i_) * a.ldx + cx.kc * BKE) * ES + (P_OFF);                    \
        if (GUARD) {                                                                                      \
            /* K past the layer's width (the folded taps of the next frame): an offset the descriptor's   \
               range check rejects, so the piece reads as zeros; rows past the tensor: same check */      \
            const bool ok_ = cx.kc * BKE + c * (16 / ES) < a.kpt;                                         \
            if constexpr (GUARD == 2) { /* fp32 source: 8 floats -> 8 bf16 */                             \
                const int voff = ok_ ? 2 * cx.xo##i_ : 0x7ffffff0;                                        \
                const float4 lo_ = buf_load16(cx.xrsrc, voff, 2 * soff);                                  \
                const float4 hi_ = buf_load16(cx.xrsrc, voff, 2 * soff + 16);                             \
                dst_ = cvt8_bf16(lo_, hi_);                                                               \
            } else {                                                                                      \
                const int voff = ok_ ? cx.xo##i_ : 0x7ffffff0;                                            \
                dst_ = buf_load16(cx.xrsrc, voff, soff);                                                  \
            }                                                                                             \
        } else {                                                                                          \
            dst_ = buf_load16(cx.xrsrc, cx.xo##i_, soff);                                                 \
        }                                                                                                 \
    }
#define XV_GLD_A(i_, n_) \
    if constexpr (G > i_) XV_GLD_X(rg.sA##i_##_##n_, i_, 0)
#define XV_GLD_B(j_, n_)                                                                                  \
    if constexpr (X3) {                                                                                   \
        if constexpr (G > j_) XV_GLD_X(rg.sB##j_##_##n_, j_, a.x_plane_bytes)                             \
    } else if constexpr (!INBF) {                                                                         \
        rg.sB##j_##_##n_ = buf_load16(cx.wrsrc, cx.w_toff, (32 * j_ * a.k_pad + cx.itl * BKE) * ES);         \
    }
// bf16: the weights are packed fragment-major at load time (pack.hip): for a 32-channel column
// tile and a 16-wide k-step, the 64 lanes' 16-byte MFMA B operands are one contiguous KiB.  Each
// wave reads its own B fragments straight into registers, one coalesced buffer load per k-step;
// LDS carries only the activations.  Fragment q (k-step q of a 64-wide chunk) of chunk c_ -> set s_.
#define XV_GLB(q_, s_, c_)                                                                                \
    if constexpr (INBF && !X3) {                                                                          \
        int cw_ = (c_);                                                                                   \
        if (cw_ >= n_chunks) cw_ -= n_chunks;                                                             \
        rg.gb##q_##_##s_ = buf_load16(cx.wfrsrc, cx.wf_voff, (4 * cw_ + q_) * 1024);                      \
    }
// bf16x3: per chunk the stream holds the four W_hi k-step blocks, then the four W_lo blocks; both
// fragments of k-step q_ of chunk c_ go to ONE register pair (gb<q>_0 = hi, gb<q>_1 = lo), reloaded
// as soon as the k-step's last MFMA has issued (three quarters of a chunk ahead of their use)
#define XV_GLB3(q_, c_)                                                                                   \
    if constexpr (X3) {                                                                                   \
        int cw_ = (c_);                                                                                   \
        if (cw_ >= n_chunks) cw_ -= n_chunks;                                                             \
        rg.gb##q_##_0 = buf_load16(cx.wfrsrc, cx.wf_voff, (8 * cw_ + q_) * 1024);                         \
        rg.gb##q_##_1 = buf_load16(cx.wfrsrc, cx.wf_voff, (8 * cw_ + 4 + q_) * 1024);                     \
    }
// bf16x3: lo-plane fragment of k-step q_ (second half of the LDS buffer) -> fragment set 1
#define XV_FRG_L(i_, q_, S_) \
    if constexpr (G > i_) { rg.fa##i_##_1 = *reinterpret_cast<const float4*>((S_) + kBM * kBK + a_rd + i_ * 32 * kBK + XV_KO(q_)); }
#define XV_GLD_ALL(n_) XV_GLD_A(0, n_) XV_GLD_A(1, n_) XV_GLD_A(2, n_) XV_GLD_A(3, n_) \
                       XV_GLD_B(0, n_) XV_GLD_B(1, n_) XV_GLD_B(2, n_) XV_GLD_B(3, n_)
#define XV_LST_ALL(n_) XV_LST_A(0, n_) XV_LST_A(1, n_) XV_LST_A(2, n_) XV_LST_A(3, n_) \
                       XV_LST_B(0, n_) XV_LST_B(1, n_) XV_LST_B(2, n_) XV_LST_B(3, n_)
// fp32: one MFMA (row group i_, k component c_, fragment set f_) and the statement slotted behind it
#define XV_MF(i_, c_, f_, slot_)                                                                          \
    if constexpr (G > i_) {                                                                               \
        acc##i_ = __builtin_amdgcn_mfma_f32_32x32x2f32(rg.fa##i_##_##f_.c_, rg.fb_##f_.c_, acc##i_, 0, 0, 0);   \
    }                                                                                                     \
    SB();                                                                                                 \
    slot_                                                                                                 \
    SB();
// bf16: one MFMA per row group consumes the whole 16-byte fragment (k-step of 16)
// (SWAP: weights as the first operand -- the accumulator's registers are then channels and its lanes frames,
// the layout store_acc turns into 16-byte stores)
#define XV_MFB(i_, f_, q_, P_)                                                                            \
    if constexpr (G > i_) {                                                                               \
        if constexpr (SWAP)                                                                               \
            acc##i_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, rg.gb##q_##_##P_), \
                                                              __builtin_bit_cast(bf16x8, rg.fa##i_##_##f_), acc##i_, 0, 0, 0); \
        else                                                                                              \
            acc##i_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, rg.fa##i_##_##f_), \
                                                              __builtin_bit_cast(bf16x8, rg.gb##q_##_##P_), acc##i_, 0, 0, 0); \
    }                                                                                                     \
    SB();
// one k-group with 16 slots.  fp32: 4 k components x 4 row groups = 16 MFMAs, one slot behind each;
// bf16: 4 MFMAs (k-step 16), four slots behind each
#define XV_KG(q_, P_, f_, s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15)           \
    if constexpr (INBF) {                                                                                 \
        XV_MFB(0, f_, q_, P_) s0 s1 s2 s3 SB(); XV_MFB(1, f_, q_, P_) s4 s5 s6 s7 SB();                   \
        XV_MFB(2, f_, q_, P_) s8 s9 s10 s11 SB(); XV_MFB(3, f_, q_, P_) s12 s13 s14 s15 SB();             \
    } else {                                                                                              \
        XV_MF(0, x, f_, s0) XV_MF(1, x, f_, s1) XV_MF(2, x, f_, s2) XV_MF(3, x, f_, s3)                   \
        XV_MF(0, y, f_, s4) XV_MF(1, y, f_, s5) XV_MF(2, y, f_, s6) XV_MF(3, y, f_, s7)                   \
        XV_MF(0, z, f_, s8) XV_MF(1, z, f_, s9) XV_MF(2, z, f_, s10) XV_MF(3, z, f_, s11)                 \
        XV_MF(0, w, f_, s12) XV_MF(1, w, f_, s13) XV_MF(2, w, f_, s14) XV_MF(3, w, f_, s15)               \
    }
// bf16x3: four MFMAs (row groups) of fragment set f_ against B register b_, one slot behind each
#define XV_M3(i_, f_, b_)                                                                                 \
    if constexpr (G > i_) {                                                                               \
        acc##i_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, rg.fa##i_##_##f_),   \
                                                          __builtin_bit_cast(bf16x8, rg.b_), acc##i_, 0, 0, 0); \
    }                                                                                                     \
    SB();
#define XV_G3(f_, b_, s0, s1, s2, s3) \
    XV_M3(0, f_, b_) s0 SB(); XV_M3(1, f_, b_) s1 SB(); XV_M3(2, f_, b_) s2 SB(); XV_M3(3, f_, b_) s3 SB();
#define XV_NOP ;
// One K-chunk held in LDS buffer P_; N_ = the other buffer = the staging set holding chunk it+1.
// Branch-free: the last chunk of a tile also stores/loads/reads ahead (clamped to the last
// chunk, results unused) -- n_chunks is even, so the two-chunk loop body needs no tail variants.
// (parenthesised: the template argument list must not be split by the slot macros' commas)
#define XV_ADVANCE (advance<GUARD, X3>)(a, cx, n_chunks);
#define XV_CHUNK(P_, N_, IT_)                                                                             \
    {                                                                                                     \
        const float* S = smem + P_ * kStageFloats;                                                        \
        const float* Sn = smem + N_ * kStageFloats;                                                       \
        XV_KG(0, P_, 0, XV_FRG_A(0, 1, 1, S), XV_FRG_A(1, 1, 1, S), XV_FRG_A(2, 1, 1, S),                 \
              XV_FRG_A(3, 1, 1, S), XV_FRG_B(1, 1, S),                                                    \
              XV_LST_A(0, N_), XV_LST_A(1, N_), XV_LST_A(2, N_), XV_LST_A(3, N_),                         \
              XV_LST_B(0, N_), XV_LST_B(1, N_), XV_LST_B(2, N_), XV_LST_B(3, N_),                         \
              XV_GLB(3, N_, (IT_) + 1), XV_NOP, XV_ADVANCE)                                \
        XV_KG(1, P_, 1, XV_FRG_A(0, 2, 0, S), XV_FRG_A(1, 2, 0, S), XV_FRG_A(2, 2, 0, S),                 \
              XV_FRG_A(3, 2, 0, S), XV_FRG_B(2, 0, S),                                                    \
              XV_GLD_A(0, N_), XV_GLD_A(1, N_), XV_GLD_A(2, N_), XV_GLD_A(3, N_),                         \
              XV_GLD_B(0, N_), XV_GLD_B(1, N_), XV_GLD_B(2, N_), XV_GLD_B(3, N_),                         \
              XV_GLB(0, P_, (IT_) + 2), XV_NOP, XV_NOP)                                                   \
        XV_KG(2, P_, 0, XV_FRG_A(0, 3, 1, S), XV_FRG_A(1, 3, 1, S), XV_FRG_A(2, 3, 1, S),                 \
              XV_FRG_A(3, 3, 1, S), XV_FRG_B(3, 1, S), XV_GLB(1, P_, (IT_) + 2), XV_NOP, XV_NOP, XV_NOP,  \
              XV_NOP, XV_NOP, XV_NOP, XV_NOP, XV_NOP, XV_NOP, XV_NOP)                                     \
        __syncthreads(); /* chunk it+1 complete in LDS; chunk it's buffer is free */                     \
        XV_KG(3, P_, 1, XV_FRG_A(0, 0, 0, Sn), XV_FRG_A(1, 0, 0, Sn), XV_FRG_A(2, 0, 0, Sn),              \
              XV_FRG_A(3, 0, 0, Sn), XV_FRG_B(0, 0, Sn), XV_GLB(2, P_, (IT_) + 2), XV_NOP, XV_NOP,        \
              XV_NOP, XV_NOP, XV_NOP, XV_NOP, XV_NOP, XV_NOP, XV_NOP, XV_NOP)                             \
    }

// bf16x3: one K-chunk = [hi tile | lo tile] in LDS buffer P_.  Per k-step q: x_hi*W_hi (hi frags in
// set 0, read during the previous k-step), x_hi*W_lo, x_lo*W_hi (lo frags into set 1 during the first
// group) -- 12 MFMAs per k-step, 48 per chunk and barrier; every fragment read and every weight
// fragment load feeds its MFMAs once, the staging of chunk it+1 / it+2 rides in the middle groups.
#define XV_CHUNK3(P_, N_, IT_)                                                                            \
    {                                                                                                     \
        const float* S = smem + P_ * kStageFloats;                                                        \
        const float* Sn = smem + N_ * kStageFloats;                                                       \
        XV_G3(0, gb0_0, XV_FRG_L(0, 0, S), XV_FRG_L(1, 0, S), XV_FRG_L(2, 0, S), XV_FRG_L(3, 0, S))       \
        XV_G3(0, gb0_1, XV_LST3(0, N_), XV_LST3(1, N_), XV_LST3(2, N_), XV_LST3(3, N_))                   \
        XV_G3(1, gb0_0, XV_FRG_A(0, 1, 0, S), XV_FRG_A(1, 1, 0, S), XV_FRG_A(2, 1, 0, S),                 \
              XV_FRG_A(3, 1, 0, S))                                                                       \
        XV_ADVANCE                                                                                        \
        XV_G3(0, gb1_0, XV_FRG_L(0, 1, S), XV_FRG_L(1, 1, S), XV_FRG_L(2, 1, S), XV_FRG_L(3, 1, S))       \
        XV_G3(0, gb1_1, XV_GLB3(0, (IT_) + 1), XV_GLD_A(0, 0) XV_GLD_A(1, 0),                             \
              XV_GLD_A(2, 0) XV_GLD_A(3, 0), XV_GLD_B(0, 0) XV_GLD_B(1, 0))                               \
        XV_G3(1, gb1_0, XV_FRG_A(0, 2, 0, S), XV_FRG_A(1, 2, 0, S), XV_FRG_A(2, 2, 0, S),                 \
              XV_FRG_A(3, 2, 0, S))                                                                       \
        XV_G3(0, gb2_0, XV_FRG_L(0, 2, S), XV_FRG_L(1, 2, S), XV_FRG_L(2, 2, S), XV_FRG_L(3, 2, S))       \
        XV_G3(0, gb2_1, XV_GLB3(1, (IT_) + 1), XV_GLD_B(2, 0) XV_GLD_B(3, 0), XV_NOP, XV_NOP)             \
        XV_G3(1, gb2_0, XV_FRG_A(0, 3, 0, S), XV_FRG_A(1, 3, 0, S), XV_FRG_A(2, 3, 0, S),                 \
              XV_FRG_A(3, 3, 0, S))                                                                       \
        XV_G3(0, gb3_0, XV_FRG_L(0, 3, S), XV_FRG_L(1, 3, S), XV_FRG_L(2, 3, S), XV_FRG_L(3, 3, S))       \
        XV_G3(0, gb3_1, XV_GLB3(2, (IT_) + 1), XV_NOP, XV_NOP, XV_NOP)                                    \
        __syncthreads(); /* chunk it+1 complete in LDS; chunk it's buffer is free */                     \
        XV_G3(1, gb3_0, XV_FRG_A(0, 0, 0, Sn), XV_FRG_A(1, 0, 0, Sn), XV_FRG_A(2, 0, 0, Sn),              \
              XV_FRG_A(3, 0, 0, Sn))                                                                      \
        XV_GLB3(3, (IT_) + 1)                                                                             \
    }

// Pipeline registers that live across tiles: two staging sets (_0/_1: A row groups 0..3 and W
// row blocks 0..3 of a chunk in flight) and two fragment sets.  A struct of named members, not
// arrays (see above).
struct Regs {
    float4 sA0_0, sA1_0, sA2_0, sA3_0, sB0_0, sB1_0, sB2_0, sB3_0;
    float4 sA0_1, sA1_1, sA2_1, sA3_1, sB0_1, sB1_1, sB2_1, sB3_1;
    float4 fa0_0, fa1_0, fa2_0, fa3_0, fb_0, fa0_1, fa1_1, fa2_1, fa3_1, fb_1;
    float4 gb0_0, gb1_0, gb2_0, gb3_0, gb0_1, gb1_1, gb2_1, gb3_1;   // bf16: B fragments of two chunks, from global
    float4 w3[6];        // bf16_split3: the weight fragments of one chunk, [k-step * 3 + plane], reloaded in place
};

struct Lane {
    int h, sw, a_rd, b_rd, st_off, r0, c, col;
    int st3, rd3;        // bf16_split3: byte offsets of this thread's plane-row store and of its k-step-0 fragment read
};

// ---------------------------------------------------------------------------------------------
// bf16_split3 (template flag S3 of the fp32 instantiations, 1-tap layers): the fp32 activations are split into three bf16
// planes on their way from the staging registers to LDS, x = hi + mid + lo exactly (hi = bf16(x), mid = bf16(x - hi),
// lo = x - hi - mid: both differences are exact in fp32 and lo fits in bf16), the weights were split the same way at
// load time (pack.hip, pack_tdnn_weight_split3_kernel), and every 16-wide k-step issues the six products
//   lo*W_hi + mid*W_mid + hi*W_lo + mid*W_hi + hi*W_mid + hi*W_hi
// (the three dropped ones are below 2^-26 |x||w|) on v_mfma_f32_32x32x16_bf16 into ONE accumulator: the MFMA adds its
// 16 products in two groups of 8 and rounds into the accumulator once per group (profiles/experiments/mfma_bf16_rounding.hip,
// DESIGN 3.1c).  Six 32-cycle MFMAs replace eight 64-cycle fp32 ones per 32x32x16 block: 0.375 of the matrix-pipe time.
//   * K chunks stay 32 fp32 wide (the fp32 staging path).  An LDS buffer holds the chunk's three planes, 8 KiB each: rows of
//     64 B (32 k), 16-byte pieces XOR-swizzled by (row >> 2) & 3, so the ds_write_b64 stores and the ds_read_b128 fragment
//     reads (lane (r, h) of k-step s: row r, k 16s + 8h .. +7) are bank-conflict free.
//   * the weight planes go from global memory straight into the MFMA B operand (one KiB per plane and k-step of a
//     32-channel column, hi | mid | lo), loaded one chunk ahead into the registers their last product has just left.
//   * three blocks per CU: 168 registers -- 64 accumulators, ONE staging set of 16 (a chunk of lead, as bf16x3:
//     with three waves per SIMD a chunk lasts several load latencies), six weight fragments reloaded in place, two rolling
//     sets of three activation fragments -- and kS3LdsBytes of LDS, the buffers packed at their 24 KiB.
// ---------------------------------------------------------------------------------------------
constexpr int kPlaneBytes = kBM * kBK * 2;   // one bf16 plane of a 128 x 32 chunk
// LDS of the split form: two buffers of three planes, then the constants table -- 50 688 B, three blocks per CU (the fp32 /
// bf16 instantiations keep kLdsBytes, two 32 KiB buffers)
constexpr int kS3BufBytes = 3 * kPlaneBytes;
// channels of a block's tile: 128 on four waves; 384 on twelve for the wave sets WS = 0, 1, 2 of tdnn_split3w.hip
template <int WS>
constexpr int kTileBN = WS < 0 ? kBN : 3 * kBN;
constexpr int kS3LdsBytes = 2 * kS3BufBytes + kConstFloats * 4;
// first float of the constants table (bias | scale | shift) in a block's LDS
template <bool S3>
constexpr int kCstFloat = S3 ? 2 * kS3BufBytes / 4 : 2 * kStageFloats;

// staging registers of row group i (fp32, 16 bytes) -> the three planes of LDS buffer B
__device__ __forceinline__ void s3_store(char* B, int st3, int i, const float4& v) {
    u32x2 hi, mid, lo;
    split3(v, hi, mid, lo);
    *reinterpret_cast<u32x2*>(B + st3 + i * 32 * 64) = hi;
    *reinterpret_cast<u32x2*>(B + kPlaneBytes + st3 + i * 32 * 64) = mid;
    *reinterpret_cast<u32x2*>(B + 2 * kPlaneBytes + st3 + i * 32 * 64) = lo;
}

// global loads of the chunk cx points at (row groups < NG) into one staging set
template <int NG>
__device__ __forceinline__ void s3_gld(const TdnnArgs& a, const Ctx& cx, float4& d0, float4& d1, float4& d2, float4& d3) {
    const int soff = ((cx.tap * a.tap_rows) * a.ldx + cx.kc * kBK) * 4;
    const int rs = 32 * a.ldx * 4;
    if constexpr (NG > 0) d0 = buf_load16(cx.xrsrc, cx.xo0, soff);
    if constexpr (NG > 1) d1 = buf_load16(cx.xrsrc, cx.xo1, soff + rs);
    if constexpr (NG > 2) d2 = buf_load16(cx.xrsrc, cx.xo2, soff + 2 * rs);
    if constexpr (NG > 3) d3 = buf_load16(cx.xrsrc, cx.xo3, soff + 3 * rs);
}

// the three weight fragments (hi | mid | lo) of k-step s of chunk c of this wave's column -> w[3s ..]; the stream wraps to
// chunk 0 past the tile's last chunk (the next tile of the block is in the same channel column)
__device__ __forceinline__ void s3_wld(const Ctx& cx, float4* w, int c, int s, int n_chunks) {
    if (c >= n_chunks) c -= n_chunks;
#pragma unroll
    for (int j = 0; j < 3; ++j) w[3 * s + j] = buf_load16(cx.wfrsrc, cx.wf_voff, (6 * c + 3 * s + j) * 1024);
}

// the three plane fragments of row group i, k-step s of the chunk in LDS buffer S
__device__ __forceinline__ void s3_frag(const char* S, int rd3, int i, int s, float4* xf) {
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
        xf[pl] = *reinterpret_cast<const float4*>(S + pl * kPlaneBytes + i * 32 * 64 + (rd3 ^ (32 * s)));
}

// Item N of a chunk's 2 G (k-step s = N / G, row group i = N % G): the fragments of item N + 1 go into the other of the two
// rolling sets, then the six products of item N; behind a k-step's last row group its three weight registers are free and
// take the same k-step of chunk c_next (tdnn_wino_s3.hip reloads U the same way), so ONE set of six holds the stream.
template <int G, int N>
__device__ __forceinline__ void s3_item(const Ctx& cx, const char* S, int rd3, f32x16& acc, float4 (&xf)[2][3], float4* w,
                                        int c_next, int n_chunks) {
    constexpr int s = N / G, i = N % G;
    if constexpr (N + 1 < 2 * G) s3_frag(S, rd3, (N + 1) % G, (N + 1) / G, xf[(N + 1) & 1]);
    s3_mfma6(acc, xf[N & 1], w + 3 * s);
    if constexpr (i == G - 1) s3_wld(cx, w, c_next, s, n_chunks);
}

#ifdef XVEC_KNOCK
// Timing-only knock-outs, compile time (-DXVEC_KNOCK=mask, the convention and the bit space of tdnn_pp16.hip; results are
// garbage), in the POOLING instantiation only, so that layer 4 still feeds layer 5 real data.  A knocked head does no s3_gld and
// no s3_store (no row loads, no split, no LDS stores); the products then run on what the LDS buffers hold (in these builds the
// block prologue puts the planes of chunk 0 into both).  The step of the load stream, the barrier, weight loads, fragment reads,
// MFMAs and the epilogue stay.  No address changes.
//   bit 20: EVERY block: the head knocked in two of every three chunks, counted through the block's tiles (a third of the
//           head work per MFMA in every block, with no cost of sharing it: the upper bound on a 384-channel tile,
//           profiles/split3_wide_bound.txt)
//   bit 21: EVERY block: every head knocked (what the head costs altogether)
#define XV_S3_KNOCK ((XVEC_KNOCK & ((1 << 20) | (1 << 21))) != 0)
// (POOL_: the instantiation pools; G0_: the tile's first row group; NCH_: chunks per tile; IT_: the chunk)
#define XV_S3_HEAD_LIVE(POOL_, G0_, NCH_, IT_) \
    (!(POOL_) || !XV_S3_KNOCK || ((XVEC_KNOCK & (1 << 21)) == 0 && ((IT_) + (int)(((G0_) >> 2) % 3) * (NCH_)) % 3 == 0))
#else
#define XV_S3_KNOCK 0
#define XV_S3_HEAD_LIVE(POOL_, G0_, NCH_, IT_) true
#endif

// One K-chunk: chunk `it` is in LDS buffer P, its weights in rg.w3; staging set N holds chunk it + 1, which goes to
// buffer N (free: every wave passed the previous chunk's barrier after its last fragment read), then set N is refilled
// with the chunk the stream points at next.  The order of the products into each accumulator is the chunk's k-steps in
// turn, whatever the order of the row groups around them.
// WS >= 0 (the 384-channel tile on twelve waves, tdnn_split3w.hip): only the wave set whose parity the chunk has (WS == P) does
// this head, and its load stream steps TWO chunks, so its one staging set holds chunk it + 1 when the head of chunk it starts
// and chunk it + 3 behind it; set 2 has no head in any chunk.  Everything behind the head is the same code for every wave.
#define XV_S3_ITEM(i_, s_, IT_)                                                                           \
    if constexpr (G > i_) { s3_item<G, s_ * G + i_>(cx, S, ln.rd3, acc##i_, xf, rg.w3, (IT_) + 1, n_chunks); SB(); }
#define XV_S3_CHUNK(P_, N_, IT_)                                                                          \
    {                                                                                                     \
        const char* S = reinterpret_cast<const char*>(smem) + P_ * kS3BufBytes;                           \
        char* Sn = reinterpret_cast<char*>(smem) + N_ * kS3BufBytes;                                      \
        float4 xf[2][3];                                                                                  \
        s3_frag(S, ln.rd3, 0, 0, xf[0]);                                                                  \
        if constexpr (WS < 0 || WS == P_) {  /* the wave sets of the 384-channel tile: head in the chunks of their parity */ \
            const bool head_ = XV_S3_HEAD_LIVE(POOL, g0, n_chunks, IT_); /* true but in knock-out builds */                                              \
            if (head_) {                                                                                  \
                if constexpr (G > 0) s3_store(Sn, ln.st3, 0, rg.sA0_0);                                   \
                if constexpr (G > 1) s3_store(Sn, ln.st3, 1, rg.sA1_0);                                   \
                if constexpr (G > 2) s3_store(Sn, ln.st3, 2, rg.sA2_0);                                   \
                if constexpr (G > 3) s3_store(Sn, ln.st3, 3, rg.sA3_0);                                   \
            }                                                                                             \
            advance<GUARD, false>(a, cx, n_chunks);                                                       \
            if constexpr (WS >= 0) advance<GUARD, false>(a, cx, n_chunks);                                \
            if (head_) s3_gld<G>(a, cx, rg.sA0_0, rg.sA1_0, rg.sA2_0, rg.sA3_0);                          \
        }                                                                                                 \
        XV_S3_ITEM(0, 0, IT_) XV_S3_ITEM(1, 0, IT_) XV_S3_ITEM(2, 0, IT_) XV_S3_ITEM(3, 0, IT_)           \
        XV_S3_ITEM(0, 1, IT_) XV_S3_ITEM(1, 1, IT_) XV_S3_ITEM(2, 1, IT_) XV_S3_ITEM(3, 1, IT_)           \
        __syncthreads(); /* chunk it+1 complete in LDS; chunk it's buffer is free */                     \
    }

// Once per block: chunk 0 of the first tile -> LDS buffer 0, its first fragments -> set 0,
// chunks 1 and 2 in flight in the two staging sets (bf16x3: chunk 1 in its single set).
template <int GUARD, bool INBF, bool X3, bool S3, int WS = -1>
__device__ __forceinline__ void block_prologue(const TdnnArgs& a, float* smem, Ctx& cx, Regs& rg, const Lane& ln,
                                               int n_chunks) {
    constexpr int G = 4;   // fetch all four row groups: rows past a short first tile are allocated
    constexpr int ES = INBF ? 2 : 4, BKE = 128 / ES;
    const int h = ln.h, sw = ln.sw, a_rd = ln.a_rd, b_rd = ln.b_rd, st_off = ln.st_off, c = ln.c;
    if constexpr (S3 && WS >= 0) {
        // the 384-channel tile (tdnn_split3w.hip).  Wave set 1 (head in the odd chunks) stages the even chunks: chunk 0 -> LDS
        // buffer 0, chunk 2 in flight; set 0 stages the odd ones: chunk 1 in flight; set 2 never stages.  Weights of chunk 0.
        if constexpr (WS == 1) {
            s3_gld<4>(a, cx, rg.sA0_0, rg.sA1_0, rg.sA2_0, rg.sA3_0);
            s3_wld(cx, rg.w3, 0, 0, n_chunks);
            s3_wld(cx, rg.w3, 0, 1, n_chunks);
            s3_store(reinterpret_cast<char*>(smem), ln.st3, 0, rg.sA0_0);
            s3_store(reinterpret_cast<char*>(smem), ln.st3, 1, rg.sA1_0);
            s3_store(reinterpret_cast<char*>(smem), ln.st3, 2, rg.sA2_0);
            s3_store(reinterpret_cast<char*>(smem), ln.st3, 3, rg.sA3_0);
            advance<GUARD, false>(a, cx, n_chunks);
            advance<GUARD, false>(a, cx, n_chunks);
            s3_gld<4>(a, cx, rg.sA0_0, rg.sA1_0, rg.sA2_0, rg.sA3_0);
        } else {
            if constexpr (WS == 0) {
                advance<GUARD, false>(a, cx, n_chunks);
                s3_gld<4>(a, cx, rg.sA0_0, rg.sA1_0, rg.sA2_0, rg.sA3_0);
            }
            s3_wld(cx, rg.w3, 0, 0, n_chunks);
            s3_wld(cx, rg.w3, 0, 1, n_chunks);
        }
        __syncthreads();
        return;
    }
    if constexpr (S3) {      // chunk 0 -> LDS buffer 0 (split), chunk 1 in flight in the one staging set, weights of chunk 0
        char* B0 = reinterpret_cast<char*>(smem);
        s3_gld<4>(a, cx, rg.sA0_0, rg.sA1_0, rg.sA2_0, rg.sA3_0);
        s3_wld(cx, rg.w3, 0, 0, n_chunks);
        s3_wld(cx, rg.w3, 0, 1, n_chunks);
        s3_store(B0, ln.st3, 0, rg.sA0_0);
        s3_store(B0, ln.st3, 1, rg.sA1_0);
        s3_store(B0, ln.st3, 2, rg.sA2_0);
        s3_store(B0, ln.st3, 3, rg.sA3_0);
        if constexpr (XV_S3_KNOCK) {      // knock-out builds: real planes in buffer 1 too (the first head overwrites them if it runs)
            s3_store(B0 + kS3BufBytes, ln.st3, 0, rg.sA0_0);
            s3_store(B0 + kS3BufBytes, ln.st3, 1, rg.sA1_0);
            s3_store(B0 + kS3BufBytes, ln.st3, 2, rg.sA2_0);
            s3_store(B0 + kS3BufBytes, ln.st3, 3, rg.sA3_0);
        }
        advance<GUARD, false>(a, cx, n_chunks);
        s3_gld<4>(a, cx, rg.sA0_0, rg.sA1_0, rg.sA2_0, rg.sA3_0);
        __syncthreads();
        return;
    }
    if constexpr (X3) {      // one staging set: chunk 0 -> LDS buffer 0, chunk 1 in flight in the set
        XV_GLD_ALL(0)
        SB();
        XV_LST3(0, 0) XV_LST3(1, 0) XV_LST3(2, 0) XV_LST3(3, 0)
        SB();
        advance<GUARD, X3>(a, cx, n_chunks);
        XV_GLD_ALL(0)
    } else {
        XV_GLD_ALL(0)
        advance<GUARD, X3>(a, cx, n_chunks);
        XV_GLD_ALL(1)
        SB();
        XV_LST_ALL(0)
        SB();
        advance<GUARD, X3>(a, cx, n_chunks);
        XV_GLD_ALL(0)
    }
    __syncthreads();
    XV_FRG_A(0, 0, 0, smem) XV_FRG_A(1, 0, 0, smem) XV_FRG_A(2, 0, 0, smem) XV_FRG_A(3, 0, 0, smem)
    XV_FRG_B(0, 0, smem)
    XV_GLB(0, 0, 0) XV_GLB(1, 0, 0) XV_GLB(2, 0, 0) XV_GLB(3, 0, 0)
    XV_GLB(0, 1, 1) XV_GLB(1, 1, 1) XV_GLB(2, 1, 1) XV_GLB(3, 1, 1)
    XV_GLB3(0, 0) XV_GLB3(1, 0) XV_GLB3(2, 0) XV_GLB3(3, 0)
    SB();
}

// One tile of G row groups (32 frames each) x 128 channels, starting at row group g0.  On entry
// the pipeline is primed for this tile (block_prologue or the previous tile's last chunks).
template <int G, int GUARD, bool POOL, bool STORE, bool INBF, bool OUTBF, bool X3, bool S3, int WS = -1>
__device__ __forceinline__ void process_tile(const TdnnArgs& a, float* smem, Ctx& cx, Regs& rg, const Lane& ln,
                                             int64_t g0, int n0, int n_chunks) {
    constexpr int ES = INBF ? 2 : 4, BKE = 128 / ES;
    constexpr int BN = kTileBN<WS>;      // channels of the block's tile = stride of the constants table
    const int h = ln.h, sw = ln.sw, a_rd = ln.a_rd, b_rd = ln.b_rd, st_off = ln.st_off, c = ln.c;
    // bf16 in, bf16 out, one plane, stored: the transposed product (channels in the accumulator's registers), so
    // that a lane ends up with 8 consecutive channels of one frame = one 16-byte store.  With frames in the
    // registers a lane holds ONE channel and every value is its own 2-byte store: 64 store instructions per
    // wave and tile -- layer 1, whose K loop is two chunks long, spent most of its 30 us issuing them.
    constexpr bool SWAP = INBF && OUTBF && !X3 && STORE && !POOL;
    f32x16 acc0, acc1, acc2, acc3;
    // this wave's 32 channels, the lane half's 4 of every 8 (SWAP): bias | scale | shift tables in LDS
    const float* cstw = smem + kCstFloat<S3> + (ln.col - n0 - (int)(threadIdx.x & 31)) + 4 * ln.h;
    if constexpr (SWAP) {      // accumulators start at the bias of their register's channel
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const float4 b4 = *reinterpret_cast<const float4*>(cstw + 8 * gq);
            acc0[4 * gq] = b4.x; acc0[4 * gq + 1] = b4.y; acc0[4 * gq + 2] = b4.z; acc0[4 * gq + 3] = b4.w;
        }
        acc1 = acc0; acc2 = acc0; acc3 = acc0;
    } else if constexpr (POOL) {
        // accumulators start at bias - K, K = the block's pooling pivot of this lane's channel (at 0 in the block's
        // first tile, whose epilogue picks K and adds bias - K: a large bias must not sit in the accumulator while
        // the K loop adds small terms to it -- every MFMA would round at ulp(bias)): tdnn_common.h, pool_group_impl
        const float b0 = smem[kCstFloat<S3> + BN + (ln.col - n0)];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc0[e] = b0;
        acc1 = acc0; acc2 = acc0; acc3 = acc0;
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; acc2[e] = 0.f; acc3[e] = 0.f; }
    }

#ifdef XVEC_DIAG
    SB();
    const unsigned long long dt0 = __builtin_amdgcn_s_memtime();
    SB();
#endif
    // ---- K chunks, two per trip (LDS buffer 0 then 1); n_chunks is even
    for (int it = 0; it < n_chunks; it += 2) {
        if constexpr (S3) {
            XV_S3_CHUNK(0, 1, it)
            XV_S3_CHUNK(1, 0, it + 1)
        } else if constexpr (X3) {
            XV_CHUNK3(0, 1, it)
            XV_CHUNK3(1, 0, it + 1)
        } else {
            XV_CHUNK(0, 1, it)
            XV_CHUNK(1, 0, it + 1)
        }
    }
#ifdef XVEC_DIAG
    SB();
    const unsigned long long dt1 = __builtin_amdgcn_s_memtime();
    SB();
#endif

    const int64_t m0 = g0 * 32;
    // ---- epilogue: bias + ReLU + folded BatchNorm (tdnn_layer.py:30-39)
    // accumulator element e of lane (r, h): row = (e&3) + 8*(e>>2) + 4*h, col = r
    const int col = ln.col;
    // epilogue constants of this lane's channel: three LDS reads per tile instead of three registers held
    // across the K loop (the pooling and first-layer variants were 3-6 registers over the 256 budget)
    float* cst = smem + kCstFloat<S3> + (col - n0);
    const float bi = cst[0], sc = cst[BN], sh = cst[2 * BN];
    // pooling variants: the three slots are bias | bias - K | -K (this wave's own channels: no barrier)
    float negk = sh;
    if constexpr (POOL) {
        if (!cx.pivot_set) {       // block-uniform: the block's first tile, whose accumulators started at 0
            // r of the block's first frame, cut to its upper 8 significant bits, and -K itself in the table.  A channel that is
            // off in an utterance of a block whose first frame (another utterance's) has it on contributes n equal terms -K: with
            // 8 bits their sums and the sums of their squares are exact in fp32 over a 32-row partial, so pool_finalize gets a
            // second moment of exactly 0 wherever the block boundaries fall (with 24 bits: ~3e-4 K of std or 0, by the last
            // bits of K -- and where the boundaries fall changes with the blocks per CU and from form to form).  Every form of
            // this body cuts alike, so the forms agree on such channels; tdnn_pp16.hip's pivots are bf16 too.
            const float piv = __uint_as_float(__float_as_uint(lower_half(fmaxf(acc0[0] + bi, 0.f))) & 0xffff0000u);
            const float bmk = bi - piv;
            negk = -piv;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                acc0[e] += bmk;
                if constexpr (G > 1) acc1[e] += bmk;
                if constexpr (G > 2) acc2[e] += bmk;
                if constexpr (G > 3) acc3[e] += bmk;
            }
            cst[BN] = bmk;
            cst[2 * BN] = negk;
            cx.pivot_set = true;
        }
    }
    // Two phases per row group: (1) all 16 values finished IN PLACE in the accumulator registers,
    // (2) 16 stores issued back to back from those 16 distinct registers, addressed by a per-tile
    // buffer descriptor + one per-lane offset + a scalar row offset.  (Computing each value into a
    // shared temporary right before its store made every store wait for the previous one to have
    // read that register, and chained 64-bit address adds: ~23k cycles per tile in layer 2.)
    const int esz = OUTBF ? 2 : 4;
    __amdgpu_buffer_rsrc_t yrsrc;
    int y_voff = 0;
    __amdgpu_buffer_rsrc_t yrsrc_lo;     // bf16x3: descriptor of the lo plane (same offsets as the hi plane)
    if (STORE) {
        yrsrc = make_rsrc(static_cast<char*>(a.Y) + (m0 * (int64_t)a.ldy + n0) * esz);
        if constexpr (X3 && OUTBF)
            yrsrc_lo = make_rsrc(static_cast<char*>(a.Y) + a.y_plane_bytes + (m0 * (int64_t)a.ldy + n0) * esz);
        y_voff = (4 * h * a.ldy + (col - n0)) * esz;
    }
#define XV_EPI(i_)                                                                                        \
    if constexpr (G > i_) {                                                                               \
        /* pooling variant: the accumulator holds z + bias - K; ReLU and sums in pool_group, BatchNorm in  \
           pool_finalize */                                                                               \
        if constexpr (!POOL) {                                                                            \
            _Pragma("unroll") for (int e = 0; e < 16; ++e)                                                \
                acc##i_[e] = fmaf(fmaxf(acc##i_[e] + bi, 0.f), sc, sh);                                   \
            asm volatile("" : "+v"(acc##i_));                                                             \
        }                                                                                                 \
        if (STORE) {                                                                                      \
            _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                              \
                const int soff = (i_ * 32 + (e & 3) + 8 * (e >> 2)) * a.ldy * esz;                        \
                if constexpr (OUTBF) {                                                                    \
                    const __bf16 hv = (__bf16)acc##i_[e];                                                 \
                    __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, hv), yrsrc,  \
                                                          y_voff, soff, 0);                               \
                    if constexpr (X3) { /* bf16x3: the remainder goes to the lo plane */                  \
                        const __bf16 lv = (__bf16)(acc##i_[e] - (float)hv);                               \
                        __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, lv),     \
                                                              yrsrc_lo, y_voff, soff, 0);                 \
                    }                                                                                     \
                } else {                                                                                  \
                    const float fv = acc##i_[e]; /* scalar copy: bit_cast of a vector ELEMENT is miscompiled */ \
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(fv), yrsrc, y_voff, soff, 0);   \
                }                                                                                         \
            }                                                                                             \
        }                                                                                                 \
        if (POOL) pool_group(a, acc##i_, negk, m0 + i_ * 32, h, col, cx.pool);                            \
    }
    if constexpr (SWAP) {
        float4 sc4[4], sh4[4];
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            sc4[gq] = *reinterpret_cast<const float4*>(cstw + kBN + 8 * gq);
            sh4[gq] = *reinterpret_cast<const float4*>(cstw + 2 * kBN + 8 * gq);
        }
        // lane = frame r of the group, 8 channels per store: (r, h) -> channels 8h.. (+16 for the second store)
        const int voff = ((int)(threadIdx.x & 31) * a.ldy + (ln.col - n0 - (int)(threadIdx.x & 31)) + 8 * h) * 2;
        if constexpr (G > 0) store_acc(acc0, sc4, sh4, yrsrc, voff, 0 * 32 * a.ldy * 2);
        if constexpr (G > 1) store_acc(acc1, sc4, sh4, yrsrc, voff, 1 * 32 * a.ldy * 2);
        if constexpr (G > 2) store_acc(acc2, sc4, sh4, yrsrc, voff, 2 * 32 * a.ldy * 2);
        if constexpr (G > 3) store_acc(acc3, sc4, sh4, yrsrc, voff, 3 * 32 * a.ldy * 2);
    } else {
        XV_EPI(0) XV_EPI(1) XV_EPI(2) XV_EPI(3)
    }
#undef XV_EPI
#ifdef XVEC_DIAG
    SB();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const unsigned long long dt2 = __builtin_amdgcn_s_memtime();
    SB();
    if (threadIdx.x == 0 && blockIdx.x < 8192) {
        unsigned long long* d = g_diag + blockIdx.x * 8;
        d[3] += dt1 - dt0;     // K loop
        d[4] += dt2 - dt1;     // epilogue (issue side; stores still in flight)
        d[5] += 1;             // tiles
    }
#endif
}

template <int GUARD, bool POOL, bool STORE, bool INBF, bool OUTBF, bool X3, bool S3, int WS = -1>
__device__ __forceinline__ void tdnn_body(const TdnnArgs& a, float* smem) {
    constexpr int BN = kTileBN<WS>;
#ifdef XVEC_DIAG
    const unsigned long long t_entry = __builtin_amdgcn_s_memtime(), r_entry = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0 && blockIdx.x < 8192) { g_diag[blockIdx.x * 8 + 3] = 0; g_diag[blockIdx.x * 8 + 4] = 0; g_diag[blockIdx.x * 8 + 5] = 0; }
#endif
    // logical id -> (row range p, channel column j); the n_tiles columns of one range are
    // consecutive ids on one XCD
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int j = lid % a.n_tiles;
    const int p = lid / a.n_tiles;
    int64_t g_begin, g_end;
    group_range(a, p, g_begin, g_end);
    const int n0 = j * BN;
    const int n_chunks = a.n_taps * a.cpt;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    Lane ln;
    ln.h = lane >> 5;
    const int r = lane & 31;
    // staging map: thread -> (row r0 + 32*j, 16-byte chunk c) of a 32-wide K chunk
    ln.c = tid & 7;
    ln.r0 = WS < 0 ? tid >> 3 : (tid & 255) >> 3;      // twelve waves: the 256-thread map within each wave set
    ln.st_off = ln.r0 * kBK + ((ln.c ^ ((ln.r0 >> 1) & 7)) << 2);
    // fragment read map: row (base + r), logical 16-B chunk 2q+h, swizzled by row
    ln.sw = (r >> 1) & 7;
    ln.a_rd = r * kBK;
    ln.b_rd = kBM * kBK + (wave * 32 + r) * kBK;
    ln.col = n0 + wave * 32 + r;
    // bf16_split3 planes: 64-byte rows, 16-byte piece q of row r stored at piece q ^ ((r >> 2) & 3)
    ln.st3 = ln.r0 * 64 + ((((ln.c >> 1) ^ ((ln.r0 >> 2) & 3)) * 16) | ((ln.c & 1) * 8));
    ln.rd3 = r * 64 + ((ln.h ^ ((r >> 2) & 3)) * 16);
    if (tid < BN) {
        smem[kCstFloat<S3> + tid] = a.bias[n0 + tid];
        smem[kCstFloat<S3> + BN + tid] = POOL ? 0.f : a.scale[n0 + tid];
        smem[kCstFloat<S3> + 2 * BN + tid] = POOL ? 0.f : a.shift[n0 + tid];
    }

    Ctx cx;
    cx.g_s = g_begin;
    cx.g_end = g_end;
    cx.m0 = g_begin * 32;
    constexpr int ES = INBF ? 2 : 4;
    cx.es = ES;
    cx.xrsrc = x_rsrc<GUARD>(a, cx);
    cx.wrsrc = make_rsrc(static_cast<const char*>(a.W) + (int64_t)n0 * a.k_pad * ES);
    cx.x_base = ln.r0 * a.ldx * ES + ln.c * 16;
    cx.w_toff = ln.r0 * a.k_pad * ES + ln.c * 16;
    cx.r0 = ln.r0;
    if (INBF) {   // 1 KiB per (column tile of 32 channels, k-step of 16)
        const int64_t ct = n0 / 32 + wave;
        cx.wfrsrc = make_rsrc(static_cast<const char*>(a.Wf) + ct * (int64_t)(a.k_pad / 16) * 1024);
        cx.wf_voff = lane * 16;
    }
    if (S3) {     // 3 KiB (hi | mid | lo) per (column tile of 32 channels, k-step of 16)
        const int64_t ct = n0 / 32 + wave;
        cx.wfrsrc = make_rsrc(static_cast<const char*>(a.Wf) + ct * (int64_t)(a.k_pad / 16) * 3072);
        cx.wf_voff = lane * 16;
    }
    cx.u_tile = __builtin_amdgcn_readfirstlane(utt_of_row(a.out_map, cx.m0));
    cx.off_next = row_off(a.out_map, cx.u_tile + 1);
    if (POOL) {
        cx.pool.u = cx.u_tile;
        cx.pool.end = cx.off_next;
    }
    cx.pivot_set = false;
    set_tile_rows(a, cx);
    cx.tap = 0;
    cx.kc = 0;
    cx.itl = 0;

    Regs rg;
    block_prologue<GUARD, INBF, X3, S3, WS>(a, smem, cx, rg, ln, n_chunks);
    int64_t g = g_begin;
    for (; g + 4 <= g_end; g += 4) process_tile<4, GUARD, POOL, STORE, INBF, OUTBF, X3, S3, WS>(a, smem, cx, rg, ln, g, n0, n_chunks);
    const int rem = (int)(g_end - g);
    if (rem == 3) process_tile<3, GUARD, POOL, STORE, INBF, OUTBF, X3, S3, WS>(a, smem, cx, rg, ln, g, n0, n_chunks);
    else if (rem == 2) process_tile<2, GUARD, POOL, STORE, INBF, OUTBF, X3, S3, WS>(a, smem, cx, rg, ln, g, n0, n_chunks);
    else if (rem == 1) process_tile<1, GUARD, POOL, STORE, INBF, OUTBF, X3, S3, WS>(a, smem, cx, rg, ln, g, n0, n_chunks);
#ifdef XVEC_DIAG
    if (threadIdx.x == 0 && blockIdx.x < 8192) {
        __builtin_amdgcn_s_waitcnt(0);
        unsigned long long* d = g_diag + blockIdx.x * 8;
        d[0] = t_entry;
        d[1] = __builtin_amdgcn_s_memtime();
        d[2] = (unsigned long long)(g_end - g_begin);
        d[6] = r_entry;                              // 100 MHz reference clock at entry / exit: core clock of the launch
        d[7] = __builtin_amdgcn_s_memrealtime();
    }
#endif
}

template <typename K>
static hipError_t launch_kernel(K kern, const TdnnArgs& a, hipStream_t s, LdsOptIn& opt, int lds_bytes = kLdsBytes) {
    if (a.groups_total <= 0 || a.blocks_per_col <= 0 || a.blocks_per_col > a.groups_total || (a.cpt & 1))
        return hipErrorInvalidValue;
    if (hipError_t e = opt.ensure(reinterpret_cast<const void*>(kern), lds_bytes); e != hipSuccess) return e;
    const int grid = a.blocks_per_col * a.n_tiles;
    kern<<<dim3(grid), dim3(256), lds_bytes, s>>>(a);
    return hipGetLastError();
}

}  // namespace xvec
