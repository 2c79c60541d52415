// fp32 frame-level layer with three equally spaced taps [-d, 0, +d] (layers 2 and 3 of the reference, main.py:39-40) as
// Winograd minimal filtering F(2,3) along time: two outputs of the 3-tap correlation from FOUR products instead of six.
//
// For a tile of two outputs (t, t + d) of one utterance, with x_m = X[t + m*d] (m = 0..3, the layer's input rows) and W_0,
// W_1, W_2 the tap weights:
//   V0 = x0 - x2     V1 = x1 + x2     V2 = x2 - x1     V3 = x1 - x3
//   U0 = W0          U1 = (W0+W1+W2)/2     U2 = (W0-W1+W2)/2     U3 = W2           (pack.hip: fp64, rounded once)
//   M_k = V_k . U_k^T                     (K = C_in each)
//   y(t) = M0 + M1 + M2       y(t+d) = M1 - M2 - M3
// then today's epilogue (bias, ReLU, folded BatchNorm) on both outputs.  Per output frame that is 2 x C_in products
// instead of 3 x C_in: 0.667x of the direct form's MFMA work at C_in = 512.
//
// Pair space.  The outputs i = 0..T_out-1 of an utterance form the tiles (i, i+d) for i mod 2d < d, numbered j = 0..P-1
// (i = j + d*(j div d)), P = d*(T_out div 2d) + min(T_out mod 2d, d); a tile whose i + d >= T_out has one output.  Tiles
// are aligned to each utterance's own frame 0, so an utterance's rows do not depend on where it sits in the batch.  The
// GEMM M axis is the flat pair index q over the batch: utterance u owns pairs [pb(u), pb(u) + P_u) with
//   pb(u) = u * P                                   (fixed length)
//   pb(u) = (row_off(u) >> 1) + u * d               (ragged: no prefix sum needed; pb(u+1) - pb(u) >= P_u, the few
//                                                    pairs in between are holes that read a valid row and store nothing)
//
// Machine mapping: the scheme of tdnn_layer.hip's fp32 kernel (persistent balanced ranges of 32-pair groups, 2 blocks per
// CU of 4 wave64, XCD-aware block ids, v_mfma_f32_32x32x2_f32, 32-wide K chunks through two LDS buffers, one barrier per
// chunk, every memory instruction slotted behind one MFMA).  A tile is 64 pairs (128 output frames) x 128 channels; wave
// w owns channels [32w, 32w+32) and holds 4 products x 2 pair groups = 8 accumulators (128 registers).  The K chunks are
// walked (chunk kc of product 0, 1, 2, 3, then kc+1): a chunk stages V_k of its 64 pairs (two input rows per pair,
// combined in registers on the way to LDS) and the 128 rows of U_k (packed in that order, pack.hip), 24 KiB.  The input
// rows of consecutive chunks are the same 128-byte slab of the same rows: L2 hits.
#include "tdnn_wino_rows.h"

namespace xvec {
namespace wino {

constexpr int kBMP = kPairs;                        // pairs of a tile
constexpr int kStage = (kBMP + kBN) * kBK;          // one LDS buffer (floats): V tile then U tile
constexpr int kLdsBytes = (2 * kStage + kConst + 2 * kTbl) * 4 + 2 * 8;   // + per parity the tile's output base row

// Step the load stream to the next chunk (products innermost); after a tile's last chunk, to chunk 0 of the block's next
// tile.  Past the block's last chunk it stays put (the look-ahead re-reads that chunk; the data is never used).
__device__ __forceinline__ void advance(const TdnnArgs& a, Ctx& cx, const Lane& ln, int* tbl, int64_t* tblh, int n_chunks) {
    if (cx.itl + 1 < n_chunks) {
        ++cx.itl;
        if (++cx.kk == 4) {
            cx.kk = 0;
            ++cx.kc;
        }
    } else {
        const int64_t g_rem = cx.g_end - cx.g_s;
        const int64_t g_next = cx.g_s + (g_rem < 2 ? g_rem : 2);
        if (g_next < cx.g_end) {
            cx.g_s = g_next;
            cx.q0 = g_next * 32;
            cx.lp ^= 1;
            set_rows(a, cx, ln, tbl, tblh);
            cx.itl = 0;
            cx.kc = 0;
            cx.kk = 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Main loop over NAMED registers (see tdnn_layer.hip: register arrays were left in scratch by hipcc once scheduling
// barriers were present).  G (pair groups of the tile, 1..2) is a template parameter; ops of an absent group vanish.
// Staging set n: xa<i>_n, xb<i>_n = the two input rows of V_k for pair group i, u<j>_n = rows 32j.. of U_k.
// ---------------------------------------------------------------------------------------------
#define WG_KO(q_) ((((2 * (q_)) + h) ^ sw) << 2)
#define WG_FRG_A(i_, q_, f_, S_) \
    if constexpr (G > i_) { rg.fa##i_##_##f_ = *reinterpret_cast<const float4*>((S_) + a_rd + i_ * 32 * kBK + WG_KO(q_)); }
#define WG_FRG_B(q_, f_, S_) \
    { rg.fb_##f_ = *reinterpret_cast<const float4*>((S_) + b_rd + WG_KO(q_)); }
// V_k of the staging set -> LDS buffer n_ (KS_: the product the set holds): x0-x2 | x1+x2 | x2-x1 | x1-x3
#define WG_LST_A(i_, n_, KS_)                                                                                  \
    if constexpr (GL > i_) {                                                                                   \
        float4 v_;                                                                                             \
        if constexpr (KS_ == 1) {                                                                              \
            v_.x = rg.xa##i_.x + rg.xb##i_.x; v_.y = rg.xa##i_.y + rg.xb##i_.y;    \
            v_.z = rg.xa##i_.z + rg.xb##i_.z; v_.w = rg.xa##i_.w + rg.xb##i_.w;    \
        } else {                                                                                               \
            v_.x = rg.xa##i_.x - rg.xb##i_.x; v_.y = rg.xa##i_.y - rg.xb##i_.y;    \
            v_.z = rg.xa##i_.z - rg.xb##i_.z; v_.w = rg.xa##i_.w - rg.xb##i_.w;    \
        }                                                                                                      \
        *reinterpret_cast<float4*>(smem + n_ * kStage + st_off + i_ * 32 * kBK) = v_;                          \
    }
#define WG_LST_B(j_, n_) *reinterpret_cast<float4*>(smem + n_ * kStage + st_off + kBMP * kBK + j_ * 32 * kBK) = rg.u##j_;
// the two input rows of V_k (KL_: the product of the chunk cx points at) for pair group i_ -> the staging set.  Rows x1,
// x2 are x0 + d, x0 + 2d: the scalar offset carries the shift; x3 has a lane offset of its own (x1 in one-output tiles).
#define WG_GLD_X(dst_, i_, M_)                                                                                 \
    if constexpr (M_ == 3) dst_ = buf_load16(cx.xrsrc, cx.x3##i_, cx.kc * 128);                                      \
    else dst_ = buf_load16(cx.xrsrc, cx.x0##i_, cx.kc * 128 + M_ * cx.drb);
#define WG_GLD_A(i_, KL_)                                                                                      \
    if constexpr (GL > i_) {                                                                                   \
        WG_GLD_X(rg.xa##i_, i_, (KL_ == 0 ? 0 : KL_ == 1 ? 1 : KL_ == 2 ? 2 : 1))                              \
        WG_GLD_X(rg.xb##i_, i_, (KL_ == 0 ? 2 : KL_ == 1 ? 2 : KL_ == 2 ? 1 : 3))                              \
    }
#define WG_GLD_B(j_) rg.u##j_ = buf_load16(cx.wrsrc, cx.w_toff, (32 * j_ * a.k_pad + cx.itl * kBK) * 4);
// one MFMA (product K_, pair group i_, k component c_, fragment set f_) and the statement slotted behind it
#define WG_MF(K_, i_, c_, f_, slot_)                                                                           \
    if constexpr (G > i_) {                                                                                    \
        acc##K_##_##i_ = __builtin_amdgcn_mfma_f32_32x32x2f32(rg.fa##i_##_##f_.c_, rg.fb_##f_.c_, acc##K_##_##i_, 0, 0, 0); \
    }                                                                                                          \
    SB();                                                                                                      \
    slot_                                                                                                      \
    SB();
// one k-group of 8 k: 4 components x 2 pair groups, one slot behind each MFMA
#define WG_KG(K_, f_, s0, s1, s2, s3, s4, s5, s6, s7)                                                         \
    WG_MF(K_, 0, x, f_, s0) WG_MF(K_, 1, x, f_, s1) WG_MF(K_, 0, y, f_, s2) WG_MF(K_, 1, y, f_, s3)            \
    WG_MF(K_, 0, z, f_, s4) WG_MF(K_, 1, z, f_, s5) WG_MF(K_, 0, w, f_, s6) WG_MF(K_, 1, w, f_, s7)
#define WG_NOP ;
#define WG_ADVANCE advance(a, cx, ln, tbl, tblh, n_chunks);
// One chunk (product K_) held in LDS buffer P_.  The single staging set holds chunk it+1 (product KS_): it goes to LDS
// buffer N_ first, then receives chunk it+2 (product KL_) -- one chunk of lead, as the bf16x3 path of tdnn_layer.hip
// (two sets do not fit next to the eight accumulators).  Branch-free: the last chunks of a block also store / load ahead.
#define WG_CHUNK(P_, N_, K_, KS_, KL_)                                                                         \
    {                                                                                                          \
        const float* S = smem + P_ * kStage;                                                                   \
        const float* Sn = smem + N_ * kStage;                                                                  \
        WG_KG(K_, 0, WG_FRG_A(0, 1, 1, S), WG_FRG_A(1, 1, 1, S), WG_FRG_B(1, 1, S), WG_LST_A(0, N_, KS_),      \
              WG_LST_A(1, N_, KS_), WG_LST_B(0, N_), WG_LST_B(1, N_), WG_LST_B(2, N_))                         \
        WG_KG(K_, 1, WG_FRG_A(0, 2, 0, S), WG_FRG_A(1, 2, 0, S), WG_FRG_B(2, 0, S), WG_LST_B(3, N_),           \
              WG_ADVANCE, WG_GLD_A(0, KL_), WG_GLD_A(1, KL_), WG_GLD_B(0))                                     \
        WG_KG(K_, 0, WG_FRG_A(0, 3, 1, S), WG_FRG_A(1, 3, 1, S), WG_FRG_B(3, 1, S), WG_GLD_B(1),               \
              WG_GLD_B(2), WG_GLD_B(3), WG_NOP, WG_NOP)                                                        \
        __syncthreads(); /* chunk it+1 complete in LDS; chunk it's buffer is free */                          \
        WG_KG(K_, 1, WG_FRG_A(0, 0, 0, Sn), WG_FRG_A(1, 0, 0, Sn), WG_FRG_B(0, 0, Sn), WG_NOP, WG_NOP, WG_NOP, \
              WG_NOP, WG_NOP)                                                                                  \
    }

struct Regs {
    float4 xa0, xb0, xa1, xb1, u0, u1, u2, u3;
    float4 fa0_0, fa1_0, fb_0, fa0_1, fa1_1, fb_1;
};

// Once per block: chunk 0 of the first tile -> LDS buffer 0, its first fragments -> set 0, chunk 1 in flight.
__device__ __forceinline__ void block_prologue(const TdnnArgs& a, float* smem, int* tbl, int64_t* tblh, Ctx& cx, Regs& rg,
                                               const Lane& ln, int n_chunks) {
    constexpr int G = 2, GL = 2;
    const int h = ln.h, sw = ln.sw, a_rd = ln.a_rd, b_rd = ln.b_rd, st_off = ln.st_off;
    WG_GLD_A(0, 0) WG_GLD_A(1, 0) WG_GLD_B(0) WG_GLD_B(1) WG_GLD_B(2) WG_GLD_B(3)
    SB();
    WG_LST_A(0, 0, 0) WG_LST_A(1, 0, 0) WG_LST_B(0, 0) WG_LST_B(1, 0) WG_LST_B(2, 0) WG_LST_B(3, 0)
    SB();
    advance(a, cx, ln, tbl, tblh, n_chunks);
    WG_GLD_A(0, 1) WG_GLD_A(1, 1) WG_GLD_B(0) WG_GLD_B(1) WG_GLD_B(2) WG_GLD_B(3)
    __syncthreads();
    WG_FRG_A(0, 0, 0, smem) WG_FRG_A(1, 0, 0, smem) WG_FRG_B(0, 0, smem)
    SB();
}

// One tile of G pair groups (32 pairs each) x 128 channels at pair group g0; tp = its row-table parity.  On entry the
// pipeline is primed for this tile (block_prologue or the previous tile's last chunks).
template <int G>
__device__ __forceinline__ void process_tile(const TdnnArgs& a, float* smem, int* tbl, int64_t* tblh, Ctx& cx, Regs& rg,
                                             const Lane& ln, int n0, int tp, int n_chunks) {
    constexpr int GL = 2;     // the load stream always fetches both groups (rows of a short tile's absent group are valid)
    const int h = ln.h, sw = ln.sw, a_rd = ln.a_rd, b_rd = ln.b_rd, st_off = ln.st_off;
    f32x16 acc0_0, acc0_1, acc1_0, acc1_1, acc2_0, acc2_1, acc3_0, acc3_1;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        acc0_0[e] = 0.f; acc1_0[e] = 0.f; acc2_0[e] = 0.f; acc3_0[e] = 0.f;
        acc0_1[e] = 0.f; acc1_1[e] = 0.f; acc2_1[e] = 0.f; acc3_1[e] = 0.f;
    }
    // ---- K chunks, four per trip (products 0..3; LDS buffers 0, 1, 0, 1); n_chunks is a multiple of 4
    for (int it = 0; it < n_chunks; it += 4) {
        WG_CHUNK(0, 1, 0, 1, 2)
        WG_CHUNK(1, 0, 1, 2, 3)
        WG_CHUNK(0, 1, 2, 3, 0)
        WG_CHUNK(1, 0, 3, 0, 1)
    }

    epilogue<G>(a, smem + 2 * kStage, tbl, tblh, ln, n0, tp, acc0_0, acc1_0, acc2_0, acc3_0, acc0_1, acc1_1, acc2_1, acc3_1);
}

__global__ __launch_bounds__(256, 2) void tdnn_wino_kernel(const TdnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int* tbl = reinterpret_cast<int*>(smem + 2 * kStage + kConst);
    int64_t* tblh = reinterpret_cast<int64_t*>(smem + 2 * kStage + kConst + 2 * kTbl);
    Ctx cx;
    Lane ln;
    const int n0 = block_setup(a, 7, cx, ln);
    const int n_chunks = 4 * a.cpt;
    const int64_t g_begin = cx.g_s, g_end = cx.g_end;     // (the load stream moves cx.g_s on)
    const int wave = ln.wave, r = ln.r;
    ln.st_off = ln.r0 * kBK + ((ln.c ^ ((ln.r0 >> 1) & 7)) << 2);
    ln.sw = (r >> 1) & 7;
    ln.a_rd = r * kBK;
    ln.b_rd = kBMP * kBK + (wave * 32 + r) * kBK;
    cx.wrsrc = make_rsrc(static_cast<const float*>(a.W) + (int64_t)n0 * a.k_pad);
    cx.w_toff = ln.r0 * a.k_pad * 4 + ln.c * 16;

    stream_start(a, n0, smem + 2 * kStage, tbl, tblh, cx, ln);

    Regs rg;
    block_prologue(a, smem, tbl, tblh, cx, rg, ln, n_chunks);
    int64_t g = g_begin;
    int tp = 0;
    for (; g + 2 <= g_end; g += 2, tp ^= 1) process_tile<2>(a, smem, tbl, tblh, cx, rg, ln, n0, tp, n_chunks);
    if (g < g_end) process_tile<1>(a, smem, tbl, tblh, cx, rg, ln, n0, tp, n_chunks);
}

}  // namespace wino

bool tdnn_wino_applicable(const TdnnGeom& g, int ldx) {
    return g.n_taps == 3 && g.tap_rows >= 1 && g.kpt == g.cin && g.kpt_pad % (2 * kBK) == 0 && g.kpt_pad <= ldx &&
           g.n_pad % wino::kBN == 0 && ldx % 4 == 0;
}

hipError_t launch_tdnn_wino(const TdnnArgs& a, hipStream_t s) {
    if (a.groups_total <= 0 || a.blocks_per_col <= 0 || a.blocks_per_col > a.groups_total || a.tap_rows < 1 || a.cpt < 1 ||
        (a.out_map.offsets == nullptr && a.p_fixed < 1))
        return hipErrorInvalidValue;
    const int grid = a.blocks_per_col * a.n_tiles;
    wino::tdnn_wino_kernel<<<dim3(grid), dim3(256), wino::kLdsBytes, s>>>(a);
    return hipGetLastError();
}

}  // namespace xvec
