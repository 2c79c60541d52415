// Frame-level TDNN layer for gfx950 (MI355X): exact fp32 (v_mfma_f32_32x32x2_f32) or bf16 inputs with
// fp32 accumulation (v_mfma_f32_32x32x16_bf16):
//   Y[p, n] = relu( sum_{tap, c} X[p + tap*dil, c] * W[n, tap, c] + bias[n] ) * scale[n] + shift[n]
// i.e. tdnn_layer.py:26-41 of the reference (context concat -> Linear -> ReLU -> eval
// BatchNorm1d) as ONE implicit-GEMM kernel over the flat frame axis.  No context copy
// (the reference's torch.cat, tdnn_layer.py:29) is ever materialised: a K-chunk that
// belongs to tap j is staged from rows p + j*dil of the same activation buffer.
//
// Machine mapping (CDNA4)
//   * persistent grid: 2 blocks per CU (64 KiB LDS each).  The output is cut into columns of
//     128 channels; the frames of one column are split, at 32-row granularity, into equal
//     contiguous ranges, one per block, so the last wave of work is ~1 % of the launch
//     instead of a partial round of fixed 128x128 tiles.  A block walks its range in tiles of
//     up to 4 row groups (128 frames); the blocks that cover the same frames for the different
//     channel columns get consecutive ids on one XCD, so the activation rows are shared in
//     that XCD's L2.
//   * 256 threads = 4 wave64; wave w owns channels [32w, 32w+32) of the tile for all its
//     frames: G accumulators of v_mfma_f32_32x32x2_f32 (<= 64 VGPRs).
//   * K is consumed in 32-wide chunks: global -> registers -> LDS (two LDS buffers, two
//     register sets, so a chunk's global loads are issued ~1.5 chunks before they are
//     stored), one block barrier per chunk.  LDS rows are 128 B with a 16-B-chunk XOR
//     swizzle: the ds_read_b128 fragment reads are bank-conflict free.
//   * the chunks of a tile are walked with the taps innermost (chunk kc of tap 0, 1, 2, then kc+1;
//     pack.hip stores the weights' K axis in that order): the dilated taps re-read a 128-byte slab
//     of activation rows while it is still in L2.  bf16: the weights are packed fragment-major and
//     go from global memory straight into the MFMA B operand, only activations pass through LDS.
//   * bf16x3 (template flag X3 of the bf16 instantiations): X and Y are two bf16 planes (hi, lo) of
//     fp32 values; an LDS buffer holds the hi and the lo tile of a chunk, the weight stream its W_hi and
//     W_lo fragments, and every k-step issues x_hi*W_hi + x_hi*W_lo + x_lo*W_hi (XV_CHUNK3; fp32-level
//     results: 1.5e-6 from the fp64 oracle).
//   * each ds_read_b128 feeds four MFMAs: lane half h owns k = 8q+4h..8q+4h+3 of every
//     8-wide k group, for A and B alike, so the products pair up (the k order inside a chunk
//     is permuted, which fp32 addition tolerates to rounding).
//   * every memory instruction of a chunk is slotted behind one MFMA (64 pipe cycles each):
//     in-kernel stamps showed bursts of 8 ds_write_b128 / 8 global loads idling the matrix
//     pipe for ~450 cycles each; spread out they are free.
//
// Epilogue: bias + ReLU + folded BatchNorm in registers; optional fused statistics pooling
// (main.py:59-63): per 32-row group and per utterance overlapping it, a pivot K (the group's frame 0)
// and the sums of (r - K), (r - K)^2 over the valid frames, r = relu(z + bias), go to a small partials
// buffer that pool_finalize merges in fp64 (tdnn_common.h, pool_group_impl), so the [frames,1500]
// activation of layer 5 never goes to HBM.
#include "tdnn_layer_impl.h"

namespace xvec {

template <int GUARD, bool POOL, bool STORE, bool INBF, bool OUTBF, bool X3>
__global__ __launch_bounds__(256, 2) void tdnn_kernel(const TdnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    tdnn_body<GUARD, POOL, STORE, INBF, OUTBF, X3, false>(a, smem);
}

template <int GUARD, bool POOL, bool STORE, bool INBF, bool OUTBF, bool X3 = false>
static hipError_t launch_variant(const TdnnArgs& a, hipStream_t s) {
    static LdsOptIn opt;            // per variant and device
    return launch_kernel(tdnn_kernel<GUARD, POOL, STORE, INBF, OUTBF, X3>, a, s, opt);
}

#ifdef XVEC_DIAG
extern "C" int xvec_diag_read(unsigned long long* host, int n_words) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_diag), (size_t)n_words * 8);
}
#endif

// a bf16 variant in its bf16x3 and plain instantiations
template <int GUARD, bool POOL, bool OUTBF>
static hipError_t launch_bf16(const TdnnArgs& a, bool x3, hipStream_t s) {
    return x3 ? launch_variant<GUARD, POOL, !POOL, true, OUTBF, true>(a, s) : launch_variant<GUARD, POOL, !POOL, true, OUTBF>(a, s);
}

hipError_t launch_tdnn(const TdnnArgs& a, TdnnMode m, hipStream_t s) {
    const bool pool = m.dst == Dst::kPool, out16 = m.dst == Dst::kAct, x3 = m.prec == Prec::kBf16x3;
    if (m.prec == Prec::kF32) {       // (an fp32 activation is fp32 output; layer 1 has no pooling epilogue)
        if (m.src == Src::kRows16 || (pool && m.src != Src::kAct)) return hipErrorInvalidValue;
        if (m.src == Src::kRows32) return launch_variant<true, false, true, false, false>(a, s);
        return !pool ? launch_variant<false, false, true, false, false>(a, s) : launch_variant<false, true, false, false, false>(a, s);
    }
    if (m.src == Src::kRows32)        // bf16x3 reads the caller's fp32 rows only through tdnn_first3
        return x3 || !out16 ? hipErrorInvalidValue : launch_variant<2, false, true, true, true>(a, s);
    const bool guard = m.src == Src::kRows16;
    if (out16) return guard ? launch_bf16<true, false, true>(a, x3, s) : launch_bf16<false, false, true>(a, x3, s);
    if (pool) return guard ? hipErrorInvalidValue : launch_bf16<false, true, false>(a, x3, s);
    return !guard ? launch_bf16<false, false, false>(a, x3, s) : launch_bf16<true, false, false>(a, x3, s);
}

}  // namespace xvec
