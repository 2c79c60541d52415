// The bf16_split3 pooling kernel of fp32 layer 5 (tdnn_split3.hip: the form; tdnn_layer_impl.h: the body and a wave's K loop) on
// a tile of 128 rows x 384 channels: twelve waves of 32 channels, one block per CU -- three waves per SIMD as at three 4-wave
// blocks per CU, and the same 168-register budget.  Per wave it is tdnn_split3_kernel<true, false> unchanged: its
// 128 x 32 sub-tile, one accumulator per row group, the weight stream one chunk ahead in one set of six registers, two rolling
// fragment sets, s3_mfma6 in the same item order, the pooling epilogue with the 8-bit pivot, partial slots by row group +
// utterance.  With blocks_per_col = CUs / 4 the row ranges are those of the three-block grid of 128-channel columns, so the
// pivots, partials and pooled statistics are the same bits.
// What changes is who stages.  The three planes of a chunk serve 384 channels instead of 128, and three wave sets (waves 0-3 |
// 4-7 | 8-11, one wave of each on every SIMD) share the head with tdnn_split3.hip's 256-thread staging map:
//   set 0  head in the even chunks: stages the odd chunks (it + 1), its load stream steps two chunks at a time
//   set 1  head in the odd chunks:  stages the even chunks
//   set 2  never stages
// so per MFMA a third of the row loads, splits, LDS stores and L2 -> CU activation bytes, and in every chunk two of a SIMD's
// three waves have no head and feed the matrix pipe while the third one stages.  One barrier per chunk as before; the rows of a
// chunk have two chunks to arrive.  LDS: two buffers of three 8 KiB planes, then the constants of 384 channels (53 760 B; the
// three 4-wave blocks of a CU hold 152 064 B).
// The schedule is the one tdnn_wino_s3w.hip measured for layers 2-3; the alternative of a three-buffer ring in which each set
// stages every third chunk into a buffer of its own was NOT built or measured here.
// Layer 4 (N = 512) and hidden widths whose layer-5 padding is no multiple of 384 keep the four-wave kernel (plan_layer).
#include "tdnn_layer_impl.h"

namespace xvec {

constexpr int kS3wBN = kTileBN<0>;                                       // channels of a tile: twelve waves of 32
constexpr int kS3wThreads = 2 * kS3wBN;
constexpr int kS3wLdsBytes = 2 * kS3BufBytes + 3 * kS3wBN * 4;           // the LDS image of tdnn_body<.., WS >= 0>
static_assert(kS3wLdsBytes == 53760 && kS3wThreads == 768 && kCstFloat<true> * 4 + 3 * kS3wBN * 4 == kS3wLdsBytes,
              "two buffers of three 8 KiB planes, then bias | bias - K | -K of 384 channels: what the launch opts into");

// Each wave set is a code path of its own from the first instruction on (as branches of one body hipcc keeps every set's
// values live and spills: tdnn_wino_s3w.hip)
__global__ __launch_bounds__(kS3wThreads, 1) void tdnn_split3w_kernel(const TdnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int set = __builtin_amdgcn_readfirstlane(threadIdx.x) >> 8;     // wave-uniform
    if (set == 0) tdnn_body<false, true, false, false, false, false, true, 0>(a, smem);
    else if (set == 1) tdnn_body<false, true, false, false, false, false, true, 1>(a, smem);
    else tdnn_body<false, true, false, false, false, false, true, 2>(a, smem);
}

static LdsOptIn opt_wide;     // per device

hipError_t tdnn_split3w_max_blocks_per_cu(int* blocks) {
    const void* kern = reinterpret_cast<const void*>(tdnn_split3w_kernel);
    if (hipError_t e = opt_wide.ensure(kern, kS3wLdsBytes); e != hipSuccess) return e;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, kern, kS3wThreads, kS3wLdsBytes);
}

// The pooling layer takes this tile from this many output rows per CU on (B >= 86 at T = 300), and the four-wave kernel below
// it.  The tile measured faster at every batch size down to B = 32 (36 rows per CU: DESIGN 3.1c,
// profiles/split3_wide_crossover.txt); the threshold keeps the batches below it on the kernel they were validated with
// (tests/test_fuzz_fp32_forms_gpu.py pins layer 5 to 256 threads below 83 rows per CU).
constexpr int kSplit3WideMinRowsPerCu = 96;

void tdnn_split3w_knobs(bool* enabled, int* min_rows_per_cu) {
    const char* on = getenv("XVEC_SPLIT3_WIDE");
    const char* rows = getenv("XVEC_SPLIT3_WIDE_MIN_ROWS");
    *enabled = !on || atoi(on) != 0;
    const int r = rows ? atoi(rows) : kSplit3WideMinRowsPerCu;
    *min_rows_per_cu = r >= 0 ? r : kSplit3WideMinRowsPerCu;
}

bool tdnn_split3w_applicable(const TdnnGeom& g) { return g.n_taps == 1 && g.n_pad % kS3wBN == 0; }

hipError_t launch_tdnn_split3w(const TdnnArgs& a, hipStream_t s) {
    if (a.n_taps != 1 || a.groups_total <= 0 || a.blocks_per_col <= 0 || a.blocks_per_col > a.groups_total || (a.cpt & 1) ||
        a.Wf == nullptr || a.pool_part == nullptr)
        return hipErrorInvalidValue;
    if (hipError_t e = opt_wide.ensure(reinterpret_cast<const void*>(tdnn_split3w_kernel), kS3wLdsBytes); e != hipSuccess) return e;
    const int grid = a.blocks_per_col * a.n_tiles;
    tdnn_split3w_kernel<<<dim3(grid), dim3(kS3wThreads), kS3wLdsBytes, s>>>(a);
    return hipGetLastError();
}

}  // namespace xvec
