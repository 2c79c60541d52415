// The Winograd F(2,3) kernel on bf16_split3 operands (tdnn_wino_s3.hip: the form, the schedule of a wave's K loop) on a tile
// of 64 pairs x 256 channels: eight waves of 32 channels, one block per CU.  Per wave it is tdnn_wino_s3.hip
// unchanged -- 2 pair groups x 4 products = 8 accumulators, six bf16 MFMAs per product and group in the same order, U
// fragments straight from TdnnArgs::Wf one chunk ahead, the same LDS image, the same epilogue -- so every output is the same
// bits.  What changes is who stages: the V planes of a chunk serve 256 channels instead of 128, and the two wave sets
// (waves 0-3 | 4-7, one wave of each on every SIMD) stage ALTERNATE chunks with tdnn_wino_s3.hip's 256-thread staging map:
//   set 0 (waves 0-3)  head in the odd chunks:  stages the even chunks (it + 1), its load stream steps two chunks at a time
//   set 1 (waves 4-7)  head in the even chunks: stages the odd chunks
// A wave does a whole head every other chunk -- half the input-row loads, V formation, splits and LDS stores per MFMA -- and in
// every chunk one of a SIMD's two waves has no head at all and feeds the matrix pipe while the other one stages; the one
// barrier per chunk (inside product 3, as there) orders the buffers as before.  The x rows of a chunk have two chunks to arrive.
//   per block and chunk: 16 KiB of input rows + 96 KiB of U planes over 8 waves x 4 products x 2 groups x 6 = 384 MFMAs
//   = 299 B per MFMA (tdnn_wino_s3.hip: 341).
// Row tables: both sets walk the tiles and fill the tables of the tile their stream enters (the same values); set 0 enters a
// tile one chunk earlier than tdnn_wino_s3.hip's stream does, which needs n_chunks >= 4 between the epilogue that last read a
// table parity and the head that rewrites it (launch_tdnn_wino_s3w checks it).
#include "tdnn_wino_rows.h"
#include "wino_s3_lds_map.h"
#include "wino_s3_tile.h"

namespace xvec {
namespace wino {

constexpr int kS3wBN = 256;                               // channels of a tile: eight waves of 32
constexpr int kS3wLdsBytes = 2 * kS3Stage + 3 * kS3wBN * 4 + 2 * kTbl * 4 + 2 * 8;   // tdnn_wino_s3.hip's, constants of 256 channels

// One tile of G pair groups x 256 channels, for the waves whose head is in the chunks of parity HP (s3_tile of
// tdnn_wino_s3.hip: entry state and schedule; the staging registers hold the tile's first chunk of parity 1 - HP that is not
// in LDS yet).
template <int G, int HP>
__device__ __forceinline__ void s3w_tile(const TdnnArgs& a, char* lds, int* tbl, int64_t* tblh, Ctx& cx, const Lane& ln,
                                         int a_rd1, S3Stage& st, S3U& u, S3Frag& f, __amdgpu_buffer_rsrc_t ursrc, int n0,
                                         int tp, int n_chunks) {
    const bool grp = (threadIdx.x >> 2) & 1;
    f32x16 acc0_0, acc0_1, acc1_0, acc1_1, acc2_0, acc2_1, acc3_0, acc3_1;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        acc0_0[e] = 0.f; acc1_0[e] = 0.f; acc2_0[e] = 0.f; acc3_0[e] = 0.f;
        acc0_1[e] = 0.f; acc1_1[e] = 0.f; acc2_1[e] = 0.f; acc3_1[e] = 0.f;
    }
    // ---- K chunks, two per trip (n_chunks is even): chunk it in buffer it & 1
    for (int it = 0; it < n_chunks; ++it) {
        WS3_CHUNK(HP == 0, 2)
        ++it;
        WS3_CHUNK(HP == 1, 2)
    }
    epilogue<G, kS3wBN>(a, reinterpret_cast<const float*>(lds + 2 * kS3Stage), tbl, tblh, ln, n0, tp, acc0_0, acc1_0, acc2_0, acc3_0,
                        acc0_1, acc1_1, acc2_1, acc3_1);
}

// A block's whole run for one wave set: a code path of its own from the first instruction on (as two branches of one body
// hipcc keeps both sets' values live and spills).
template <int HP>
__device__ __forceinline__ void s3w_block(const TdnnArgs& a, char* lds) {
    float* cst = reinterpret_cast<float*>(lds + 2 * kS3Stage);
    int* tbl = reinterpret_cast<int*>(cst + 3 * kS3wBN);
    int64_t* tblh = reinterpret_cast<int64_t*>(tbl + 2 * kTbl);
    Ctx cx;
    Lane ln;
    const int n0 = block_setup<kS3wBN>(a, 3, cx, ln);
    const int n_chunks = 2 * a.cpt;        // 16-wide chunks per product (cpt counts 32-wide ones)
    const int64_t g_begin = cx.g_s, g_end = cx.g_end;     // (the load stream moves cx.g_s on)
    const int tid = threadIdx.x, lane = tid & 63, wave = ln.wave;
    // staging map of tdnn_wino_s3.hip within the wave set: thread (tid & 255)
    ln.r0 = (tid & 255) >> 3;
    ln.st_off = s3_st_off(tid & 255);
    ln.a_rd = s3_a_rd(lane, 0);
    const int a_rd1 = s3_a_rd(lane, 1);
    ln.sw = 0;
    ln.b_rd = lane * 16;                      // U fragment: 16 bytes per lane of a 1 KiB block
    // U planes of this wave's 32-channel column: 12 KiB per chunk ((chunk, product, plane) blocks of 1 KiB)
    const int64_t ct = n0 / 32 + wave;
    const __amdgpu_buffer_rsrc_t ursrc = make_rsrc(static_cast<const char*>(a.Wf) + ct * (int64_t)n_chunks * 12288);

    stream_start<kS3wBN>(a, n0, cst, tbl, tblh, cx, ln);

    // prologue.  HP 1 (stages the even chunks): chunk 0 -> LDS buffer 0, chunk 2 in the staging registers.  HP 0: chunk 1 in the
    // staging registers.  Then as tdnn_wino_s3.hip: the U planes of chunk 0, the barrier, the A fragments of product 0.
    const bool grp = (tid >> 2) & 1;
    S3Stage st;
    S3U u;
    S3Frag f;
    if constexpr (HP == 1) {
        s3_gld(cx, grp, st);
        s3_vstore(lds, ln.st_off, st);
        s3_advance<2>(a, cx, ln, tbl, tblh, n_chunks);
    } else {
        cx.kc = 1;
    }
    s3_gld(cx, grp, st);
    SB();
    {
        const int it = -1;
        WS3_ULD(0) WS3_ULD(1) WS3_ULD(2) WS3_ULD(3)
    }
    SB();
    __syncthreads();
    WS3_RD(f.a2, lds, 0, 2, 0) WS3_RD(f.a1, lds, 0, 1, 0) WS3_RD(f.a0, lds, 0, 0, 0)

    int64_t g = g_begin;
    int tp = 0;
    for (; g + 2 <= g_end; g += 2, tp ^= 1) s3w_tile<2, HP>(a, lds, tbl, tblh, cx, ln, a_rd1, st, u, f, ursrc, n0, tp, n_chunks);
    if (g < g_end) s3w_tile<1, HP>(a, lds, tbl, tblh, cx, ln, a_rd1, st, u, f, ursrc, n0, tp, n_chunks);
}

__global__ __launch_bounds__(512, 1) void tdnn_wino_s3w_kernel(const TdnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    if (__builtin_amdgcn_readfirstlane(threadIdx.x) < 256) s3w_block<1>(a, lds);      // wave-uniform: waves 0-3
    else s3w_block<0>(a, lds);
}
#undef WS3_CHUNK
#undef WS3_PRODUCT2
#undef WS3_PRODUCT1
#undef WS3_ULD
#undef WS3_RD
#undef WS3_MF

}  // namespace wino

hipError_t tdnn_wino_s3w_max_blocks_per_cu(int* blocks) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, reinterpret_cast<const void*>(wino::tdnn_wino_s3w_kernel), 512,
                                                        wino::kS3wLdsBytes);
}

bool tdnn_wino_s3w_applicable(const TdnnGeom& g, int ldx) {
    return tdnn_wino_s3_applicable(g, ldx) && g.n_pad % wino::kS3wBN == 0 && g.kpt_pad / wino::kS3K >= 4;
}

hipError_t launch_tdnn_wino_s3w(const TdnnArgs& a, hipStream_t s) {
    if (a.groups_total <= 0 || a.blocks_per_col <= 0 || a.blocks_per_col > a.groups_total || a.tap_rows < 1 || a.cpt < 2 ||
        a.Wf == nullptr || (a.out_map.offsets == nullptr && a.p_fixed < 1))
        return hipErrorInvalidValue;
    const int grid = a.blocks_per_col * a.n_tiles;
    wino::tdnn_wino_s3w_kernel<<<dim3(grid), dim3(512), wino::kS3wLdsBytes, s>>>(a);
    return hipGetLastError();
}

}  // namespace xvec
