// fp32 frame-level layer with three equally spaced taps (layers 2 and 3) as Winograd F(2,3) along time (tdnn_wino.hip: the
// math and the pair space) on bf16_split3 operands (tdnn_layer_impl.h: the form; tdnn_common.h: split3, s3_mfma6): the four
// products M_k = V_k . U_k^T run on v_mfma_f32_32x32x16_bf16 with both operands split exactly into hi + mid + lo bf16 pieces,
// six products per 16-wide k-step into one accumulator.  Matrix-pipe work: 0.667 (Winograd) x 0.375 (split3) =
// 0.25 of the direct fp32 form.
//
// Tiling.  A tile is 64 pairs x 128 channels, four waves of 32 channels, 2 pair groups x 4 products = 8
// accumulators per wave, as tdnn_wino.hip.  The K loop walks 16-wide chunks, each holding ALL FOUR products: a thread
// loads the four input rows x0..x3 of its pair (16 bytes each), forms V0..V3 in fp32 (x0-x2 | x1+x2 | x2-x1 | x1-x3) and
// writes their hi / mid / lo pieces to LDS -- each input row is read once per chunk instead of twice per product.  An LDS
// buffer is [product][plane][64 pairs][16 k] bf16 = 24 KiB, every (product, plane) block in the bank-conflict-free image of
// wino_s3_lds_map.h; two buffers, one barrier per chunk.  The U planes go from global memory straight into the MFMA B operands
// (fragment-major, pack.hip: 12 KiB per wave and chunk, requested product by product a whole chunk ahead, right behind the
// MFMAs that last read their registers); the A fragments are read from LDS half a product ahead (s3_tile: the schedule).
//   per block and chunk: 16 KiB of input rows + 48 KiB of U planes over 4 waves x 4 products x 2 groups x 6 = 192 MFMAs
//   = 341 B per MFMA (the direct port of tdnn_wino.hip's tile: 427).
#include "tdnn_wino_rows.h"
#include "wino_s3_lds_map.h"
#include "wino_s3_tile.h"

namespace xvec {
namespace wino {

static_assert(kS3Pairs == kPairs, "wino_s3_lds_map.h: kS3K, kS3Plane, kS3Stage and the image of a (product, plane) block");
constexpr int kS3Const = kConst * 4;                      // bias | scale | shift of the tile's channels, bytes
constexpr int kS3LdsBytes = 2 * kS3Stage + kS3Const + 2 * kTbl * 4 + 2 * 8;   // + row tables, per parity the base row

#ifdef XVEC_KNOCK
// Timing-only knock-outs, compile time (-DXVEC_KNOCK=mask, the convention and the bit space of tdnn_pp16.hip; results are
// garbage).  A knocked head does no input-row loads, no V formation, no split and no LDS stores; the products then run on what
// the LDS buffers hold (the block prologue fills both with real V planes).  Everything else stays: the step of the load stream
// (its row tables address the epilogue's stores), barriers, U loads, fragment reads, MFMAs, epilogue.  No address changes.
//   bit 17: the blocks of ODD column tiles: every head knocked (half the head work per MFMA of the launch, but only in half
//           the blocks: the launch ends with the unchanged ones)
//   bit 18: EVERY block: the head of every odd chunk knocked (half the head work per MFMA in every block, with no cost of
//           sharing it: the upper bound on a 256-channel tile, profiles/wino_s3_wide_bound.txt)
//   bit 19: EVERY block: every head knocked (what the head costs altogether)
#define WS3_KNOCK_HEAD ((XVEC_KNOCK & (131072 | 262144 | 524288)) != 0)
#define WS3_KNOCK_MODE ((XVEC_KNOCK & 524288) ? 3 : (XVEC_KNOCK & 262144) ? 2 : 1)
#else
#define WS3_KNOCK_HEAD 0
#endif

// One tile of G pair groups x 128 channels; tp = its row-table parity.  On entry chunk 0 of the tile is in LDS buffer 0, its
// U planes are in u (or on their way), pair group 0's A fragments of its product 0 in f.a*, and the staging registers hold
// chunk 1 (block prologue or the previous tile's last chunks).
//
// Schedule of chunk `it` (buffer S = it & 1, Sn the other one), per wave; every step is pinned in this order:
//   head       V of chunk it+1 (staging registers) -> Sn; the load stream steps on; the four x rows of chunk it+2 are requested
//   product k  (k = 0..3) 6 G MFMAs, the A fragments of each half read half a product ahead (WS3_PRODUCT2; G = 1: a whole
//              product, WS3_PRODUCT1); then the three U fragments of product k of chunk it+1 are requested, straight into the
//              registers product k has just finished with
//   barrier    inside product 3, between its two pair groups (G = 1: in front of it): every wave has then READ all of S (the
//              wait in front of the barrier covers its last fragments) and WRITTEN all of Sn (head).  Behind it, under the
//              second half of product 3, pair group 0's fragments of product 0 of chunk it+1 are read from Sn; the next head
//              overwrites S.
// Vector-memory queue of a wave, oldest first, when the head of chunk it starts (buffer loads return in order):
//   x(it+1) x 4 | U(it, 0) x 3 | U(it, 1) x 3 | U(it, 2) x 3 | U(it, 3) x 3
//   head:       the V stores need x(it+1): 12 younger entries may stay            -> vmcnt(12); then x(it+2) x 4 is appended
//   product 0:  needs U(it, 0): younger are U(it, 1..3) = 9 and x(it+2) = 4       -> vmcnt(13); then U(it+1, 0) x 3
//   product k:  needs U(it, k): younger are U(it, k+1..3), x(it+2), U(it+1, 0..k-1) = 3 (3-k) + 4 + 3 k = 13  -> vmcnt(13)
// (13 for the fragment a product takes last; its first two MFMAs take the two requested before it: vmcnt(15), vmcnt(14))
// so a U fragment has a whole chunk (48 MFMAs) to arrive and the queue is never drained.  The counts are hipcc's own (it sees
// every load here); the block prologue requests in the same order, so the first chunk meets the same queue.  A tile's first
// head may find the previous epilogue's stores behind the loads: its wait then covers a few entries more, never fewer.
// KN: the knock-out build's tiles (WS3_KNOCK_HEAD; 1: no head, 2: no head in odd chunks); the shipped build has KN = 0 only.
template <int G, int KN = 0>
__device__ __forceinline__ void s3_tile(const TdnnArgs& a, char* lds, int* tbl, int64_t* tblh, Ctx& cx, const Lane& ln,
                                        int a_rd1, S3Stage& st, S3U& u, S3Frag& f, __amdgpu_buffer_rsrc_t ursrc, int n0,
                                        int tp, int n_chunks) {
    const bool grp = (threadIdx.x >> 2) & 1;
    f32x16 acc0_0, acc0_1, acc1_0, acc1_1, acc2_0, acc2_1, acc3_0, acc3_1;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        acc0_0[e] = 0.f; acc1_0[e] = 0.f; acc2_0[e] = 0.f; acc3_0[e] = 0.f;
        acc0_1[e] = 0.f; acc1_1[e] = 0.f; acc2_1[e] = 0.f; acc3_1[e] = 0.f;
    }
    // ---- K chunks: chunk it in buffer it & 1 (n_chunks is even, so every tile starts in buffer 0)
    for (int it = 0; it < n_chunks; ++it) {
        WS3_CHUNK(KN != 1, 1)
        if constexpr (KN == 2) {       // n_chunks is even
            ++it;
            WS3_CHUNK(false, 1)
        }
    }
    epilogue<G>(a, reinterpret_cast<const float*>(lds + 2 * kS3Stage), tbl, tblh, ln, n0, tp, acc0_0, acc1_0, acc2_0, acc3_0, acc0_1,
                acc1_1, acc2_1, acc3_1);
    // With two chunks per tile the load stream reaches the tile after the next one at the head of the next tile's chunk 0:
    // set_rows then rewrites the row-table parity this epilogue has just read, with no barrier of the K loop in between (from
    // four chunks on there is one).  A wave that is still in this epilogue must not see those rows.
    if (n_chunks == 2) __syncthreads();
}

#if WS3_KNOCK_HEAD
// Knock-out build only: a block's whole run as a function, KN = without head work -- a code path of its own from the first
// instruction on, so that the two forms share no registers (as two branches of one body hipcc spilled 197 of them).
template <int KN>
__device__ __forceinline__ void s3_block(const TdnnArgs& a, char* lds) {
#else
__global__ __launch_bounds__(256, 2) void tdnn_wino_s3_kernel(const TdnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int KN = 0;
#endif
    float* cst = reinterpret_cast<float*>(lds + 2 * kS3Stage);
    int* tbl = reinterpret_cast<int*>(cst + kConst);
    int64_t* tblh = reinterpret_cast<int64_t*>(tbl + 2 * kTbl);
    // staging map: thread (r0 = tid >> 3, c = tid & 7) -> pair r0 + 32 * (c >> 2) of the tile, k 4 (c & 3) .. +3 of the
    // chunk; set_rows takes the 16-byte column c & 3 and returns the input rows of both of r0's pairs
    Ctx cx;
    Lane ln;
    const int n0 = block_setup(a, 3, cx, ln);
    const int n_chunks = 2 * a.cpt;        // 16-wide chunks per product (cpt counts 32-wide ones)
    const int64_t g_begin = cx.g_s, g_end = cx.g_end;     // (the load stream moves cx.g_s on)
    const int tid = threadIdx.x, lane = tid & 63, wave = ln.wave;
    // byte offsets in a (product, plane) block (wino_s3_lds_map.h: the conflict-free image): of this thread's 8 staged bytes,
    // and of the A fragment of lane (r, h) -- pair r of the group, k 8h .. 8h + 7 -- in pair groups 0 (a_rd) and 1 (a_rd1)
    ln.st_off = s3_st_off(tid);
    ln.a_rd = s3_a_rd(lane, 0);
    const int a_rd1 = s3_a_rd(lane, 1);
    ln.sw = 0;
    ln.b_rd = lane * 16;                      // U fragment: 16 bytes per lane of a 1 KiB block
    // U planes of this wave's 32-channel column: 12 KiB per chunk ((chunk, product, plane) blocks of 1 KiB)
    const int64_t ct = n0 / 32 + wave;
    const __amdgpu_buffer_rsrc_t ursrc = make_rsrc(static_cast<const char*>(a.Wf) + ct * (int64_t)n_chunks * 12288);

    stream_start(a, n0, cst, tbl, tblh, cx, ln);

    // prologue: chunk 0 -> LDS buffer 0, chunk 1 in the staging registers, the U planes of chunk 0 requested behind it (the
    // K loop's request order: s3_tile), the A fragments of product 0 read behind the barrier
    const bool grp = (tid >> 2) & 1;
    S3Stage st;
    S3U u;
    S3Frag f;
    s3_gld(cx, grp, st);
    s3_vstore(lds, ln.st_off, st);
    s3_advance(a, cx, ln, tbl, tblh, n_chunks);
    s3_gld(cx, grp, st);
    SB();
    {
        const int it = -1;
        WS3_ULD(0) WS3_ULD(1) WS3_ULD(2) WS3_ULD(3)
    }
    SB();
    if constexpr (KN) s3_vstore(lds + kS3Stage, ln.st_off, st);      // chunk 1 -> buffer 1: the K loop will not write it
    __syncthreads();
    WS3_RD(f.a2, lds, 0, 2, 0) WS3_RD(f.a1, lds, 0, 1, 0) WS3_RD(f.a0, lds, 0, 0, 0)

    int64_t g = g_begin;
    int tp = 0;
    for (; g + 2 <= g_end; g += 2, tp ^= 1) s3_tile<2, KN>(a, lds, tbl, tblh, cx, ln, a_rd1, st, u, f, ursrc, n0, tp, n_chunks);
    if (g < g_end) s3_tile<1, KN>(a, lds, tbl, tblh, cx, ln, a_rd1, st, u, f, ursrc, n0, tp, n_chunks);
}

#if WS3_KNOCK_HEAD
__global__ __launch_bounds__(256, 2) void tdnn_wino_s3_kernel(const TdnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    if constexpr (WS3_KNOCK_MODE > 1) s3_block<(WS3_KNOCK_MODE == 2 ? 2 : 1)>(a, lds);
    else if ((xcd_remap(blockIdx.x, gridDim.x) % a.n_tiles) & 1) s3_block<1>(a, lds);      // block_setup: the block's column tile
    else s3_block<0>(a, lds);
}
#endif
#undef WS3_CHUNK
#undef WS3_PRODUCT2
#undef WS3_PRODUCT1
#undef WS3_ULD
#undef WS3_RD
#undef WS3_MF

}  // namespace wino

bool tdnn_wino_s3_applicable(const TdnnGeom& g, int ldx) {
    return tdnn_wino_applicable(g, ldx) && (g.kpt_pad / wino::kS3K) % 2 == 0;
}

hipError_t launch_tdnn_wino_s3(const TdnnArgs& a, hipStream_t s) {
    if (a.groups_total <= 0 || a.blocks_per_col <= 0 || a.blocks_per_col > a.groups_total || a.tap_rows < 1 || a.cpt < 1 ||
        a.Wf == nullptr || (a.out_map.offsets == nullptr && a.p_fixed < 1))
        return hipErrorInvalidValue;
    const int grid = a.blocks_per_col * a.n_tiles;
    wino::tdnn_wino_s3_kernel<<<dim3(grid), dim3(256), wino::kS3LdsBytes, s>>>(a);
    return hipGetLastError();
}

}  // namespace xvec
