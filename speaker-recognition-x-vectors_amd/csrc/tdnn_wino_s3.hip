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
// buffer is [product][plane][64 pairs][16 k] bf16 = 24 KiB; two buffers, one barrier per chunk.  The U planes go from
// global memory straight into the MFMA B operands (fragment-major, pack.hip: 12 KiB per wave and chunk, reloaded product
// by product as soon as the previous chunk's MFMAs of that product have issued).
//   per block and chunk: 16 KiB of input rows + 48 KiB of U planes over 4 waves x 4 products x 2 groups x 6 = 192 MFMAs
//   = 341 B per MFMA (the direct port of tdnn_wino.hip's tile: 427).
#include "tdnn_wino_rows.h"

namespace xvec {
namespace wino {

constexpr int kS3K = 16;                                  // k per chunk (one bf16 k-step)
constexpr int kS3Plane = kPairs * kS3K * 2;               // bytes of one (product, plane) block: 64 pairs x 32 B
constexpr int kS3Stage = 4 * 3 * kS3Plane;                // one LDS buffer: 4 products x hi | mid | lo
constexpr int kS3Const = kConst * 4;                      // bias | scale | shift of the tile's channels, bytes
constexpr int kS3LdsBytes = 2 * kS3Stage + kS3Const + 2 * kTbl * 4 + 2 * 8;   // + row tables, per parity the base row

// Step the load stream to the next chunk; after a tile's last chunk, to chunk 0 of the block's next tile.  Past the block's
// last chunk it stays put (the look-ahead re-reads that chunk; the data is never used).
__device__ __forceinline__ void s3_advance(const TdnnArgs& a, Ctx& cx, const Lane& ln, int* tbl, int64_t* tblh, int n_chunks) {
    if (cx.kc + 1 < n_chunks) {
        ++cx.kc;
    } else {
        const int64_t g_rem = cx.g_end - cx.g_s;
        const int64_t g_next = cx.g_s + (g_rem < 2 ? g_rem : 2);
        if (g_next < cx.g_end) {
            cx.g_s = g_next;
            cx.q0 = g_next * 32;
            cx.lp ^= 1;
            set_rows(a, cx, ln, tbl, tblh);
            cx.kc = 0;
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

// the three U-plane fragments (hi | mid | lo) of product k of chunk c of this wave's column; the stream wraps to chunk 0
// past the tile's last chunk (the next tile of the block is in the same channel column)
__device__ __forceinline__ void s3_uld(__amdgpu_buffer_rsrc_t rsrc, int voff, float4* w, int k, int c, int n_chunks) {
    if (c >= n_chunks) c -= n_chunks;
#pragma unroll
    for (int p = 0; p < 3; ++p) w[p] = buf_load16(rsrc, voff, ((4 * c + k) * 3 + p) * 1024);
}

// One tile of G pair groups x 128 channels; tp = its row-table parity.  On entry chunk 0 of the tile is in LDS buffer 0,
// the U planes of chunk 0 are in w, and the staging registers hold chunk 1 (block prologue or the previous tile's chunks).
template <int G>
__device__ __forceinline__ void s3_tile(const TdnnArgs& a, char* lds, int* tbl, int64_t* tblh, Ctx& cx, const Lane& ln,
                                        S3Stage& st, float4 (&w)[4][3], __amdgpu_buffer_rsrc_t ursrc, int n0, int tp,
                                        int n_chunks) {
    const bool grp = (threadIdx.x >> 2) & 1;
    f32x16 acc0_0, acc0_1, acc1_0, acc1_1, acc2_0, acc2_1, acc3_0, acc3_1;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        acc0_0[e] = 0.f; acc1_0[e] = 0.f; acc2_0[e] = 0.f; acc3_0[e] = 0.f;
        acc0_1[e] = 0.f; acc1_1[e] = 0.f; acc2_1[e] = 0.f; acc3_1[e] = 0.f;
    }
    // ---- K chunks: chunk it in buffer it & 1 (n_chunks is even, so every tile starts in buffer 0)
    for (int it = 0; it < n_chunks; ++it) {
        const char* S = lds + (it & 1) * kS3Stage;
        char* Sn = lds + ((it & 1) ^ 1) * kS3Stage;
        // chunk it + 1 -> the other buffer (free: every wave passed the barrier behind its last read of chunk it - 1),
        // then the staging registers receive the chunk after it
        s3_vstore(Sn, ln.st_off, st);
        s3_advance(a, cx, ln, tbl, tblh, n_chunks);
        s3_gld(cx, grp, st);
#define WS3_PRODUCT(K_)                                                                                        \
        {                                                                                                      \
            float4 xf0[3], xf1[3];                                                                             \
            _Pragma("unroll") for (int pl = 0; pl < 3; ++pl) {                                                 \
                xf0[pl] = *reinterpret_cast<const float4*>(S + (3 * K_ + pl) * kS3Plane + ln.a_rd);            \
                if constexpr (G > 1)                                                                           \
                    xf1[pl] = *reinterpret_cast<const float4*>(S + (3 * K_ + pl) * kS3Plane + 32 * 32 + ln.a_rd); \
            }                                                                                                  \
            s3_mfma6(acc##K_##_0, xf0, w[K_]);                                                                 \
            if constexpr (G > 1) s3_mfma6(acc##K_##_1, xf1, w[K_]);                                            \
            s3_uld(ursrc, ln.b_rd, w[K_], K_, it + 1, n_chunks);                                               \
        }
        WS3_PRODUCT(0) WS3_PRODUCT(1) WS3_PRODUCT(2) WS3_PRODUCT(3)
#undef WS3_PRODUCT
        __syncthreads();   // chunk it + 1 complete in LDS; chunk it's buffer is free
    }

    epilogue<G>(a, reinterpret_cast<const float*>(lds + 2 * kS3Stage), tbl, tblh, ln, n0, tp, acc0_0, acc1_0, acc2_0, acc3_0, acc0_1,
                acc1_1, acc2_1, acc3_1);
}

__global__ __launch_bounds__(256, 2) void tdnn_wino_s3_kernel(const TdnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
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
    ln.st_off = (ln.r0 + 32 * ((tid >> 2) & 1)) * (kS3K * 2) + (tid & 3) * 8;   // byte offset in a plane block
    ln.a_rd = ln.r * (kS3K * 2) + ln.h * 16;     // A fragment of lane (r, h): pair r of the group, k 8h .. 8h + 7
    ln.b_rd = lane * 16;                      // U fragment: 16 bytes per lane of a 1 KiB block
    ln.sw = 0;
    // U planes of this wave's 32-channel column: 12 KiB per chunk ((chunk, product, plane) blocks of 1 KiB)
    const int64_t ct = n0 / 32 + wave;
    const __amdgpu_buffer_rsrc_t ursrc = make_rsrc(static_cast<const char*>(a.Wf) + ct * (int64_t)n_chunks * 12288);

    stream_start(a, n0, cst, tbl, tblh, cx, ln);

    // prologue: chunk 0 -> LDS buffer 0, the U planes of chunk 0 -> w, chunk 1 in the staging registers
    const bool grp = (tid >> 2) & 1;
    S3Stage st;
    float4 w[4][3];
    s3_gld(cx, grp, st);
#pragma unroll
    for (int k = 0; k < 4; ++k) s3_uld(ursrc, ln.b_rd, w[k], k, 0, n_chunks);
    s3_vstore(lds, ln.st_off, st);
    s3_advance(a, cx, ln, tbl, tblh, n_chunks);
    s3_gld(cx, grp, st);
    __syncthreads();

    int64_t g = g_begin;
    int tp = 0;
    for (; g + 2 <= g_end; g += 2, tp ^= 1) s3_tile<2>(a, lds, tbl, tblh, cx, ln, st, w, ursrc, n0, tp, n_chunks);
    if (g < g_end) s3_tile<1>(a, lds, tbl, tblh, cx, ln, st, w, ursrc, n0, tp, n_chunks);
}

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
