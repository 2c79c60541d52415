// What the two Winograd F(2,3) kernels share (tdnn_wino.hip: fp32 operands, the math and the pair space are described there;
// tdnn_wino_s3.hip: bf16_split3 operands): the pair-space machinery, the block set-up and the epilogue.  A tile is kPairs = 64
// pairs (two 32-pair groups) x kBN channels; every thread (r0 = tid >> 3, c) stages pairs q0 + r0 and q0 + r0 + 32 at 16-byte
// column c of the chunk, and set_rows fills the tile's output-row tables (kTbl ints per parity).  Both kernels read TdnnArgs
// as xvec_internal.h says at launch_tdnn_wino.
#pragma once
#include "tdnn_common.h"

namespace xvec {
namespace wino {

constexpr int kPairs = 64;                          // pairs of a tile
constexpr int kBN = 128;                            // channels of a tile: four waves of 32
constexpr int kConst = 3 * kBN;                     // floats: bias | scale | shift of the tile's channels
constexpr int kTbl = 2 * kPairs;                    // per tile parity: output row of y(t) per pair | of y(t+d) (-1: none)

struct Ctx {
    __amdgpu_buffer_rsrc_t xrsrc;   // X + in_base*ldx: the load tile's first input row
    __amdgpu_buffer_rsrc_t wrsrc;   // U + n0*k_pad
    int x00, x30, x01, x31;         // byte offsets of rows x0 and x3 of this thread's pair in groups 0, 1 (+ its 16-byte column)
    int drb;                        // d rows in bytes (x1 = x0 + drb, x2 = x0 + 2 drb); stream_start
    int w_toff;
    int u_tile;                     // utterance holding pair q0, and the first pair of the next one
    int64_t nb_next;
    int64_t q0;                     // first pair of the tile the load stream is in
    int64_t g_s, g_end;             // its first 32-pair group; end of the block's range
    int kk, kc, itl;                // next chunk to fetch: product kk of K chunk kc, linear index itl in the tile
    int lp;                         // parity of the load stream's tile (row tables)
};

struct Lane {
    int wave, r, h, r0, c, col;     // block_setup: wave, row of the 32 x 32 fragment, lane half; staging row and 16-byte column
                                    // (set_rows); channel
    int sw, a_rd, b_rd, st_off;     // the kernel's own LDS / fragment offsets
};

// Input offsets and output rows of the 64 pairs of the tile at pair cx.q0.  The utterance of the tile's first pair is
// tracked incrementally (tiles only move forward); the utterance starts inside the tile are walked with block-uniform
// values (scalar loads of the offsets for ragged batches), each lane selecting the ones its pairs have passed -- no
// division over the batch and no vector-memory load whose wait would drain the staging loads in flight.
template <bool RAGGED>
__device__ __forceinline__ void set_rows_impl(const TdnnArgs& a, Ctx& cx, const Lane& ln, int* tbl, int64_t* tblh) {
    const RowMap& m = a.out_map;
    const int n_last = m.n_utts - 1, d = a.tap_rows;
    const int64_t t_fix = (int64_t)m.fixed_T - m.cum;
    // first compact output row of utterance u (u <= n_utts): first_row (tdnn_common.h) without its readfirstlane -- every u
    // below is a uniform value already (cx.u_tile and the walk's counter are kept so), and the extra copy per call made hipcc
    // arrange the 64-bit row arithmetic of this function differently in both kernels
    auto ro = [&](int u) -> int64_t {
        if (RAGGED) return sload_i64(m.offsets + u) - (int64_t)u * m.cum;
        return (int64_t)u * t_fix;
    };
    auto pb = [&](int u, int64_t r) -> int64_t {   // first pair of utterance u, whose first row is r
        if (RAGGED) return (r >> 1) + (int64_t)u * d;
        return (int64_t)u * a.p_fixed;
    };
    while (cx.q0 >= cx.nb_next && cx.u_tile < n_last) {
        cx.u_tile = __builtin_amdgcn_readfirstlane(cx.u_tile + 1);
        cx.nb_next = pb(cx.u_tile + 1, ro(cx.u_tile + 1));
    }
    const int ut = cx.u_tile;
    const int64_t ro_t = ro(ut), ro_n = ro(ut + 1), pb_t = pb(ut, ro_t);
    const int to_t = (int)(ro_n - ro_t);
    // the tile's bases: its first pair (clamped to the utterance's last pair, for a tile that starts in a hole)
    int64_t j0 = cx.q0 - pb_t;
    const int p_t = wino_pair_count(to_t, d);
    if (j0 > p_t - 1) j0 = p_t - 1;
    const int64_t i0 = j0 + d * (j0 / d);
    const int64_t ob = ro_t + i0;                                  // output row of the tile's first pair
    const int64_t in_base = ro_t + (int64_t)ut * a.span + i0;      // its input row x0
    cx.xrsrc = make_rsrc(static_cast<const float*>(a.X) + in_base * a.ldx);
    const int rb = a.ldx * 4;
    // this thread's two pairs (groups 0, 1)
    const int64_t qa = cx.q0 + ln.r0, qb = qa + 32;
    int ua = ut, ub = ut, toa = to_t, tob = to_t;
    int64_t roa = ro_t, rob = ro_t, pba = pb_t, pbb = pb_t;
    {
        int u = ut + 1;
        int64_t r = ro_n;
        int64_t nb = cx.nb_next;
        while (u <= n_last && nb < cx.q0 + kPairs) {         // block-uniform walk over the utterance starts in the tile
            const int64_t rn = ro(u + 1);
            const int to = (int)(rn - r);
            if (qa >= nb) { ua = u; roa = r; toa = to; pba = nb; }
            if (qb >= nb) { ub = u; rob = r; tob = to; pbb = nb; }
            u = __builtin_amdgcn_readfirstlane(u + 1);
            r = rn;
            nb = pb(u, rn);
        }
    }
    auto one = [&](int64_t q, int u, int64_t r, int to, int64_t p0, int& o0, int& o1, int& x0, int& x3) {
        const int jl = (int)(q - p0);
        const bool valid = jl < wino_pair_count(to, d);
        const int i = jl + d * (jl / d);
        const bool second = valid && i + d < to;
        // pairs past the batch or in a ragged hole read the tile's first rows (valid frames) and store nothing
        const int rin = valid ? (int)(r + (int64_t)u * a.span + i - in_base) : 0;
        x0 = rin * rb + ln.c * 16;
        // a one-output tile: x3 would be past the utterance (another utterance's row, or padding that may hold NaN);
        // x1 instead (V3 = x1 - x1 = 0), and y(t+d) is not stored
        x3 = x0 + (second ? 3 : 1) * d * rb;
        o0 = valid ? (int)(r + i - ob) : -1;
        o1 = second ? o0 + d : -1;
    };
    int o0a, o1a, o0b, o1b;
    one(qa, ua, roa, toa, pba, o0a, o1a, cx.x00, cx.x30);
    one(qb, ub, rob, tob, pbb, o0b, o1b, cx.x01, cx.x31);
    // output rows for the epilogue of this tile: every thread of a row writes the same values (8 per pair)
    int* t = tbl + cx.lp * kTbl;
    t[ln.r0] = o0a;
    t[ln.r0 + 32] = o0b;
    t[kPairs + ln.r0] = o1a;
    t[kPairs + ln.r0 + 32] = o1b;
    tblh[cx.lp] = ob;
}

__device__ __forceinline__ void set_rows(const TdnnArgs& a, Ctx& cx, const Lane& ln, int* tbl, int64_t* tblh) {
    if (a.out_map.offsets == nullptr) set_rows_impl<false>(a, cx, ln, tbl, tblh);
    else set_rows_impl<true>(a, cx, ln, tbl, tblh);
}

// The utterance of the block's first pair cx.q0 (largest u with pb(u) <= q0) and the first pair of the next one
__device__ __forceinline__ void first_utterance(const TdnnArgs& a, Ctx& cx) {
    const RowMap& m = a.out_map;
    int u;
    if (m.offsets == nullptr) {
        const int64_t uu = cx.q0 / a.p_fixed;
        u = (int)(uu < m.n_utts - 1 ? uu : m.n_utts - 1);
    } else {
        int lo = 0, hi = m.n_utts;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if ((row_off(m, mid) >> 1) + (int64_t)mid * a.tap_rows <= cx.q0) lo = mid; else hi = mid;
        }
        u = lo;
    }
    cx.u_tile = __builtin_amdgcn_readfirstlane(u);
    const int64_t rn = row_off(m, cx.u_tile + 1);
    cx.nb_next = m.offsets ? (rn >> 1) + (int64_t)(cx.u_tile + 1) * a.tap_rows : (int64_t)(cx.u_tile + 1) * a.p_fixed;
}

// Block set-up of both kernels, in two parts with the kernel's own lane offsets (ln.sw, a_rd, b_rd, st_off) and weight
// descriptor in between -- the order the kernels were scheduled in: moving those behind the constants' store below changed
// hipcc's instruction order inside the bf16_split3 K loop.  Part 1: logical block id -> channel column (returned: its first
// channel n0) and range of 32-pair groups (cx.g_s, cx.g_end); the lane roles that do not depend on the kernel's LDS layout
// (c = tid & c_mask: the 16-byte column set_rows addresses).
// BN: channels of the block's tile (kBN; tdnn_wino_s3w.hip: 256 on eight waves).
template <int BN = kBN>
__device__ __forceinline__ int block_setup(const TdnnArgs& a, int c_mask, Ctx& cx, Lane& ln) {
    // the n_tiles columns of one range are consecutive ids on one XCD
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int n0 = (lid % a.n_tiles) * BN;
    int64_t g_begin, g_end;
    group_range(a, lid / a.n_tiles, g_begin, g_end);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    ln.wave = tid >> 6;
    ln.h = lane >> 5;
    ln.r = lane & 31;
    ln.c = tid & c_mask;
    ln.r0 = tid >> 3;
    ln.col = n0 + ln.wave * 32 + ln.r;
    cx.g_s = g_begin;
    cx.g_end = g_end;
    return n0;
}

// Part 2: bias | scale | shift of the column -> cst (LDS, kConst floats); the load stream at chunk 0 of the block's first tile
// with that tile's rows set.  cx.drb is a constant of the launch and is set HERE, once: assigned again by every set_rows it was
// a loop-carried value that hipcc kept in a vector register, and every input-row load of tdnn_wino_kernel's K loop that adds
// it to its scalar offset was wrapped in a v_readfirstlane / v_cmp_eq / s_and_saveexec loop (34 of them, 4-6 % of the kernel).
template <int BN = kBN>
__device__ __forceinline__ void stream_start(const TdnnArgs& a, int n0, float* cst, int* tbl, int64_t* tblh, Ctx& cx, const Lane& ln) {
    const int tid = threadIdx.x;
    if (tid < BN) {
        cst[tid] = a.bias[n0 + tid];
        cst[BN + tid] = a.scale[n0 + tid];
        cst[2 * BN + tid] = a.shift[n0 + tid];
    }
    cx.q0 = cx.g_s * 32;
    first_utterance(a, cx);
    cx.lp = 0;
    cx.drb = a.tap_rows * a.ldx * 4;
    set_rows(a, cx, ln, tbl, tblh);
    cx.kk = 0;
    cx.kc = 0;
    cx.itl = 0;
}

// Epilogue of a tile of G pair groups (tp: its row-table parity; acc<k>_<i>: product k of group i): y(t) = M0 + M1 + M2,
// y(t+d) = M1 - M2 - M3, then bias + ReLU + folded BatchNorm (tdnn_layer.py:30-39), stored to the rows set_rows tabled (-1:
// none).  Accumulator element e of lane (r, h): pair = (e&3) + 8*(e>>2) + 4*h of the group, channel = r.
template <int G, int BN = kBN>
__device__ __forceinline__ void epilogue(const TdnnArgs& a, const float* cst, const int* tbl, const int64_t* tblh, const Lane& ln,
                                         int n0, int tp, const f32x16& acc0_0, const f32x16& acc1_0, const f32x16& acc2_0,
                                         const f32x16& acc3_0, const f32x16& acc0_1, const f32x16& acc1_1, const f32x16& acc2_1,
                                         const f32x16& acc3_1) {
    const int h = ln.h, col = ln.col;
    cst += col - n0;
    const float bi = cst[0], sc = cst[BN], sh = cst[2 * BN];
    // the tile's base row: the same in every lane (set_rows wrote it to LDS)
    const int64_t ob = (int64_t)uniform64((unsigned long long)tblh[tp]);
    const __amdgpu_buffer_rsrc_t yrsrc = make_rsrc(static_cast<float*>(a.Y) + ob * a.ldy);
    const int row_b = a.ldy * 4, col_b = col * 4;
    auto group = [&](const int* t0, const f32x16& m0, const f32x16& m1, const f32x16& m2, const f32x16& m3) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int4 r0v = *reinterpret_cast<const int4*>(t0 + 8 * g4 + 4 * h);
            const int4 r1v = *reinterpret_cast<const int4*>(t0 + kPairs + 8 * g4 + 4 * h);
            const int o0s[4] = {r0v.x, r0v.y, r0v.z, r0v.w};
            const int o1s[4] = {r1v.x, r1v.y, r1v.z, r1v.w};
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) {
                const int e = 4 * g4 + e4;
                const float y0 = fmaf(fmaxf((m0[e] + m1[e]) + m2[e] + bi, 0.f), sc, sh);
                const float y1 = fmaf(fmaxf((m1[e] - m2[e]) - m3[e] + bi, 0.f), sc, sh);
                if (o0s[e4] >= 0) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y0), yrsrc, o0s[e4] * row_b + col_b, 0, 0);
                if (o1s[e4] >= 0) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y1), yrsrc, o1s[e4] * row_b + col_b, 0, 0);
            }
        }
    };
    group(tbl + tp * kTbl, acc0_0, acc1_0, acc2_0, acc3_0);
    if constexpr (G > 1) group(tbl + tp * kTbl + 32, acc0_1, acc1_1, acc2_1, acc3_1);
}

}  // namespace wino
}  // namespace xvec
