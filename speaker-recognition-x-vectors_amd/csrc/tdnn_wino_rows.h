// Pair-space machinery of the Winograd F(2,3) kernels (tdnn_wino.hip: the pair space is described there), shared by the
// translation units that use it: tdnn_wino.hip (fp32 operands) and tdnn_wino_s3.hip (bf16_split3 operands).  A tile is
// kPairs = 64 pairs (two 32-pair groups); every thread (r0 = tid >> 3, c) stages pairs q0 + r0 and q0 + r0 + 32 at 16-byte
// column c of the chunk, and set_rows fills the tile's output-row tables (kTbl ints per parity).
#pragma once
#include "tdnn_common.h"

namespace xvec {
namespace wino {

constexpr int kPairs = 64;                          // pairs of a tile
constexpr int kTbl = 2 * kPairs;                    // per tile parity: output row of y(t) per pair | of y(t+d) (-1: none)

__device__ __forceinline__ float4 ld16(__amdgpu_buffer_rsrc_t rsrc, int voff, int soff) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0);
    const f32x4 f = __builtin_bit_cast(f32x4, v);
    return make_float4(f.x, f.y, f.z, f.w);
}

// pairs of an utterance with T output frames (wino_pair_count on the device)
__device__ __forceinline__ int pair_count(int T, int d) { return d * (T / (2 * d)) + min(T % (2 * d), d); }

struct Ctx {
    __amdgpu_buffer_rsrc_t xrsrc;   // X + in_base*ldx: the load tile's first input row
    __amdgpu_buffer_rsrc_t wrsrc;   // U + n0*k_pad
    int x00, x30, x01, x31;         // byte offsets of rows x0 and x3 of this thread's pair in groups 0, 1 (+ its 16-byte column)
    int drb;                        // d rows in bytes (x1 = x0 + drb, x2 = x0 + 2 drb)
    int w_toff;
    int u_tile;                     // utterance holding pair q0, and the first pair of the next one
    int64_t nb_next;
    int64_t q0;                     // first pair of the tile the load stream is in
    int64_t g_s, g_end;             // its first 32-pair group; end of the block's range
    int kk, kc, itl;                // next chunk to fetch: product kk of K chunk kc, linear index itl in the tile
    int lp;                         // parity of the load stream's tile (row tables)
};

struct Lane {
    int h, sw, a_rd, b_rd, st_off, r0, c, col;
};

// Input offsets and output rows of the 64 pairs of the tile at pair cx.q0.  The utterance of the tile's first pair is
// tracked incrementally (tiles only move forward); the utterance starts inside the tile are walked with block-uniform
// values (scalar loads of the offsets for ragged batches), each lane selecting the ones its pairs have passed -- no
// division over the batch and no vector-memory load whose wait would drain the staging loads in flight.
template <bool RAGGED>
__device__ __forceinline__ void set_rows_impl(const WinoArgs& a, Ctx& cx, const Lane& ln, int* tbl, int64_t* tblh) {
    const RowMap& m = a.out_map;
    const int n_last = m.n_utts - 1, d = a.d;
    const int64_t t_fix = (int64_t)m.fixed_T - m.cum;
    auto ro = [&](int u) -> int64_t {       // first compact output row of utterance u (u <= n_utts)
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
    const int p_t = pair_count(to_t, d);
    if (j0 > p_t - 1) j0 = p_t - 1;
    const int64_t i0 = j0 + d * (j0 / d);
    const int64_t ob = ro_t + i0;                                  // output row of the tile's first pair
    const int64_t in_base = ro_t + (int64_t)ut * a.span + i0;      // its input row x0
    cx.xrsrc = make_rsrc(a.X + in_base * a.ldx);
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
        const bool valid = jl < pair_count(to, d);
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
    cx.drb = d * rb;
    // output rows for the epilogue of this tile: every thread of a row writes the same values (8 per pair)
    int* t = tbl + cx.lp * kTbl;
    t[ln.r0] = o0a;
    t[ln.r0 + 32] = o0b;
    t[kPairs + ln.r0] = o1a;
    t[kPairs + ln.r0 + 32] = o1b;
    tblh[cx.lp] = ob;
}

__device__ __forceinline__ void set_rows(const WinoArgs& a, Ctx& cx, const Lane& ln, int* tbl, int64_t* tblh) {
    if (a.out_map.offsets == nullptr) set_rows_impl<false>(a, cx, ln, tbl, tblh);
    else set_rows_impl<true>(a, cx, ln, tbl, tblh);
}

// Range of 32-pair groups of block p of a column (the CU-pair-aware split of tdnn_layer.hip)
__device__ __forceinline__ void group_range(const WinoArgs& a, int p, int64_t& g_begin, int64_t& g_end) {
    if (a.pair_period > 0) {
        const int P = a.blocks_per_col, PQ = a.pair_period, hq = PQ >> 1;
        const int64_t base = a.groups_total / P;
        const int rem = (int)(a.groups_total % P);
        const int rem1 = rem < (P >> 1) ? rem : (P >> 1), rem2 = rem - rem1;
        const int xq = p / PQ, w = p % PQ;
        const int nf = xq * hq + (w < hq ? w : hq);
        const int ns = xq * hq + (w > hq ? w - hq : 0);
        g_begin = base * p + (nf < rem1 ? nf : rem1) + (ns < rem2 ? ns : rem2);
        const bool extra = (w < hq) ? (nf < rem1) : (ns < rem2);
        g_end = g_begin + base + (extra ? 1 : 0);
    } else {
        g_begin = a.groups_total * (int64_t)p / a.blocks_per_col;
        g_end = a.groups_total * (int64_t)(p + 1) / a.blocks_per_col;
    }
}

// The utterance of the block's first pair cx.q0 (largest u with pb(u) <= q0) and the first pair of the next one
__device__ __forceinline__ void first_utterance(const WinoArgs& a, Ctx& cx) {
    const RowMap& m = a.out_map;
    int u;
    if (m.offsets == nullptr) {
        const int64_t uu = cx.q0 / a.p_fixed;
        u = (int)(uu < m.n_utts - 1 ? uu : m.n_utts - 1);
    } else {
        int lo = 0, hi = m.n_utts;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if ((row_off(m, mid) >> 1) + (int64_t)mid * a.d <= cx.q0) lo = mid; else hi = mid;
        }
        u = lo;
    }
    cx.u_tile = __builtin_amdgcn_readfirstlane(u);
    const int64_t rn = row_off(m, cx.u_tile + 1);
    cx.nb_next = m.offsets ? (rn >> 1) + (int64_t)(cx.u_tile + 1) * a.d : (int64_t)(cx.u_tile + 1) * a.p_fixed;
}

}  // namespace wino
}  // namespace xvec
