// The host side of DER scoring (csrc/der.hip, include/xvec_der.h): the argument checks (one text per refusal), the layout of
// the workspace and the launch plan.  Host-compilable (no HIP header, like vbx_plan.h), so that tests/test_der.py can ask it
// on the CPU (tests/abi/der_plan_dump.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/xvec_der.h"
#include "rec_plan.h"

namespace xvec {
namespace der_plan {

constexpr int32_t kChunk = XVEC_DER_CHUNK_TICKS;
constexpr int32_t kThreads = XVEC_DER_THREADS;
constexpr int32_t kSpk = XVEC_DER_MAX_SPEAKERS;
constexpr int32_t kTurnsPerBlock = XVEC_DER_THREADS / 64;      // the rasteriser: a wave per turn
static_assert(XVEC_DER_CHUNK_TICKS == XVEC_DER_THREADS * XVEC_DER_WAVE_ROWS, "the rows of a block's waves tile its chunk");

// rec_start [n_rec + 1]: from 0, every recording with a tick or more, fewer than 2^31 ticks in all.
// 0, or 1 with the reason in why.
inline int check_rec_start(const int64_t* rs, int32_t n_rec, Refusal& why) {
    return rec_plan::check_rec_start(rs, n_rec, {"tick", 0, ""}, why);
}

// The turn counts of the two sides (a wave of the rasteriser each: their sum must leave the grid below 2^31 blocks).
inline int check_turn_counts(int64_t m_ref, int64_t m_hyp, Refusal& why) {
    if (m_ref < 0) return why.refuse("m_ref = %lld must not be negative", (long long)m_ref);
    if (m_hyp < 0) return why.refuse("m_hyp = %lld must not be negative", (long long)m_hyp);
    if (m_ref > 0x7fffffff || m_hyp > 0x7fffffff)
        return why.refuse("%lld and %lld turns: a side may have 2^31 - 1 at most", (long long)m_ref, (long long)m_hyp);
    return 0;
}

inline int check_collar(int32_t collar, Refusal& why) {
    if (collar < 0) return why.refuse("collar = %d must not be negative", collar);
    return 0;
}

// A turn list with its count: a list of no turns may be a null pointer, any other may not.
inline int check_turns(const void* turns, int64_t m, const char* side, Refusal& why) {
    if (m > 0 && !turns) return why.refuse("null pointer: %s_turns with m_%s = %lld", side, side, (long long)m);
    return 0;
}

// Byte offsets of the workspace's parts (each 256-byte aligned) for checked arguments.  Every per-tick part is one array over
// the N ticks of the batch: recording r owns the entries rec_start[r] .. rec_start[r + 1] - 1.  Everything from zero_from to
// total is zeroed at the start of a call (one memset); the two parts in front of it are written in full.
struct Layout {
    size_t rec_start;      // int64 [n_rec + 1]: the copy of rec_start_host
    size_t blk_start;      // int32 [n_rec + 1]: the first block of every recording in the counting pass (written on the device)
    size_t ref_mask;       // uint64 [N]: R_t
    size_t hyp_mask;       // uint64 [N]: H_t
    size_t noscore;        // uint32 [N / 32 + 1]: a bit per tick, the collar zones
    size_t acc;            // int64 [n_rec, 4]: scored, total, miss, fa
    size_t ignored;        // int64 [2]
    size_t cooc;           // int64 [n_rec, 64, 64]
    size_t zero_from;      // = ref_mask
    size_t total;
};

inline Layout make_layout(const int64_t* rs, int32_t n_rec) {
    Layout l{};
    const size_t N = (size_t)rs[n_rec], R = (size_t)n_rec;
    Carver c;
    l.rec_start = c.take_bytes((R + 1) * sizeof(int64_t));
    l.blk_start = c.take_bytes((R + 1) * sizeof(int32_t));
    l.ref_mask = c.take_bytes(N * sizeof(uint64_t));
    l.hyp_mask = c.take_bytes(N * sizeof(uint64_t));
    l.noscore = c.take_bytes((N / 32 + 1) * sizeof(uint32_t));
    l.acc = c.take_bytes(R * 4 * sizeof(int64_t));
    l.ignored = c.take_bytes(2 * sizeof(int64_t));
    l.cooc = c.take_bytes(R * (size_t)kSpk * (size_t)kSpk * sizeof(int64_t));
    l.zero_from = l.ref_mask;
    l.total = c.total();
    return l;
}

// The counting pass: a block owns kChunk consecutive ticks of ONE recording; the blocks of recording r are
// first_block(r) .. first_block(r + 1) - 1 in the order of their chunks.
inline int64_t chunks_of(int64_t ticks) { return (ticks + kChunk - 1) / kChunk; }

inline int64_t pass_blocks(const int64_t* rs, int32_t n_rec) {
    int64_t b = 0;
    for (int32_t r = 0; r < n_rec; ++r) b += chunks_of(rs[r + 1] - rs[r]);
    return b;          // <= the ticks of the batch < 2^31
}

struct Chunk {
    int32_t rec;
    int32_t chunk;
    int64_t first_tick;    // in the recording
    int32_t ticks;         // 1 .. kChunk
};

// The host restatement of what a block of the pass finds by bisection in blk_start.
inline Chunk block_chunk(const int64_t* rs, int32_t n_rec, int64_t block) {
    int64_t first = 0;
    for (int32_t r = 0; r < n_rec; ++r) {
        const int64_t n = rs[r + 1] - rs[r], c = chunks_of(n);
        if (block < first + c) {
            const int64_t k = block - first, t0 = k * kChunk;
            return Chunk{r, (int32_t)k, t0, (int32_t)(n - t0 < kChunk ? n - t0 : kChunk)};
        }
        first += c;
    }
    return Chunk{-1, -1, -1, 0};
}

using rec_plan::Launch;

// The rasteriser: a wave per turn of either side, and one block more that lays out blk_start.
inline Launch raster_launch(int64_t m_ref, int64_t m_hyp) {
    return Launch{(m_ref + m_hyp + kTurnsPerBlock - 1) / kTurnsPerBlock + 1, kThreads};
}
inline Launch pass_launch(const int64_t* rs, int32_t n_rec) { return Launch{pass_blocks(rs, n_rec), kThreads}; }
// The solver: a wave per recording.  The pooling: one block.
inline Launch assign_launch(int32_t n_rec) { return Launch{n_rec, 64}; }
inline Launch pool_launch() { return Launch{1, kThreads}; }

}  // namespace der_plan
}  // namespace xvec
