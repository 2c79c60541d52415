// The host side of energy VAD and sliding CMVN (csrc/vad.hip, include/xvec_vad.h): the window of a frame (the same text the
// kernel runs), the argument checks, the workspace layout, and the tile plan of the normalise-and-select kernel.
// Host-compilable (no HIP header, like diar_plan.h and resample_taps.h), so that tests/test_vad.py can ask it on the CPU
// (tests/abi/vad_plan_dump.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/xvec_vad.h"
#include "plan_support.h"

#if defined(__HIPCC__)
#define XVEC_VAD_FN __host__ __device__ __forceinline__
#else
#define XVEC_VAD_FN inline
#endif

namespace xvec {
namespace vad_plan {

// The window [lo, hi) of frame t in an utterance of L frames (0 <= t < L), include/xvec_vad.h.  0 <= lo <= t < hi <= L and
// hi - lo <= span(cmn_window, min_window, center); from t to t + 1 lo rises by 0 or 1 and hi never falls.
XVEC_VAD_FN void window(int t, int L, int cmn_window, int min_window, int center, int* lo_out, int* hi_out) {
    int lo, hi;
    if (center) {
        lo = t - cmn_window / 2;
        hi = lo + cmn_window;
    } else {
        lo = t - cmn_window;
        hi = t + 1;
    }
    if (lo < 0) {
        hi -= lo;
        lo = 0;
    }
    if (!center && hi > t) hi = t + 1 > min_window ? t + 1 : min_window;
    if (hi > L) {
        lo -= hi - L;
        hi = L;
        if (lo < 0) lo = 0;
    }
    *lo_out = lo;
    *hi_out = hi;
}

// The most frames a window holds: what a tile's halo is sized by.  Without normalisation (cmvn == NULL) a frame reads itself.
inline int span(const xvec_cmvn_options* o) {
    if (!o) return 1;
    if (o->center) return o->cmn_window;
    return o->cmn_window + 1 > o->min_window ? o->cmn_window + 1 : o->min_window;
}

// The chunks of XVEC_VAD_LANES frames of an utterance of T frames.
XVEC_VAD_FN int chunks(int T) { return (T + XVEC_VAD_LANES - 1) / XVEC_VAD_LANES; }

// ---------------------------------------------------------------- argument checks: 0, or 1 with the reason in why

inline int check_shape(int32_t B, int32_t T, int32_t C, int64_t row_stride, int64_t utt_stride, const char* what, Refusal& why) {
    if (B < 1 || T < 1 || C < 1) return why.refuse("B = %d, T = %d, C = %d: every one must be at least 1", B, T, C);
    if (C > XVEC_VAD_MAX_CHANNELS)
        return why.refuse("C = %d is over XVEC_VAD_MAX_CHANNELS = %d", C, XVEC_VAD_MAX_CHANNELS);
    if (row_stride < C) return why.refuse("%s row stride %lld is smaller than C = %d", what, (long long)row_stride, C);
    const int64_t need = (int64_t)(T - 1) * row_stride + C;
    if (utt_stride < need)
        return why.refuse("%s utterance stride %lld is smaller than the %lld floats of an utterance", what, (long long)utt_stride,
                          (long long)need);
    return 0;
}

inline int check_mask_stride(int64_t mask_stride, int32_t T, Refusal& why) {
    if (mask_stride < T) return why.refuse("mask stride %lld is smaller than T = %d", (long long)mask_stride, T);
    return 0;
}

inline int check_vad(const xvec_vad_options* o, int32_t C, Refusal& why) {
    if (!o) return why.refuse("null pointer: vad options");
    if (o->energy_threshold != o->energy_threshold || o->energy_mean_scale != o->energy_mean_scale)
        return why.refuse("energy_threshold or energy_mean_scale is NaN");
    if (!(o->proportion_threshold > 0.0 && o->proportion_threshold < 1.0))
        return why.refuse("proportion_threshold = %g must lie strictly between 0 and 1", o->proportion_threshold);
    if (o->frames_context < 0) return why.refuse("frames_context = %d must not be negative", o->frames_context);
    if (o->energy_col < 0 || o->energy_col >= C)
        return why.refuse("energy_col = %d must lie in 0 .. C - 1 = %d", o->energy_col, C - 1);
    return 0;
}

// (a null pointer is fine: no normalisation)
inline int check_cmvn(const xvec_cmvn_options* o, Refusal& why) {
    if (!o) return 0;
    if (o->cmn_window < 1 || o->cmn_window > XVEC_CMVN_MAX_WINDOW)
        return why.refuse("cmn_window = %d must lie in 1 .. XVEC_CMVN_MAX_WINDOW = %d", o->cmn_window, XVEC_CMVN_MAX_WINDOW);
    if (o->min_window < 1 || o->min_window > XVEC_CMVN_MAX_WINDOW + 1)
        return why.refuse("min_window = %d must lie in 1 .. XVEC_CMVN_MAX_WINDOW + 1 = %d", o->min_window, XVEC_CMVN_MAX_WINDOW + 1);
    return 0;
}

// ---------------------------------------------------------------- workspace

// Byte offsets of the workspace's parts (each 256-byte aligned).
struct Layout {
    size_t prefix;      // int32 [B, chunks(T)]: the voiced frames of the utterance in front of every chunk
    size_t count;       // int32 [B]: the voiced frames of every utterance
    size_t total;
};

inline Layout make_layout(int32_t B, int32_t T) {
    Layout l{};
    if (B < 1 || T < 1) return l;
    Carver c;
    l.prefix = c.take_bytes((size_t)B * (size_t)chunks(T) * sizeof(int32_t));
    l.count = c.take_bytes((size_t)B * sizeof(int32_t));
    l.total = c.total();
    return l;
}

// ---------------------------------------------------------------- the tile plan of the normalise-and-select kernel

// A block stages `rows` rows of `channels` fp32 values: the tile's `frames` frames and the halo of their windows.  Tiles start
// at multiples of `frames` from the utterance's first frame, groups at multiples of `channels` from channel 0.  `frames` is a
// power of two that divides XVEC_VAD_LANES: a tile never straddles a chunk.
struct Tile {
    int32_t frames, channels, rows;
    size_t lds_bytes;      // rows * channels * 4 <= XVEC_CMVN_LDS_BYTES
    int32_t run;           // consecutive frames of one channel a thread slides its window sums over (run_frames)
};

// The block's XVEC_VAD_LANES threads share the tile as (channel, run of frames) items: as many runs as whole sets of the
// group's channels fit the block (one at least, the tile's frames at most), each of this many frames.  The sums of a run's
// first frame are formed directly, the following frames slide them: the partition is part of the arithmetic (xvec_vad.h).
XVEC_VAD_FN int run_frames(int frames, int channels) {
    int runs = XVEC_VAD_LANES / channels;
    runs = runs < 1 ? 1 : (runs > frames ? frames : runs);
    return (frames + runs - 1) / runs;
}

// The tallest tile first (the halo is read again by every tile), all channels before a split of them (a split reads nothing
// twice, but shortens the contiguous run of a row); groups halve down to XVEC_CMVN_GROUP_MIN channels.  0, or 1 when even the
// smallest tile of the smallest group is over the budget (never for arguments that passed check_shape and check_cmvn).
inline int plan_tile(int32_t C, int32_t span_frames, Tile* out) {
    const int32_t group_min = C < XVEC_CMVN_GROUP_MIN ? C : XVEC_CMVN_GROUP_MIN;
    for (int32_t frames = XVEC_CMVN_TILE_MAX; frames >= XVEC_CMVN_TILE_MIN; frames /= 2) {
        const int64_t rows = (int64_t)frames - 1 + span_frames;
        for (int32_t parts = 1;; parts *= 2) {
            int32_t ch = (C + parts - 1) / parts;
            if (ch < group_min) ch = group_min;
            if (rows * ch * 4 <= (int64_t)XVEC_CMVN_LDS_BYTES) {
                *out = Tile{frames, ch, (int32_t)rows, (size_t)(rows * ch * 4), run_frames(frames, ch)};
                return 0;
            }
            if (ch == group_min) break;
        }
    }
    return 1;
}

static_assert(XVEC_VAD_LANES % XVEC_CMVN_TILE_MAX == 0 && (XVEC_CMVN_TILE_MAX & (XVEC_CMVN_TILE_MAX - 1)) == 0 &&
              (XVEC_CMVN_TILE_MIN & (XVEC_CMVN_TILE_MIN - 1)) == 0, "tiles are powers of two inside a chunk");
static_assert(((int64_t)XVEC_CMVN_TILE_MIN - 1 + XVEC_CMVN_MAX_WINDOW + 1) * XVEC_CMVN_GROUP_MIN * 4 <= XVEC_CMVN_LDS_BYTES,
              "the smallest tile of the smallest group fits at the largest window");

// Blocks of the normalise-and-select launch: (utterance, tile, channel group), flattened.
inline int64_t grid_blocks(int32_t B, int32_t T, int32_t C, const Tile& t) {
    return (int64_t)B * ((T + t.frames - 1) / t.frames) * ((C + t.channels - 1) / t.channels);
}

}  // namespace vad_plan
}  // namespace xvec
