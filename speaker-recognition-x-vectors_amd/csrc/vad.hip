// Energy-based voice activity detection, sliding-window CMVN and the selection of the voiced frames: the two steps between
// the MFCC front end and the extractor.  C ABI and the definitions: include/xvec_vad.h; the host-only half (the window
// function, checks, workspace layout, tile plan): vad_plan.h.
//   decide   one block per utterance: the energy sum in the header's order and the threshold; then, chunk of 256 frames after
//            chunk, a frame's vote over t +- frames_context (the energies are read again: they are in L2), the mask, and by
//            ballot and popcount the voiced frames of the chunk.  Thread 0 writes the count in front of every chunk.
//   count    the same tally for a mask the caller brings (xvec_cmvn_sliding with a mask).
//   cmvn     one block per (utterance, tile of frames, group of channels).  The block finds every frame's output row (its rank
//            among the voiced frames: the chunk's leading count, a ballot of the chunk's mask and a popcount; the j-th unvoiced
//            frame of the utterance owns the zero row new_len + j, so the tail is written exactly once), stages the tile's rows
//            and their window halo in LDS, and a thread per (channel, run of frames) forms the window sums of the run's first
//            frame directly in fp64 and slides them over the others: what enters is added, then what leaves subtracted.
// Every loop's trip count is fixed at launch by T, C, the options and the plan; no block waits on another; no atomics.  Every
// row index the kernels derive from data (a length, a mask, a leading count) is clamped to the buffer it indexes.
#include <hip/hip_runtime.h>

#include "../../include/xvec_hip.h"
#include "../../include/xvec_vad.h"
#include "host_support.h"
#include "vad_plan.h"

// The threshold is a product and a sum, each rounded on its own: the decisions are compared bit by bit.
#pragma clang fp contract(off)

namespace xvec {
namespace {

using vad_plan::chunks;
using vad_plan::window;

constexpr int kLanes = XVEC_VAD_LANES;
constexpr int kWaves = kLanes / 64;
constexpr int kTileMax = XVEC_CMVN_TILE_MAX;
static_assert(kLanes % 64 == 0 && kTileMax <= kLanes, "whole waves; a thread per frame of a tile");

struct VadArgs {
    const float* x;
    int B, T, C;
    int64_t rs, us;                // row and utterance stride of x, in floats
    const int* lengths;            // may be null
    double thr0, scale, prop;
    int ctx, col;                  // ctx already clamped to T
    const uint8_t* mask_in;        // the count kernel's mask
    uint8_t* mask;                 // the decide kernel's
    int64_t ms;
    int* counts;                   // may be null (count kernel)
    double* thr;                   // may be null
    int* prefix;                   // workspace, may be null (xvec_vad_energy): [B, chunks(T)]
    int* count_ws;                 // workspace, may be null: [B]
};

struct CmvnArgs {
    const float* x;
    int B, T, C;
    int64_t rs, us;
    const int* lengths;
    int normalise, cmn_window, min_window, center, norm_vars;
    const uint8_t* mask;           // null: no selection
    int64_t ms;
    const int* prefix;             // with a mask: the tally of the launch before
    const int* count;
    float* y;
    int64_t yrs, yus;
    int* new_lengths;              // may be null
    int tile, group, rows_cap, run;     // the plan: frames of a tile, channels of a group, rows of LDS, frames of a run
    int n_tiles, n_groups;
};

__device__ __forceinline__ int utt_len(const int* lengths, int b, int T) {
    if (!lengths) return T;
    const int L = lengths[b];
    return L < 0 ? 0 : (L > T ? T : L);
}

// The voiced frames of the chunk the block's threads hold a frame each of, in every thread.  Two barriers.
__device__ __forceinline__ int chunk_tally(bool voiced, int* wave_cnt) {
    const unsigned long long m = __ballot(voiced);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    int n = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) n += wave_cnt[w];
    __syncthreads();
    return n;
}

// ---------------------------------------------------------------- decide

__global__ __launch_bounds__(kLanes) void vad_decide_kernel(const VadArgs g) {
    __shared__ double part[kLanes];
    __shared__ int wave_cnt[kWaves];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int L = utt_len(g.lengths, b, g.T);
    const int n_chunks = chunks(g.T);
    const float* e = g.x + (int64_t)b * g.us + g.col;
    double thr = g.thr0;
    if (g.scale != 0.0) {
        double p = 0.0;
        for (int q = 0; q < n_chunks; ++q) {
            const int t = q * kLanes + tid;
            if (t < L) p = p + (double)e[(int64_t)t * g.rs];
        }
        part[tid] = p;
        __syncthreads();
        for (int stride = kLanes / 2; stride >= 1; stride >>= 1) {
            if (tid < stride) part[tid] = part[tid] + part[tid + stride];
            __syncthreads();
        }
        const double mean = part[0] / (double)L;
        const double scaled = g.scale * mean;
        thr = g.thr0 + scaled;
    }
    int running = 0;
    for (int q = 0; q < n_chunks; ++q) {
        const int t = q * kLanes + tid;
        bool voiced = false;
        if (t < L) {
            int num = 0, den = 0;
            for (int d = -g.ctx; d <= g.ctx; ++d) {
                const int u = t + d;
                if (u < 0 || u >= L) continue;
                ++den;
                if ((double)e[(int64_t)u * g.rs] > thr) ++num;
            }
            voiced = (double)num >= (double)den * g.prop;
        }
        if (t < g.T) g.mask[(int64_t)b * g.ms + t] = voiced ? 1 : 0;
        if (tid == 0 && g.prefix) g.prefix[(int64_t)b * n_chunks + q] = running;
        running += chunk_tally(voiced, wave_cnt);
    }
    if (tid == 0) {
        g.counts[b] = running;
        if (g.count_ws) g.count_ws[b] = running;
        if (g.thr) g.thr[b] = thr;
    }
}

// ---------------------------------------------------------------- the tally of a mask the caller brings

__global__ __launch_bounds__(kLanes) void vad_count_kernel(const VadArgs g) {
    __shared__ int wave_cnt[kWaves];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int L = utt_len(g.lengths, b, g.T);
    const int n_chunks = chunks(g.T);
    int running = 0;
    for (int q = 0; q < n_chunks; ++q) {
        const int t = q * kLanes + tid;
        const bool voiced = t < L && g.mask_in[(int64_t)b * g.ms + t] != 0;
        if (tid == 0) g.prefix[(int64_t)b * n_chunks + q] = running;
        running += chunk_tally(voiced, wave_cnt);
    }
    if (tid == 0) {
        g.count_ws[b] = running;
        if (g.counts) g.counts[b] = running;
    }
}

// ---------------------------------------------------------------- normalise and select

__global__ __launch_bounds__(kLanes) void cmvn_select_kernel(const CmvnArgs g) {
    extern __shared__ float staged[];                 // [rows, nc]: rows r0 .. r0 + rows - 1 of the group's channels
    __shared__ int dest[kTileMax];                    // a frame's output row; -1 - row: a row of zeros
    __shared__ unsigned long long bits[kWaves];       // the mask of the tile's chunk
    const int tid = threadIdx.x;
    int64_t blk = blockIdx.x;
    const int grp = (int)(blk % g.n_groups);
    blk /= g.n_groups;
    const int tile = (int)(blk % g.n_tiles), b = (int)(blk / g.n_tiles);
    const int L = utt_len(g.lengths, b, g.T);
    const int t0 = tile * g.tile;
    const int frames = (t0 + g.tile < g.T ? t0 + g.tile : g.T) - t0;      // of the tile, 1 .. g.tile
    const int c0 = grp * g.group;
    const int nc = g.group < g.C - c0 ? g.group : g.C - c0;
    const float* xb = g.x + (int64_t)b * g.us + c0;
    float* yb = g.y + (int64_t)b * g.yus + c0;

    if (g.mask) {
        const int chunk = t0 / kLanes, cs = chunk * kLanes;               // (a tile lies inside one chunk)
        const int t = cs + tid;
        const bool v = t < L && g.mask[(int64_t)b * g.ms + t] != 0;
        const unsigned long long m = __ballot(v);
        if ((tid & 63) == 0) bits[tid >> 6] = m;
        __syncthreads();
        if (tid < frames) {
            const int ft = t0 + tid, k = ft - cs;
            int before = g.prefix[(int64_t)b * chunks(g.T) + chunk];
#pragma unroll
            for (int w = 0; w < kWaves; ++w)
                if (w < (k >> 6)) before += __popcll(bits[w]);
            const unsigned long long word = bits[k >> 6];
            before += __popcll(word & ((1ull << (k & 63)) - 1ull));
            int row = ((word >> (k & 63)) & 1ull) ? before : g.count[b] + (ft - before);
            row = row < 0 ? 0 : (row > g.T - 1 ? g.T - 1 : row);
            dest[tid] = ((word >> (k & 63)) & 1ull) ? row : -1 - row;
        }
        if (tile == 0 && grp == 0 && tid == 0 && g.new_lengths) g.new_lengths[b] = g.count[b];
    } else {
        if (tid < frames) {
            const int ft = t0 + tid;
            dest[tid] = ft < L ? ft : -1 - ft;
        }
        if (tile == 0 && grp == 0 && tid == 0 && g.new_lengths) g.new_lengths[b] = L;
    }

    // the rows the tile's frames below L read: from the first frame's window to the last one's
    int r0 = 0, rows = 0;
    if (t0 < L) {
        const int last = (t0 + frames < L ? t0 + frames : L) - 1;
        int r1;
        if (g.normalise) {
            int lo, hi;
            window(t0, L, g.cmn_window, g.min_window, g.center, &r0, &hi);
            window(last, L, g.cmn_window, g.min_window, g.center, &lo, &r1);
        } else {
            r0 = t0;
            r1 = last + 1;
        }
        rows = r1 - r0 < g.rows_cap ? r1 - r0 : g.rows_cap;
        for (int idx = tid; idx < rows * nc; idx += kLanes) {
            const int r = idx / nc, c = idx - r * nc;
            staged[idx] = xb[(int64_t)(r0 + r) * g.rs + c];
        }
    }
    __syncthreads();

    // (channel, run of frames) items: a run's first frame sums its window, the following ones slide it
    const int runs = (frames + g.run - 1) / g.run;
    for (int item = tid; item < runs * nc; item += kLanes) {
        const int s = item / nc, c = item - s * nc;
        const int f0 = s * g.run, f1 = f0 + g.run < frames ? f0 + g.run : frames;
        int cur_lo = 0, cur_hi = 0;                   // the window the sums hold
        double sum = 0.0, sq = 0.0;
        for (int f = f0; f < f1; ++f) {
            const int d = dest[f], ft = t0 + f;
            if (ft >= L) {                            // (d < 0: the frame is unvoiced or past the length)
                yb[(int64_t)(-1 - d) * g.yrs + c] = 0.0f;
                continue;
            }
            float v;
            if (!g.normalise) {
                v = staged[(ft - r0) * nc + c];
            } else {
                int lo, hi;
                window(ft, L, g.cmn_window, g.min_window, g.center, &lo, &hi);
                lo = lo < r0 ? r0 : lo;               // (both hold already: the window function is monotone in t)
                hi = hi > r0 + rows ? r0 + rows : hi;
                const float* col = staged + c;        // col[(r - r0) * nc]: row r of the utterance
                if (f == f0) {
                    sum = 0.0;
                    sq = 0.0;
                    cur_lo = cur_hi = lo;
                }
                if (g.norm_vars) {
                    for (int r = cur_hi; r < hi; ++r) {
                        const double a = (double)col[(r - r0) * nc];
                        sum = sum + a;
                        sq = sq + a * a;
                    }
                    for (int r = cur_lo; r < lo; ++r) {
                        const double a = (double)col[(r - r0) * nc];
                        sum = sum - a;
                        sq = sq - a * a;
                    }
                } else {
#pragma unroll 4
                    for (int r = cur_hi; r < hi; ++r) sum = sum + (double)col[(r - r0) * nc];
                    for (int r = cur_lo; r < lo; ++r) sum = sum - (double)col[(r - r0) * nc];
                }
                cur_lo = lo;
                cur_hi = hi;
                const int n = hi - lo;
                const double xd = (double)col[(ft - r0) * nc];
                const double mean = sum / (double)n;
                if (!g.norm_vars) {
                    v = (float)(xd - mean);
                } else {
                    const double mean2 = mean * mean;
                    double var = sq / (double)n - mean2;
                    var = var < 1e-10 ? 1e-10 : var;  // (a NaN variance stays NaN)
                    v = n == 1 ? 0.0f : (float)((xd - mean) * (1.0 / sqrt(var)));
                }
            }
            if (d < 0) yb[(int64_t)(-1 - d) * g.yrs + c] = 0.0f;
            else yb[(int64_t)d * g.yrs + c] = v;
        }
    }
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_verr;

struct Shape {
    const float* x;
    int32_t B, T, C;
    int64_t rs, us;
    const int32_t* lengths;
};

int check_decide(const Shape& s, const xvec_vad_options* vad, const uint8_t* mask, int64_t mask_stride, const int32_t* counts) {
    Refusal why;
    if (vad_plan::check_shape(s.B, s.T, s.C, s.rs, s.us, "x:", why) || vad_plan::check_vad(vad, s.C, why) ||
        vad_plan::check_mask_stride(mask_stride, s.T, why))
        return g_verr.refused(XVEC_ERR_ARG, why);
    if (!s.x || !mask || !counts) return g_verr.fail(XVEC_ERR_ARG, "null pointer: x / mask / counts");
    return XVEC_OK;
}

int check_normalise(const Shape& s, const xvec_cmvn_options* cmvn, const float* y, int64_t yrs, int64_t yus, vad_plan::Tile* tile) {
    Refusal why;
    if (vad_plan::check_shape(s.B, s.T, s.C, s.rs, s.us, "x:", why) || vad_plan::check_shape(s.B, s.T, s.C, yrs, yus, "y:", why) ||
        vad_plan::check_cmvn(cmvn, why))
        return g_verr.refused(XVEC_ERR_ARG, why);
    if (!s.x || !y) return g_verr.fail(XVEC_ERR_ARG, "null pointer: x / y");
    if (vad_plan::plan_tile(s.C, vad_plan::span(cmvn), tile))
        return g_verr.fail(XVEC_ERR_ARG, "no tile of C = %d channels fits the LDS budget at this window", s.C);
    if (vad_plan::grid_blocks(s.B, s.T, s.C, *tile) > 0x7fffffffLL)
        return g_verr.fail(XVEC_ERR_TOO_LARGE, "B = %d utterances of T = %d frames are more than 2^31 - 1 blocks", s.B, s.T);
    return XVEC_OK;
}

VadArgs decide_args(const Shape& s, const xvec_vad_options& vad, uint8_t* mask, int64_t mask_stride, int32_t* counts, double* thr) {
    VadArgs g{};
    g.x = s.x;
    g.B = s.B;
    g.T = s.T;
    g.C = s.C;
    g.rs = s.rs;
    g.us = s.us;
    g.lengths = s.lengths;
    g.thr0 = vad.energy_threshold;
    g.scale = vad.energy_mean_scale;
    g.prop = vad.proportion_threshold;
    g.ctx = vad.frames_context < s.T ? vad.frames_context : s.T;      // a wider context reaches no further frame
    g.col = vad.energy_col;
    g.mask = mask;
    g.ms = mask_stride;
    g.counts = counts;
    g.thr = thr;
    return g;
}

int launch_cmvn(const Shape& s, const xvec_cmvn_options* cmvn, const vad_plan::Tile& tile, const uint8_t* mask, int64_t mask_stride,
                const int* prefix, const int* count, float* y, int64_t yrs, int64_t yus, int32_t* new_lengths, hipStream_t stream) {
    CmvnArgs g{};
    g.x = s.x;
    g.B = s.B;
    g.T = s.T;
    g.C = s.C;
    g.rs = s.rs;
    g.us = s.us;
    g.lengths = s.lengths;
    g.normalise = cmvn ? 1 : 0;
    if (cmvn) {
        g.cmn_window = cmvn->cmn_window;
        g.min_window = cmvn->min_window;
        g.center = cmvn->center ? 1 : 0;
        g.norm_vars = cmvn->norm_vars ? 1 : 0;
    }
    g.mask = mask;
    g.ms = mask_stride;
    g.prefix = prefix;
    g.count = count;
    g.y = y;
    g.yrs = yrs;
    g.yus = yus;
    g.new_lengths = new_lengths;
    g.tile = tile.frames;
    g.group = tile.channels;
    g.run = tile.run;
    g.rows_cap = tile.rows < s.T ? tile.rows : s.T;                   // no window reaches past the utterance
    g.n_tiles = (s.T + tile.frames - 1) / tile.frames;
    g.n_groups = (s.C + tile.channels - 1) / tile.channels;
    const size_t lds = (size_t)g.rows_cap * tile.channels * sizeof(float);
    cmvn_select_kernel<<<(unsigned)vad_plan::grid_blocks(s.B, s.T, s.C, tile), kLanes, lds, stream>>>(g);
    return g_verr.launch_ok("cmvn_select_kernel");
}

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_vad_last_error(void) { return g_verr.c_str(); }

size_t xvec_vad_workspace_bytes(int32_t B, int32_t T) { return vad_plan::make_layout(B, T).total; }

int xvec_vad_energy(const float* x, int32_t B, int32_t T, int32_t C, int64_t row_stride, int64_t utt_stride,
                    const int32_t* lengths, const xvec_vad_options* vad, uint8_t* mask, int64_t mask_stride, int32_t* counts,
                    double* thr, xvec_stream stream) {
    const Shape s{x, B, T, C, row_stride, utt_stride, lengths};
    int rc;
    if ((rc = check_decide(s, vad, mask, mask_stride, counts))) return rc;
    const VadArgs g = decide_args(s, *vad, mask, mask_stride, counts, thr);
    vad_decide_kernel<<<(unsigned)B, kLanes, 0, static_cast<hipStream_t>(stream)>>>(g);
    return g_verr.launch_ok("vad_decide_kernel");
}

int xvec_cmvn_sliding(const float* x, int32_t B, int32_t T, int32_t C, int64_t row_stride, int64_t utt_stride,
                      const int32_t* lengths, const xvec_cmvn_options* cmvn, const uint8_t* mask, int64_t mask_stride, float* y,
                      int64_t y_row_stride, int64_t y_utt_stride, int32_t* new_lengths, void* workspace, size_t workspace_bytes,
                      xvec_stream stream) {
    const Shape s{x, B, T, C, row_stride, utt_stride, lengths};
    vad_plan::Tile tile{};
    int rc;
    if ((rc = check_normalise(s, cmvn, y, y_row_stride, y_utt_stride, &tile))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!mask) return launch_cmvn(s, cmvn, tile, nullptr, 0, nullptr, nullptr, y, y_row_stride, y_utt_stride, new_lengths, st);
    Refusal why;
    if (vad_plan::check_mask_stride(mask_stride, T, why)) return g_verr.refused(XVEC_ERR_ARG, why);
    if (!new_lengths) return g_verr.fail(XVEC_ERR_ARG, "null pointer: new_lengths (optional only without a mask)");
    const vad_plan::Layout l = vad_plan::make_layout(B, T);
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, l.total, g_verr))) return rc;
    VadArgs g{};
    g.B = B;
    g.T = T;
    g.lengths = lengths;
    g.mask_in = mask;
    g.ms = mask_stride;
    g.prefix = part<int>(workspace, l.prefix);
    g.count_ws = part<int>(workspace, l.count);
    vad_count_kernel<<<(unsigned)B, kLanes, 0, st>>>(g);
    if ((rc = g_verr.launch_ok("vad_count_kernel"))) return rc;
    return launch_cmvn(s, cmvn, tile, mask, mask_stride, g.prefix, g.count_ws, y, y_row_stride, y_utt_stride, new_lengths, st);
}

int xvec_vad_cmvn(const float* x, int32_t B, int32_t T, int32_t C, int64_t row_stride, int64_t utt_stride, const int32_t* lengths,
                  const xvec_vad_options* vad, const xvec_cmvn_options* cmvn, int32_t select, uint8_t* mask, int64_t mask_stride,
                  int32_t* counts, double* thr, float* y, int64_t y_row_stride, int64_t y_utt_stride, int32_t* new_lengths,
                  void* workspace, size_t workspace_bytes, xvec_stream stream) {
    const Shape s{x, B, T, C, row_stride, utt_stride, lengths};
    vad_plan::Tile tile{};
    int rc;
    if ((rc = check_decide(s, vad, mask, mask_stride, counts))) return rc;
    if ((rc = check_normalise(s, cmvn, y, y_row_stride, y_utt_stride, &tile))) return rc;
    const vad_plan::Layout l = vad_plan::make_layout(B, T);
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, l.total, g_verr))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    VadArgs g = decide_args(s, *vad, mask, mask_stride, counts, thr);
    g.prefix = part<int>(workspace, l.prefix);
    g.count_ws = part<int>(workspace, l.count);
    vad_decide_kernel<<<(unsigned)B, kLanes, 0, st>>>(g);
    if ((rc = g_verr.launch_ok("vad_decide_kernel"))) return rc;
    if (!select) return launch_cmvn(s, cmvn, tile, nullptr, 0, nullptr, nullptr, y, y_row_stride, y_utt_stride, new_lengths, st);
    return launch_cmvn(s, cmvn, tile, mask, mask_stride, g.prefix, g.count_ws, y, y_row_stride, y_utt_stride, new_lengths, st);
}

}  // extern "C"
