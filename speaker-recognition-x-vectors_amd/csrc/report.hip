// Trial report: the trial map, the range of the score matrix, the six TensorBoard images and the DET curve.
//   reference: plda_score_stat.py:132-192 (the image half of plot_images)
// C ABI, the definitions and the deviations: include/xvec_report.h.  Plan, checks and the shared host/device rules: report_plan.h.
// The trial reader, the inverse of the score key and the block scans, counts and extremes: trial_device.h, shared with eval.hip and
// calib.hip, so that the DET curve leaves out the trials the sort leaves out.
//   trial_map  memset, then one thread per trial: a 32-bit OR atomic on the aligned word that holds the cell's byte
//   range      tiles of one row x 1024 columns, block partials (min, max, count of non-finite cells) -> one block
//   images     a block stages a tile of cells in LDS (the normalised value and six flag bits of every cell, consecutive lanes
//              on consecutive cells), then writes every selected plane from there: per row of the tile the aligned 16-byte
//              pieces with vector stores, the ragged ends one element per lane; the gap columns by the tiles of the last column
//   det        prepare (count NaN / bad trials; all pairs: the cells as a trial list) -> xvec_eval_sorted_keys -> sums (targets,
//              kept trials, run ends per block) -> scan (one block) -> points; with a grid: keep flags per block -> scan ->
//              compaction; -> header
// Only integer counts and ORs go through atomics; min / max and the scans have the one order the header states.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "../../include/xvec_eval.h"
#include "../../include/xvec_hip.h"
#include "../../include/xvec_report.h"
#include "host_support.h"
#include "report_plan.h"
#include "trial_device.h"

// Every operation rounds on its own: (S - mn) / (mx - mn) and K * S are numpy's results bit for bit.
#pragma clang fp contract(off)

namespace xvec {
namespace {

using namespace report_plan;
using namespace trial_device;      // the trial reader (as eval.hip gathers the trials), key_score, the block primitives

constexpr int kWaves = kThreads / 64;

// flag bits of a staged cell
constexpr uint32_t kP = 1, kNg = 2, kGeE = 4, kLtE = 8, kGeM = 16, kLtM = 32;
// what a plane holds
enum { kModeZero = 0, kModeCount = 1, kModeValue = 2, kModeOne = 3 };

// ---------------------------------------------------------------- trial map

__global__ __launch_bounds__(kThreads) void report_map_kernel(const int32_t* __restrict__ row_idx,
                                                              const int32_t* __restrict__ col_idx,
                                                              const uint8_t* __restrict__ is_target, int64_t n, int64_t n_rows,
                                                              int64_t n_cols, uint8_t* map, int64_t ld_map,
                                                              unsigned long long* n_bad) {
    __shared__ uint32_t s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t < n) {
        const int64_t r = row_idx[t], c = col_idx[t];
        if (r < 0 || r >= n_rows || c < 0 || c >= n_cols) {
            atomicAdd(&s_bad, 1u);
        } else {
            const uint64_t byte = (uint64_t)(r * ld_map + c);          // inside [0, n_rows * ld_map): the word is too (ld_map % 4 == 0)
            uint32_t* word = reinterpret_cast<uint32_t*>(map + (byte & ~(uint64_t)3));
            atomicOr(word, (is_target[t] ? kP : kNg) << (8 * (uint32_t)(byte & 3)));
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_bad && n_bad) atomicAdd(n_bad, (unsigned long long)s_bad);
}

// ---------------------------------------------------------------- range

// part[3 b ..]: minimum, maximum, count (as int64 bits) of block b
__global__ __launch_bounds__(kThreads) void report_range_kernel(const double* __restrict__ s, int64_t ld, int64_t n_cols,
                                                                int64_t col_tiles, int64_t tiles, double* __restrict__ part) {
    __shared__ double wbuf[kWaves];
    __shared__ long long wcnt[kWaves];
    double mn = std::numeric_limits<double>::infinity(), mx = -std::numeric_limits<double>::infinity();
    long long bad = 0;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row = tile / col_tiles, c0 = (tile - row * col_tiles) * kRangeTile;
#pragma unroll
        for (int k = 0; k < kRangeTile / kThreads; ++k) {
            const int64_t c = c0 + k * kThreads + threadIdx.x;
            if (c < n_cols) {
                const double v = s[row * ld + c];
                if (isfinite(v)) {
                    mn = fmin(mn, v);
                    mx = fmax(mx, v);
                } else {
                    ++bad;
                }
            }
        }
    }
    mn = block_extreme<true>(mn, wbuf);
    mx = block_extreme<false>(mx, wbuf);
    const long long total = block_count(bad, wcnt);
    if (threadIdx.x == 0) {
        part[3 * (size_t)blockIdx.x] = mn;
        part[3 * (size_t)blockIdx.x + 1] = mx;
        reinterpret_cast<long long*>(part)[3 * (size_t)blockIdx.x + 2] = total;
    }
}

__global__ __launch_bounds__(kThreads) void report_range_final_kernel(const double* __restrict__ part, int blocks,
                                                                      xvec_report_range_result* out) {
    __shared__ double wbuf[kWaves];
    __shared__ long long wcnt[kWaves];
    double mn = std::numeric_limits<double>::infinity(), mx = -std::numeric_limits<double>::infinity();
    long long bad = 0;
    for (int b = threadIdx.x; b < blocks; b += kThreads) {
        mn = fmin(mn, part[3 * (size_t)b]);
        mx = fmax(mx, part[3 * (size_t)b + 1]);
        bad += reinterpret_cast<const long long*>(part)[3 * (size_t)b + 2];
    }
    mn = block_extreme<true>(mn, wbuf);
    mx = block_extreme<false>(mx, wbuf);
    const long long total = block_count(bad, wcnt);
    if (threadIdx.x == 0) {
        out->min = mn;
        out->max = mx;
        out->n_nonfinite = total;
    }
}

// ---------------------------------------------------------------- images

// One plane of one panel: element (row, j) of the panel lies at base + (row * width + off + j) elements.
struct Plane {
    uint64_t base;             // the channel's first element (an address)
    int64_t width, off;
    uint32_t need;             // flag bits a cell must have
    uint32_t mode;             // kMode*
};

struct ImageArgs {
    const double* s;
    const uint8_t* map;
    const xvec_report_range_result* range;
    int64_t ld, ld_map, n_rows, n_cols;
    double th_e, th_m;
    int64_t tc, tr, col_tiles;
    int32_t n_planes, n_gaps;
    uint64_t gap_base[3];      // the wide images selected (their first element)
    Plane planes[kMaxPlanes];
};

__device__ __forceinline__ uint8_t to_u8(float v) {      // trunc(clamp(v * 255, 0, 255)), NaN -> 0
    const float x = v * 255.0f;
    if (!(x == x)) return 0;
    return (uint8_t)(x < 0.0f ? 0.0f : x > 255.0f ? 255.0f : x);
}

// The staged tile in LDS: per cell the value as the output type and the flag byte.  uint8: both in one 16-bit word, so that a
// lane that builds a 16-byte piece reads 16 words, not 32 bytes.
template <typename T>
struct Stage;
template <>
struct Stage<float> {
    float v[kTile];
    uint8_t f[kTile];
    __device__ __forceinline__ void put(int e, float value, uint32_t flags) {
        v[e] = value;
        f[e] = (uint8_t)flags;
    }
    __device__ __forceinline__ float get(int e, uint32_t* flags) const {
        *flags = f[e];
        return v[e];
    }
};
template <>
struct Stage<uint8_t> {
    uint16_t c[kTile];
    __device__ __forceinline__ void put(int e, float value, uint32_t flags) { c[e] = (uint16_t)(to_u8(value) | (flags << 8)); }
    __device__ __forceinline__ uint8_t get(int e, uint32_t* flags) const {
        const uint32_t w = c[e];
        *flags = w >> 8;
        return (uint8_t)w;
    }
};

// The element of a plane behind a staged cell (value v, flags f).
template <typename T>
__device__ __forceinline__ T plane_value(uint32_t mode, uint32_t need, T v, uint32_t f) {
    const bool on = (f & need) == need;
    if (sizeof(T) == 1) {
        if (mode == kModeValue) return on ? v : (T)0;
        return on && mode != kModeZero ? (T)255 : (T)0;
    }
    if (mode == kModeValue) return on ? v : (T)((float)v * 0.0f);            // v * 0: NaN behind a non-finite cell, as numpy
    if (mode == kModeCount) return on ? (T)(float)((f & kP) + ((f >> 1) & 1u)) : (T)0;
    return on && mode == kModeOne ? (T)1 : (T)0;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void report_images_kernel(const ImageArgs g) {
    constexpr int kEs = (int)sizeof(T), kEpc = kChunk / kEs;      // elements of a 16-byte piece
    __shared__ Stage<T> st;
    const int tid = threadIdx.x;
    const int64_t rt = blockIdx.x / g.col_tiles, ct = blockIdx.x - rt * g.col_tiles;
    const int64_t r0 = rt * g.tr, c0 = ct * g.tc;
    const int rows = (int)(g.n_rows - r0 < g.tr ? g.n_rows - r0 : g.tr);
    const int cols = (int)(g.n_cols - c0 < g.tc ? g.n_cols - c0 : g.tc);
    const int cells = rows * cols;                                // <= kTile
    const double mn = g.range->min, d = g.range->max - mn;

    for (int e = tid; e < cells; e += kThreads) {
        const int lr = e / cols, lc = e - lr * cols;
        const double S = g.s[(r0 + lr) * g.ld + c0 + lc];
        const uint32_t m = g.map[(r0 + lr) * g.ld_map + c0 + lc] & 3u;
        const uint32_t K = (m & 1u) + (m >> 1);
        uint32_t f = m;
        if (K) {
            const double cv = (double)K * S;
            if (cv >= g.th_e) f |= kGeE;
            if (cv < g.th_e) f |= kLtE;
            if (cv >= g.th_m) f |= kGeM;
            if (cv < g.th_m) f |= kLtM;
        }
        const double v = (S - mn) / d;
        st.put(e, __double2float_rn(v), f);
    }
    __syncthreads();

    const int cpi = cols / kEpc;                                  // a row of the tile holds at most that many whole aligned pieces
    for (int p = 0; p < g.n_planes; ++p) {
        const uint64_t base = g.planes[p].base;
        const int64_t width = g.planes[p].width, off = g.planes[p].off;
        const uint32_t need = g.planes[p].need, mode = g.planes[p].mode;
        // the aligned body of every row's piece: one 16-byte store per lane
        for (int u = tid; u < rows * cpi; u += kThreads) {
            const int lr = u / cpi, ch = u - lr * cpi;
            const uint64_t a = base + (uint64_t)((r0 + lr) * width + off + c0) * kEs, b = a + (uint64_t)cols * kEs;
            const Piece pc = split_piece(a, b);
            const uint64_t x = pc.body + (uint64_t)ch * kChunk;
            if (x + kChunk > pc.tail) continue;
            const int j0 = lr * cols + (int)((x - a) / kEs);
            T out[kEpc];
            if (mode == kModeZero) {
#pragma unroll
                for (int i = 0; i < kEpc; ++i) out[i] = (T)0;
            } else {
#pragma unroll
                for (int i = 0; i < kEpc; ++i) {
                    uint32_t f;
                    const T v = st.get(j0 + i, &f);
                    out[i] = plane_value<T>(mode, need, v, f);
                }
            }
            uint4 w;
            __builtin_memcpy(&w, out, sizeof(w));
            *reinterpret_cast<uint4*>(x) = w;
        }
        // the ragged ends: slots 0 .. 15 the piece in front of the body, 16 .. 31 the one behind it; one element per lane
        for (int u = tid; u < rows * 32; u += kThreads) {
            const int lr = u >> 5, e = u & 15;
            if (e >= kEpc) continue;
            const uint64_t a = base + (uint64_t)((r0 + lr) * width + off + c0) * kEs, b = a + (uint64_t)cols * kEs;
            const Piece pc = split_piece(a, b);
            uint64_t x;
            if (u & 16) {
                x = pc.tail + (uint64_t)e * kEs;
                if (x >= b) continue;
            } else {
                x = (a & ~(uint64_t)(kChunk - 1)) + (uint64_t)e * kEs;
                if (x < a || x >= pc.body) continue;
            }
            const int j = lr * cols + (int)((x - a) / kEs);
            uint32_t f;
            const T v = st.get(j, &f);
            *reinterpret_cast<T*>(x) = mode == kModeZero ? (T)0 : plane_value<T>(mode, need, v, f);
        }
    }
    // the gap of the wide images: the tiles that hold the last column write it for their rows
    if (c0 + cols == g.n_cols) {
        const int64_t width = wide_cols(g.n_cols);
        for (int q = 0; q < g.n_gaps; ++q)
            for (int u = tid; u < rows * 3 * kGap; u += kThreads) {
                const int lr = u / (3 * kGap), rest = u - lr * (3 * kGap), ch = rest / kGap, k = rest - ch * kGap;
                const uint64_t x = g.gap_base[q] + (uint64_t)(((int64_t)ch * g.n_rows + r0 + lr) * width + g.n_cols + k) * kEs;
                *reinterpret_cast<T*>(x) = sizeof(T) == 1 ? (T)255 : (T)1;
            }
    }
}

// ---------------------------------------------------------------- DET curve

struct DetState {              // in the state slot of the workspace
    unsigned long long n_nan, n_bad;
    long long P, m, n_full, n_kept;
};
static_assert(sizeof(DetState) <= 256, "the state's slot in the workspace");

struct DetTrials {
    TrialArgs trials;
    int32_t* row_out;          // all pairs only: the cells as a trial list
    int32_t* col_out;
    uint8_t* tgt_out;
};

// Counts the trials the sort will leave out; all pairs: writes the cells as a trial list (row -1 for a skipped diagonal cell:
// xvec_eval_sorted_keys leaves an index outside the matrix out and never reads its cell).
template <bool ALL_PAIRS>
__global__ __launch_bounds__(kThreads) void report_det_prepare_kernel(const DetTrials g, DetState* st) {
    __shared__ uint32_t cnt[2];
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t < g.trials.n) {
        const Trial tr = read_trial<ALL_PAIRS>(g.trials, t);
        if (ALL_PAIRS) {
            g.row_out[t] = tr.what == kSkip ? -1 : (int32_t)tr.row;
            g.col_out[t] = (int32_t)tr.col;
            g.tgt_out[t] = tr.target ? 1 : 0;
        }
        if (tr.what == kNan) atomicAdd(&cnt[0], 1u);
        if (tr.what == kBad) atomicAdd(&cnt[1], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0 && cnt[0]) atomicAdd(&st->n_nan, (unsigned long long)cnt[0]);
    if (threadIdx.x == 1 && cnt[1]) atomicAdd(&st->n_bad, (unsigned long long)cnt[1]);
}

// What a thread needs of its kDetItems consecutive sorted trials: the target bit, whether a trial is kept, whether it is the
// last of its run of equal keys.
struct DetItems {
    uint32_t key[kDetItems];
    uint32_t tar, kept, ends;      // bit masks over the items
};

__device__ __forceinline__ DetItems det_load(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ bits, int64_t n,
                                             int64_t base) {
    DetItems it;
    it.tar = it.kept = it.ends = 0;
    uint32_t next = base + kDetItems < n ? keys[base + kDetItems] : 0u;
#pragma unroll
    for (int k = kDetItems - 1; k >= 0; --k) {
        const bool in = base + k < n;
        const uint32_t key = in ? keys[base + k] : 0u;
        const uint8_t bit = in ? bits[base + k] : kBitVoid;
        it.key[k] = key;
        const bool following = base + k + 1 < n;
        if (bit != kBitVoid) {
            it.kept |= 1u << k;
            if (bit == 1) it.tar |= 1u << k;
            if (!following || next != key) it.ends |= 1u << k;      // a void trial's key differs from every kept one
        }
        next = key;
    }
    return it;
}

// sums[0][b] targets, sums[1][b] kept trials, sums[2][b] run ends among the kDetTile trials of block b
__global__ __launch_bounds__(kThreads) void report_det_sums_kernel(const uint32_t* __restrict__ keys,
                                                                   const uint8_t* __restrict__ bits, int64_t n,
                                                                   uint32_t* __restrict__ sums, int64_t blocks) {
    __shared__ uint32_t wtot[kWaves];
    const DetItems it = det_load(keys, bits, n, (int64_t)blockIdx.x * kDetTile + (int64_t)threadIdx.x * kDetItems);
    uint32_t t0, t1, t2;
    block_excl_scan((uint32_t)__popc(it.tar), wtot, &t0);
    block_excl_scan((uint32_t)__popc(it.kept), wtot, &t1);
    block_excl_scan((uint32_t)__popc(it.ends), wtot, &t2);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = t0;
        sums[blocks + blockIdx.x] = t1;
        sums[2 * blocks + blockIdx.x] = t2;
    }
}

// One block, chunks of kThreads blocks in rising order: sums[0] and sums[2] <- their exclusive scans; the totals.
__global__ __launch_bounds__(kThreads) void report_det_scan_kernel(uint32_t* __restrict__ sums, int64_t blocks, DetState* st) {
    __shared__ uint32_t wtot[kWaves];
    uint32_t* ends = sums + 2 * blocks;
    const uint32_t targets = block_scan_array(sums, sums, blocks, wtot);
    const uint32_t kept = block_scan_array(sums + blocks, nullptr, blocks, wtot);      // at most n < 2^31
    const uint32_t n_ends = block_scan_array(ends, ends, blocks, wtot);
    if (threadIdx.x == 0) {
        st->P = (long long)targets;
        st->m = (long long)kept;
        st->n_full = (long long)n_ends;
        st->n_kept = (long long)n_ends;
    }
}

struct DetOut {
    float* thr;
    int64_t* tp;
    int64_t* nn;
    int64_t capacity;
    float* pt_thr;             // the unthinned points (grid > 0)
    int32_t* pt_tp;
    int32_t* pt_nn;
};

// Point k of the run that ends at sorted trial i: (score, targets among the trials 0 .. i, the other i + 1 - targets).
template <bool THIN>
__global__ __launch_bounds__(kThreads) void report_det_points_kernel(const uint32_t* __restrict__ keys,
                                                                     const uint8_t* __restrict__ bits, int64_t n,
                                                                     const uint32_t* __restrict__ sums, int64_t blocks,
                                                                     const DetOut o) {
    __shared__ uint32_t wtot[kWaves];
    const int64_t base = (int64_t)blockIdx.x * kDetTile + (int64_t)threadIdx.x * kDetItems;
    const DetItems it = det_load(keys, bits, n, base);
    int64_t tp = (int64_t)block_excl_scan((uint32_t)__popc(it.tar), wtot, nullptr) + (int64_t)sums[blockIdx.x];
    int64_t k = (int64_t)block_excl_scan((uint32_t)__popc(it.ends), wtot, nullptr) + (int64_t)sums[2 * blocks + blockIdx.x];
#pragma unroll
    for (int q = 0; q < kDetItems; ++q) {
        tp += (it.tar >> q) & 1u;
        if ((it.ends >> q) & 1u) {
            const int64_t nn = base + q + 1 - tp;      // the kept trials are the sorted prefix
            if (THIN) {
                o.pt_thr[k] = key_score(it.key[q]);
                o.pt_tp[k] = (int32_t)tp;
                o.pt_nn[k] = (int32_t)nn;
            } else if (k < o.capacity) {
                o.thr[k] = key_score(it.key[q]);
                o.tp[k] = tp;
                o.nn[k] = nn;
            }
            ++k;
        }
    }
}

// The keep flags of a thread's kDetItems consecutive points (a bit mask).
__device__ __forceinline__ uint32_t det_keep_mask(const DetOut& o, const DetState* st, int64_t grid, int64_t base) {
    const int64_t n_full = st->n_full, P = st->P, N = st->m - st->P;
    uint32_t mask = 0;
    int64_t tp_prev = 0, nn_prev = 0;
    if (base > 0 && base <= n_full) {
        tp_prev = o.pt_tp[base - 1];
        nn_prev = o.pt_nn[base - 1];
    }
#pragma unroll
    for (int q = 0; q < kDetItems; ++q) {
        const int64_t k = base + q;
        if (k < n_full) {
            const int64_t tp = o.pt_tp[k], nn = o.pt_nn[k];
            if (det_keep(tp, nn, tp_prev, nn_prev, P, N, grid, k == 0, k + 1 == n_full)) mask |= 1u << q;
            tp_prev = tp;
            nn_prev = nn;
        }
    }
    return mask;
}

__global__ __launch_bounds__(kThreads) void report_det_keep_kernel(const DetOut o, const DetState* st, int64_t grid,
                                                                   uint32_t* __restrict__ keep_sums) {
    __shared__ uint32_t wtot[kWaves];
    const uint32_t mask = det_keep_mask(o, st, grid, (int64_t)blockIdx.x * kDetTile + (int64_t)threadIdx.x * kDetItems);
    uint32_t total;
    block_excl_scan((uint32_t)__popc(mask), wtot, &total);
    if (threadIdx.x == 0) keep_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void report_det_keep_scan_kernel(uint32_t* __restrict__ keep_sums, int64_t blocks,
                                                                        DetState* st) {
    __shared__ uint32_t wtot[kWaves];
    const uint32_t total = block_scan_array(keep_sums, keep_sums, blocks, wtot);
    if (threadIdx.x == 0) st->n_kept = (long long)total;
}

__global__ __launch_bounds__(kThreads) void report_det_compact_kernel(const DetOut o, const DetState* st, int64_t grid,
                                                                      const uint32_t* __restrict__ keep_sums) {
    __shared__ uint32_t wtot[kWaves];
    const int64_t base = (int64_t)blockIdx.x * kDetTile + (int64_t)threadIdx.x * kDetItems;
    const uint32_t mask = det_keep_mask(o, st, grid, base);
    int64_t at = (int64_t)block_excl_scan((uint32_t)__popc(mask), wtot, nullptr) + (int64_t)keep_sums[blockIdx.x];
#pragma unroll
    for (int q = 0; q < kDetItems; ++q)
        if ((mask >> q) & 1u) {
            if (at < o.capacity) {
                o.thr[at] = o.pt_thr[base + q];
                o.tp[at] = o.pt_tp[base + q];
                o.nn[at] = o.pt_nn[base + q];
            }
            ++at;
        }
}

__global__ void report_det_header_kernel(const DetState* st, int all_pairs, xvec_report_det_header* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    xvec_report_det_header h;
    h.n_points = st->n_kept;
    h.n_target = st->P;
    h.n_nontarget = st->m - st->P;
    h.n_nan = (int64_t)st->n_nan;
    h.n_bad_index = all_pairs ? 0 : (int64_t)st->n_bad;
    *out = h;
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_rerr;

int refused(const Refusal& why, bool too_large, const char* call) {
    return g_rerr.refused(too_large ? XVEC_ERR_TOO_LARGE : XVEC_ERR_ARG, why, call);
}

void add_plane(ImageArgs& g, uint64_t image, int es, int ch, int64_t width, int64_t off, uint32_t need, uint32_t mode) {
    Plane& p = g.planes[g.n_planes++];
    p.base = image + (uint64_t)ch * (uint64_t)g.n_rows * (uint64_t)width * (uint64_t)es;
    p.width = width;
    p.off = off;
    p.need = need;
    p.mode = mode;
}

int det(const TrialArgs& trials, bool all_pairs, int64_t grid, xvec_report_det_header* header, float* thr, int64_t* tp,
        int64_t* nn, int64_t capacity, void* workspace, size_t workspace_bytes, xvec_stream stream, const char* call) {
    Refusal why;
    if (check_curve(grid, header, thr, tp, nn, capacity, why)) return refused(why, false, call);
    const int64_t n = trials.n;
    const size_t eval_bytes = xvec_eval_workspace_bytes(n);
    const Layout lay = make_layout(n, eval_bytes);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, lay.total, g_rerr))) return rc;
    char* base = static_cast<char*>(workspace);
    DetState* st = reinterpret_cast<DetState*>(base + lay.state);
    uint32_t* keys = reinterpret_cast<uint32_t*>(base + lay.keys);
    uint8_t* bits = reinterpret_cast<uint8_t*>(base + lay.bits);
    uint32_t* sums = reinterpret_cast<uint32_t*>(base + lay.sums);
    uint32_t* keep_sums = reinterpret_cast<uint32_t*>(base + lay.keep_sums);
    const DetTrials g{trials, reinterpret_cast<int32_t*>(base + lay.row), reinterpret_cast<int32_t*>(base + lay.col),
                      reinterpret_cast<uint8_t*>(base + lay.tgt)};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = hipMemsetAsync(st, 0, 256, s);
    if (e != hipSuccess) return g_rerr.fail(XVEC_ERR_HIP, "%s: clearing the counters failed: %s", call, hipGetErrorString(e));
    const unsigned per_trial = (unsigned)((n + kThreads - 1) / kThreads);
    if (all_pairs) report_det_prepare_kernel<true><<<per_trial, kThreads, 0, s>>>(g, st);
    else report_det_prepare_kernel<false><<<per_trial, kThreads, 0, s>>>(g, st);
    if ((rc = g_rerr.launch_ok("report_det_prepare_kernel"))) return rc;
    // the sort takes a trial list: the one given, or the one the kernel has just written
    if ((rc = xvec_eval_sorted_keys(trials.scores, trials.ld, trials.n_rows, trials.n_cols, all_pairs ? g.row_out : trials.a,
                                    all_pairs ? g.col_out : trials.b, all_pairs ? g.tgt_out : trials.is_target, n, keys, bits,
                                    base + lay.eval, eval_bytes, stream)))
        return g_rerr.fail(rc, "%s: xvec_eval_sorted_keys: %s", call, xvec_eval_last_error());
    const unsigned blocks = (unsigned)lay.blocks;
    report_det_sums_kernel<<<blocks, kThreads, 0, s>>>(keys, bits, n, sums, lay.blocks);
    if ((rc = g_rerr.launch_ok("report_det_sums_kernel"))) return rc;
    report_det_scan_kernel<<<1, kThreads, 0, s>>>(sums, lay.blocks, st);
    if ((rc = g_rerr.launch_ok("report_det_scan_kernel"))) return rc;
    DetOut o{thr, tp, nn, capacity, reinterpret_cast<float*>(base + lay.pt_thr), reinterpret_cast<int32_t*>(base + lay.pt_tp),
             reinterpret_cast<int32_t*>(base + lay.pt_nn)};
    if (grid == 0) {
        report_det_points_kernel<false><<<blocks, kThreads, 0, s>>>(keys, bits, n, sums, lay.blocks, o);
        if ((rc = g_rerr.launch_ok("report_det_points_kernel"))) return rc;
    } else {
        report_det_points_kernel<true><<<blocks, kThreads, 0, s>>>(keys, bits, n, sums, lay.blocks, o);
        if ((rc = g_rerr.launch_ok("report_det_points_kernel"))) return rc;
        report_det_keep_kernel<<<blocks, kThreads, 0, s>>>(o, st, grid, keep_sums);
        if ((rc = g_rerr.launch_ok("report_det_keep_kernel"))) return rc;
        report_det_keep_scan_kernel<<<1, kThreads, 0, s>>>(keep_sums, lay.blocks, st);
        if ((rc = g_rerr.launch_ok("report_det_keep_scan_kernel"))) return rc;
        report_det_compact_kernel<<<blocks, kThreads, 0, s>>>(o, st, grid, keep_sums);
        if ((rc = g_rerr.launch_ok("report_det_compact_kernel"))) return rc;
    }
    report_det_header_kernel<<<1, 64, 0, s>>>(st, all_pairs ? 1 : 0, header);
    return g_rerr.launch_ok("report_det_header_kernel");
}

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_report_last_error(void) { return g_rerr.c_str(); }

int xvec_report_trial_map(const int32_t* row_idx, const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials,
                          int64_t n_rows, int64_t n_cols, uint8_t* map, int64_t ld_map, int64_t* n_bad_index, xvec_stream stream) {
    const char* call = "xvec_report_trial_map";
    Refusal why;
    bool too_large;
    if (check_trial_map(row_idx, col_idx, is_target, n_trials, n_rows, n_cols, map, ld_map, why, &too_large))
        return refused(why, too_large, call);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(map, 0, (size_t)n_rows * (size_t)ld_map, s);
    if (e == hipSuccess && n_bad_index) e = hipMemsetAsync(n_bad_index, 0, sizeof(int64_t), s);
    if (e != hipSuccess) return g_rerr.fail(XVEC_ERR_HIP, "%s: clearing the map failed: %s", call, hipGetErrorString(e));
    if (n_trials == 0) return XVEC_OK;
    report_map_kernel<<<(unsigned)((n_trials + kThreads - 1) / kThreads), kThreads, 0, s>>>(
        row_idx, col_idx, is_target, n_trials, n_rows, n_cols, map, ld_map, reinterpret_cast<unsigned long long*>(n_bad_index));
    return g_rerr.launch_ok("report_map_kernel");
}

size_t xvec_report_range_workspace_bytes(void) { return range_bytes(); }

int xvec_report_range(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, xvec_report_range_result* out,
                      void* workspace, size_t workspace_bytes, xvec_stream stream) {
    const char* call = "xvec_report_range";
    Refusal why;
    if (check_matrix(scores, ld, n_rows, n_cols, why)) return refused(why, false, call);
    if (!out) return g_rerr.fail(XVEC_ERR_ARG, "%s: null pointer: out", call);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, range_bytes(), g_rerr))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t col_tiles = range_col_tiles(n_cols), blocks = range_blocks(n_rows, n_cols);
    double* part = static_cast<double*>(workspace);
    report_range_kernel<<<(unsigned)blocks, kThreads, 0, s>>>(scores, ld, n_cols, col_tiles, n_rows * col_tiles, part);
    if ((rc = g_rerr.launch_ok("report_range_kernel"))) return rc;
    report_range_final_kernel<<<1, kThreads, 0, s>>>(part, (int)blocks, out);
    return g_rerr.launch_ok("report_range_final_kernel");
}

int xvec_report_images(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const uint8_t* map, int64_t ld_map,
                       const xvec_report_range_result* range, double eer_threshold, double min_dcf_threshold, uint32_t which,
                       int32_t dtype, void* score_matrix, void* ground_truth, void* ground_truth_scores, void* prediction,
                       void* correct_prediction, void* false_prediction, xvec_stream stream) {
    const char* call = "xvec_report_images";
    void* const images[6] = {score_matrix, ground_truth, ground_truth_scores, prediction, correct_prediction, false_prediction};
    Refusal why;
    bool too_large;
    if (check_images(scores, ld, n_rows, n_cols, map, ld_map, range, which, dtype, images, why, &too_large))
        return refused(why, too_large, call);
    ImageArgs g{};
    g.s = scores;
    g.map = map;
    g.range = range;
    g.ld = ld;
    g.ld_map = ld_map;
    g.n_rows = n_rows;
    g.n_cols = n_cols;
    g.th_e = eer_threshold;
    g.th_m = min_dcf_threshold;
    g.tc = tile_cols(n_cols);
    g.tr = tile_rows(n_cols);
    g.col_tiles = col_tiles(n_cols);
    const int es = dtype == XVEC_REPORT_U8 ? 1 : 4;
    auto at = [&](int i) { return (uint64_t)reinterpret_cast<uintptr_t>(images[i]); };
    if (which & XVEC_REPORT_SCORE_MATRIX) add_plane(g, at(0), es, 0, n_cols, 0, 0, kModeValue);
    if (which & XVEC_REPORT_GROUND_TRUTH) {
        add_plane(g, at(1), es, 0, n_cols, 0, kNg, kModeOne);
        add_plane(g, at(1), es, 1, n_cols, 0, kP, kModeOne);
        add_plane(g, at(1), es, 2, n_cols, 0, 0, kModeZero);
    }
    if (which & XVEC_REPORT_GROUND_TRUTH_SCORES) {
        add_plane(g, at(2), es, 0, n_cols, 0, kNg, kModeValue);
        add_plane(g, at(2), es, 1, n_cols, 0, kP, kModeValue);
        add_plane(g, at(2), es, 2, n_cols, 0, 0, kModeZero);
    }
    // the wide images: channel 0 the rejections (of: anything, non-targets, targets), channel 1 the acceptances
    const uint32_t with0[3] = {0, kNg, kP}, with1[3] = {0, kP, kNg};
    const int64_t width = wide_cols(n_cols);
    for (int i = 0; i < 3; ++i) {
        if (!(which >> (3 + i) & 1u)) continue;
        g.gap_base[g.n_gaps++] = at(3 + i);
        for (int panel = 0; panel <= 2; panel += 2) {
            const int64_t off = panel_first(panel, n_cols);
            add_plane(g, at(3 + i), es, 0, width, off, (panel ? kLtM : kLtE) | with0[i], kModeCount);
            add_plane(g, at(3 + i), es, 1, width, off, (panel ? kGeM : kGeE) | with1[i], kModeCount);
            add_plane(g, at(3 + i), es, 2, width, off, 0, kModeZero);
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)image_tiles(n_rows, n_cols);
    if (dtype == XVEC_REPORT_U8) report_images_kernel<uint8_t><<<grid, kThreads, 0, s>>>(g);
    else report_images_kernel<float><<<grid, kThreads, 0, s>>>(g);
    return g_rerr.launch_ok("report_images_kernel");
}

size_t xvec_report_det_workspace_bytes(int64_t n_trials) {
    if (!count_ok(n_trials)) return 0;
    return make_layout(n_trials, xvec_eval_workspace_bytes(n_trials)).total;
}

int xvec_report_det(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                    const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, int64_t grid,
                    xvec_report_det_header* header, float* thr, int64_t* tp, int64_t* nn, int64_t capacity, void* workspace,
                    size_t workspace_bytes, xvec_stream stream) {
    const char* call = "xvec_report_det";
    Refusal why;
    bool too_large;
    if (check_trials(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, why, &too_large))
        return refused(why, too_large, call);
    return det(trial_args(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, false), false, grid, header, thr, tp, nn,
               capacity, workspace, workspace_bytes, stream, call);
}

int xvec_report_det_all_pairs(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_class,
                              const int32_t* col_class, int32_t skip_diagonal, int64_t grid, xvec_report_det_header* header,
                              float* thr, int64_t* tp, int64_t* nn, int64_t capacity, void* workspace, size_t workspace_bytes,
                              xvec_stream stream) {
    const char* call = "xvec_report_det_all_pairs";
    Refusal why;
    bool too_large;
    if (check_all_pairs(scores, ld, n_rows, n_cols, row_class, col_class, why, &too_large)) return refused(why, too_large, call);
    return det(trial_args(scores, ld, n_rows, n_cols, row_class, col_class, nullptr, n_rows * n_cols, skip_diagonal != 0), true, grid,
               header, thr, tp, nn, capacity, workspace, workspace_bytes, stream, call);
}

}  // extern "C"
