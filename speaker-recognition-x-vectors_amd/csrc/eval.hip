// Trial-list evaluation: EER and minDCF from scores that stay on the device.
//   reference: plda_score_stat.py:36-97 -> speechbrain 0.5.12 utils.metric_stats EER / minDCF (float32 tensors)
// C ABI and the algorithm: include/xvec_eval.h.  The score key, the trial reader and the block scan: trial_device.h; the argument
// checks: trial_plan.h (both shared with calib.hip and report.hip).  Stages, one kernel each:
//   gather + key   trial score -> fp32 (RNE) -> order-preserving 32-bit key, target bit next to it
//   sort           stable LSD radix sort, 4 passes of 8 bits: per-tile digit histogram, scan of the histograms, scatter that
//                  ranks inside the tile with wave ballots and reorders through LDS
//   prefix sum     of the target bit: per-tile counts, scan of the counts; the last phase runs inside the sweep
//   sweep          at the last element of every run of equal keys: both arg-min objectives; block partials
//   final          one block reduces the partials and writes xvec_eval_result
// Counters are integer counts (order does not matter); nothing else goes through an atomic on global memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <limits>

#include "../../include/xvec_eval.h"
#include "../../include/xvec_hip.h"
#include "host_support.h"
#include "trial_device.h"
#include "trial_plan.h"

namespace xvec {
namespace {

using namespace trial_device;

constexpr int kThreads = 256;
constexpr int kItems = 16;
constexpr int kTile = kThreads * kItems;      // elements a block owns in every stage
constexpr int kWaves = kThreads / 64;
constexpr int kRadix = 256;                   // 8-bit digits

// counters in the workspace (uint64 each)
enum { kCntNan = 0, kCntBad = 1, kCntSkipped = 2, kCntTargets = 3, kCounters = 4 };

// ---------------------------------------------------------------- stage 1: gather and key

struct GatherArgs {
    TrialArgs trials;
    uint32_t* keys;
    uint8_t* bits;
    unsigned long long* counters;
};

template <bool ALL_PAIRS>
__global__ __launch_bounds__(kThreads) void eval_gather_kernel(const GatherArgs g) {
    __shared__ uint32_t cnt[3];
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kTile;
    uint32_t n_nan = 0, n_bad = 0, n_skip = 0;
#pragma unroll 4
    for (int k = 0; k < kItems; ++k) {
        const int64_t t = base + k * kThreads + threadIdx.x;
        if (t >= g.trials.n) break;
        const Trial tr = read_trial<ALL_PAIRS>(g.trials, t);
        uint32_t key = kKeyVoid;
        uint8_t bit = kBitVoid;
        if (tr.what == kUse) {
            key = score_key(tr.score);
            bit = tr.target ? 1 : 0;
        }
        n_nan += tr.what == kNan;
        n_bad += tr.what == kBad;
        n_skip += tr.what == kSkip;
        g.keys[t] = key;
        g.bits[t] = bit;
    }
    if (n_nan) atomicAdd(&cnt[0], n_nan);
    if (n_bad) atomicAdd(&cnt[1], n_bad);
    if (n_skip) atomicAdd(&cnt[2], n_skip);
    __syncthreads();
    if (threadIdx.x < 3 && cnt[threadIdx.x])
        atomicAdd(&g.counters[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);      // kCntNan, kCntBad, kCntSkipped
}

// ---------------------------------------------------------------- stage 2: radix sort

// hist[digit * num_tiles + tile] = elements of the tile with that digit (digit-major: one scan of the whole table gives every
// (digit, tile) its first output position)
__global__ __launch_bounds__(kThreads) void eval_hist_kernel(const uint32_t* __restrict__ keys, int64_t n, int shift,
                                                             uint32_t* __restrict__ hist, int num_tiles) {
    __shared__ uint32_t h[kRadix];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kTile;
#pragma unroll 4
    for (int k = 0; k < kItems; ++k) {
        const int64_t i = base + k * kThreads + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & (kRadix - 1)], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * num_tiles + blockIdx.x] = h[threadIdx.x];
}

// In-place exclusive scan of a uint32 array of any length, three launches: chunk sums, scan of the chunk sums (one block),
// scan of every chunk with its offset.  A chunk is kTile elements.
__global__ __launch_bounds__(kThreads) void eval_scan_sums_kernel(const uint32_t* __restrict__ v, int64_t len,
                                                                  uint32_t* __restrict__ sums) {
    __shared__ uint32_t wtot[kWaves];
    const int64_t base = (int64_t)blockIdx.x * kTile;
    uint32_t s = 0;
#pragma unroll 4
    for (int k = 0; k < kItems; ++k) {
        const int64_t i = base + k * kThreads + threadIdx.x;
        if (i < len) s += v[i];
    }
    uint32_t total;
    block_excl_scan(s, wtot, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void eval_scan_top_kernel(uint32_t* __restrict__ sums, int64_t n_sums,
                                                                 unsigned long long* __restrict__ total_out) {
    __shared__ uint32_t wtot[kWaves];
    const uint32_t total = block_scan_array(sums, sums, n_sums, wtot);
    if (total_out && threadIdx.x == 0) *total_out = total;
}

__global__ __launch_bounds__(kThreads) void eval_scan_apply_kernel(uint32_t* __restrict__ v, int64_t len,
                                                                   const uint32_t* __restrict__ sums) {
    __shared__ uint32_t wtot[kWaves];
    const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
    uint32_t x[kItems], s = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        x[k] = base + k < len ? v[base + k] : 0u;
        s += x[k];
    }
    uint32_t run = block_excl_scan(s, wtot, nullptr) + sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        if (base + k < len) v[base + k] = run;
        run += x[k];
    }
}

// One pass: the tile's elements, in input order, go to offs[digit][tile] + (rank among the tile's elements of that digit).
// Wave w owns the elements [w * 1024, (w + 1) * 1024) of the tile, 64 at a time: the lanes with the same digit find each other
// with eight ballots, rank = that wave's count of the digit so far + lanes below.  The tile is then laid out in digit order in
// LDS and written from there, so that neighbouring threads write neighbouring addresses within each digit's run.
__global__ __launch_bounds__(kThreads) void eval_scatter_kernel(const uint32_t* __restrict__ kin,
                                                                const uint8_t* __restrict__ bin,
                                                                uint32_t* __restrict__ kout, uint8_t* __restrict__ bout,
                                                                int64_t n, int shift, const uint32_t* __restrict__ offs,
                                                                int num_tiles) {
    __shared__ uint32_t wcnt[kWaves][kRadix];     // per wave: running count of each digit, then the wave's base inside the digit
    __shared__ uint32_t dstart[kRadix];           // first tile-local position of each digit
    __shared__ uint32_t goff[kRadix];             // first output position of each digit of this tile
    __shared__ uint32_t wtot[kWaves];
    __shared__ uint32_t skey[kTile];
    __shared__ uint8_t sbit[kTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) wcnt[w][tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kTile;
    const int cnt = (int)std::min<int64_t>(kTile, n - base);
    const uint64_t below_mask = (1ull << lane) - 1ull;

    uint32_t key[kItems], rank[kItems];
    uint8_t bit[kItems];
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
        const int li = wave * (64 * kItems) + r * 64 + lane;
        const bool active = li < cnt;
        key[r] = active ? kin[base + li] : 0u;
        bit[r] = active ? bin[base + li] : (uint8_t)0;
        const uint32_t d = (key[r] >> shift) & (kRadix - 1);
        uint64_t peers = __ballot(active);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool set = (d >> b) & 1u;
            const uint64_t bal = __ballot(set);
            peers &= set ? bal : ~bal;
        }
        const uint32_t below = (uint32_t)__popcll(peers & below_mask);
        const uint32_t prev = active ? wcnt[wave][d] : 0u;
        __builtin_amdgcn_wave_barrier();
        if (active && below == 0) wcnt[wave][d] = prev + (uint32_t)__popcll(peers);     // the lowest lane of each digit
        __builtin_amdgcn_wave_barrier();
        rank[r] = prev + below;
    }
    __syncthreads();
    {   // thread = digit: the waves' counts -> each wave's base inside the digit; digit totals -> tile-local starts
        uint32_t run = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint32_t c = wcnt[w][tid];
            wcnt[w][tid] = run;
            run += c;
        }
        dstart[tid] = block_excl_scan(run, wtot, nullptr);
        goff[tid] = offs[(size_t)tid * num_tiles + blockIdx.x];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
        const int li = wave * (64 * kItems) + r * 64 + lane;
        if (li < cnt) {
            const uint32_t d = (key[r] >> shift) & (kRadix - 1);
            const uint32_t p = dstart[d] + wcnt[wave][d] + rank[r];
            if (p < (uint32_t)kTile) {      // always true: a bound, not a branch taken
                skey[p] = key[r];
                sbit[p] = bit[r];
            }
        }
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < kItems; ++k) {
        const int p = k * kThreads + tid;
        if (p < cnt) {
            const uint32_t kk = skey[p];
            const uint32_t d = (kk >> shift) & (kRadix - 1);
            const int64_t pos = (int64_t)goff[d] + (int64_t)(p - (int)dstart[d]);
            if (pos >= 0 && pos < n) {      // always true when offs is the scan of this pass's histogram
                kout[pos] = kk;
                bout[pos] = sbit[p];
            }
        }
    }
}

// ---------------------------------------------------------------- stage 3: target counts per tile

__global__ __launch_bounds__(kThreads) void eval_bit_sums_kernel(const uint8_t* __restrict__ bits, int64_t n,
                                                                 uint32_t* __restrict__ sums) {
    __shared__ uint32_t wtot[kWaves];
    const int64_t base = (int64_t)blockIdx.x * kTile;
    uint32_t s = 0;
#pragma unroll 4
    for (int k = 0; k < kItems; ++k) {
        const int64_t i = base + k * kThreads + threadIdx.x;
        if (i < n) s += bits[i] == 1;
    }
    uint32_t total;
    block_excl_scan(s, wtot, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// ---------------------------------------------------------------- stage 4: sweep

// A candidate threshold: objective, sorted index, targets at or below it.  Order: smaller objective, then smaller index --
// a total order, so the reduction gives the same winner whatever its shape.
struct EerCand {
    int64_t val, idx, tp;
};
struct DcfCand {
    double val;
    int64_t idx, tp;
};
__device__ __forceinline__ bool better(const EerCand& a, const EerCand& b) {
    return a.val < b.val || (a.val == b.val && a.idx < b.idx);
}
__device__ __forceinline__ bool better(const DcfCand& a, const DcfCand& b) {
    return a.val < b.val || (a.val == b.val && a.idx < b.idx);
}
constexpr int64_t kNoIdx = std::numeric_limits<int64_t>::max();

template <typename C>
__device__ __forceinline__ C block_best(C mine, C* sh) {
    sh[threadIdx.x] = mine;
    __syncthreads();
#pragma unroll
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half && better(sh[threadIdx.x + half], sh[threadIdx.x])) sh[threadIdx.x] = sh[threadIdx.x + half];
        __syncthreads();
    }
    return sh[0];
}

struct SweepArgs {
    const uint32_t* keys;
    const uint8_t* bits;
    int64_t n;
    const unsigned long long* counters;
    const uint32_t* tile_off;      // targets in front of each tile (scanned per-tile counts)
    double c_miss, c_fa, p_target;
    EerCand* eer_part;
    DcfCand* dcf_part;
};

__global__ __launch_bounds__(kThreads) void eval_sweep_kernel(const SweepArgs g) {
    __shared__ uint32_t wtot[kWaves];
    __shared__ EerCand s_eer[kThreads];
    __shared__ DcfCand s_dcf[kThreads];
    const int64_t m = g.n - (int64_t)(g.counters[kCntNan] + g.counters[kCntBad] + g.counters[kCntSkipped]);   // trials kept: the sorted prefix
    const int64_t P = (int64_t)g.counters[kCntTargets], N = m - P;
    const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
    uint32_t key[kItems + 1];
    uint8_t bit[kItems];
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const bool in = base + k < m;
        key[k] = in ? g.keys[base + k] : 0u;
        bit[k] = in ? g.bits[base + k] : (uint8_t)0;
        mine += bit[k] == 1;
    }
    key[kItems] = base + kItems < m ? g.keys[base + kItems] : 0u;
    int64_t tp = (int64_t)block_excl_scan(mine, wtot, nullptr) + (int64_t)g.tile_off[blockIdx.x];
    EerCand be{kNoIdx, kNoIdx, 0};
    DcfCand bd{std::numeric_limits<double>::infinity(), kNoIdx, 0};
    if (P > 0 && N > 0) {
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const int64_t i = base + k;
            if (i >= m) break;
            tp += bit[k] == 1;
            if (i + 1 < m && key[k + 1] == key[k]) continue;      // inside a run of equal scores
            const int64_t fa = N - ((i + 1) - tp);                // non-targets above the threshold
            const int64_t diff = fa * P - tp * N;                 // |.| < 2^62
            const EerCand ce{diff < 0 ? -diff : diff, i, tp};
            if (better(ce, be)) be = ce;
            const double frr = (double)tp / (double)P, far = (double)fa / (double)N;
            const DcfCand cd{g.c_miss * frr * g.p_target + g.c_fa * far * (1.0 - g.p_target), i, tp};
            if (better(cd, bd)) bd = cd;
        }
    }
    be = block_best(be, s_eer);
    bd = block_best(bd, s_dcf);
    if (threadIdx.x == 0) {
        g.eer_part[blockIdx.x] = be;
        g.dcf_part[blockIdx.x] = bd;
    }
}

__global__ __launch_bounds__(kThreads) void eval_final_kernel(const SweepArgs g, int num_tiles, xvec_eval_result* out) {
    __shared__ EerCand s_eer[kThreads];
    __shared__ DcfCand s_dcf[kThreads];
    EerCand be{kNoIdx, kNoIdx, 0};
    DcfCand bd{std::numeric_limits<double>::infinity(), kNoIdx, 0};
    for (int t = threadIdx.x; t < num_tiles; t += kThreads) {
        const EerCand ce = g.eer_part[t];
        const DcfCand cd = g.dcf_part[t];
        if (better(ce, be)) be = ce;
        if (better(cd, bd)) bd = cd;
    }
    be = block_best(be, s_eer);
    bd = block_best(bd, s_dcf);
    if (threadIdx.x != 0) return;
    const int64_t n_nan = (int64_t)g.counters[kCntNan], n_bad = (int64_t)g.counters[kCntBad];
    const int64_t m = g.n - n_nan - n_bad - (int64_t)g.counters[kCntSkipped];
    const int64_t P = (int64_t)g.counters[kCntTargets], N = m - P;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    xvec_eval_result r;
    r.eer = r.eer_threshold = r.far = r.frr = r.min_dcf = r.min_dcf_threshold = nan;
    r.n_target = P;
    r.n_nontarget = N;
    r.n_nan = n_nan;
    r.n_bad_index = n_bad;
    if (be.idx != kNoIdx && bd.idx != kNoIdx && be.idx < m && bd.idx < m) {
        const int64_t fa = N - ((be.idx + 1) - be.tp);
        r.far = (double)fa / (double)N;
        r.frr = (double)be.tp / (double)P;
        r.eer = (r.far + r.frr) / 2.0;
        r.eer_threshold = (double)key_score(g.keys[be.idx]);
        r.min_dcf = bd.val;
        r.min_dcf_threshold = (double)key_score(g.keys[bd.idx]);
    }
    *out = r;
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_eerr;

inline int64_t chunks(int64_t len) { return (len + kTile - 1) / kTile; }

// The sizes of one evaluation and its workspace buffers (null, all of them, when the plan is made over a null workspace)
struct EvalPlan {
    int64_t n, tiles, hist_len;
    uint32_t* keys[2];
    uint8_t* bits[2];
    uint32_t *hist, *hist_sums, *tile_sums, *tile_top;
    unsigned long long* counters;
    EerCand* eer;
    DcfCand* dcf;
    size_t total;
};

EvalPlan make_plan(void* workspace, int64_t n) {
    EvalPlan p{};
    p.n = n;
    p.tiles = chunks(n);
    p.hist_len = p.tiles * kRadix;
    Carver c(workspace);
    for (int i = 0; i < 2; ++i) p.keys[i] = c.take<uint32_t>((size_t)n);
    for (int i = 0; i < 2; ++i) p.bits[i] = c.take<uint8_t>((size_t)n);
    p.hist = c.take<uint32_t>((size_t)p.hist_len);
    p.hist_sums = c.take<uint32_t>((size_t)chunks(p.hist_len));
    p.tile_sums = c.take<uint32_t>((size_t)p.tiles);
    p.tile_top = c.take<uint32_t>((size_t)chunks(p.tiles));
    p.counters = c.take<unsigned long long>(kCounters);
    p.eer = c.take<EerCand>((size_t)p.tiles);
    p.dcf = c.take<DcfCand>((size_t)p.tiles);
    p.total = c.total();
    return p;
}

// v[0 .. len) <- its exclusive scan; *total_out (device, may be null) <- the sum
int scan_in_place(uint32_t* v, int64_t len, uint32_t* sums, unsigned long long* total_out, hipStream_t s) {
    const int64_t nc = chunks(len);
    int rc;
    eval_scan_sums_kernel<<<(unsigned)nc, kThreads, 0, s>>>(v, len, sums);
    if ((rc = g_eerr.launch_ok("eval_scan_sums_kernel"))) return rc;
    eval_scan_top_kernel<<<1, kThreads, 0, s>>>(sums, nc, total_out);
    if ((rc = g_eerr.launch_ok("eval_scan_top_kernel"))) return rc;
    eval_scan_apply_kernel<<<(unsigned)nc, kThreads, 0, s>>>(v, len, sums);
    return g_eerr.launch_ok("eval_scan_apply_kernel");
}

// stages 1 and 2: afterwards keys[0] / bits[0] hold the sorted pairs
int gather_and_sort(const TrialArgs& trials, bool all_pairs, const EvalPlan& p, hipStream_t s) {
    const GatherArgs ga{trials, p.keys[0], p.bits[0], p.counters};
    const hipError_t e = hipMemsetAsync(p.counters, 0, kCounters * sizeof(unsigned long long), s);
    if (e != hipSuccess) return g_eerr.fail(XVEC_ERR_HIP, "clearing the counters failed: %s", hipGetErrorString(e));
    const unsigned grid = (unsigned)p.tiles;
    int rc;
    if (all_pairs) eval_gather_kernel<true><<<grid, kThreads, 0, s>>>(ga);
    else eval_gather_kernel<false><<<grid, kThreads, 0, s>>>(ga);
    if ((rc = g_eerr.launch_ok("eval_gather_kernel"))) return rc;
    for (int pass = 0; pass < 4; ++pass) {
        const int src = pass & 1, dst = src ^ 1, shift = 8 * pass;
        eval_hist_kernel<<<grid, kThreads, 0, s>>>(p.keys[src], p.n, shift, p.hist, (int)p.tiles);
        if ((rc = g_eerr.launch_ok("eval_hist_kernel"))) return rc;
        if ((rc = scan_in_place(p.hist, p.hist_len, p.hist_sums, nullptr, s))) return rc;
        eval_scatter_kernel<<<grid, kThreads, 0, s>>>(p.keys[src], p.bits[src], p.keys[dst], p.bits[dst], p.n, shift, p.hist,
                                                      (int)p.tiles);
        if ((rc = g_eerr.launch_ok("eval_scatter_kernel"))) return rc;
    }
    return XVEC_OK;
}

int sweep(const EvalPlan& p, double c_miss, double c_fa, double p_target, xvec_eval_result* out, hipStream_t s) {
    const unsigned grid = (unsigned)p.tiles;
    int rc;
    eval_bit_sums_kernel<<<grid, kThreads, 0, s>>>(p.bits[0], p.n, p.tile_sums);
    if ((rc = g_eerr.launch_ok("eval_bit_sums_kernel"))) return rc;
    if ((rc = scan_in_place(p.tile_sums, p.tiles, p.tile_top, p.counters + kCntTargets, s))) return rc;
    SweepArgs g{};
    g.keys = p.keys[0];
    g.bits = p.bits[0];
    g.n = p.n;
    g.counters = p.counters;
    g.tile_off = p.tile_sums;
    g.c_miss = c_miss;
    g.c_fa = c_fa;
    g.p_target = p_target;
    g.eer_part = p.eer;
    g.dcf_part = p.dcf;
    eval_sweep_kernel<<<grid, kThreads, 0, s>>>(g);
    if ((rc = g_eerr.launch_ok("eval_sweep_kernel"))) return rc;
    eval_final_kernel<<<1, kThreads, 0, s>>>(g, (int)p.tiles, out);
    return g_eerr.launch_ok("eval_final_kernel");
}

int refused(const Refusal& why, bool too_large = false) {
    return g_eerr.refused(too_large ? XVEC_ERR_TOO_LARGE : XVEC_ERR_ARG, why);
}

int check_costs(double c_miss, double c_fa, double p_target) {
    if (!(c_miss >= 0.0) || !(c_fa >= 0.0) || !(p_target >= 0.0 && p_target <= 1.0) || c_miss > 1e300 || c_fa > 1e300)
        return g_eerr.fail(XVEC_ERR_ARG, "c_miss = %g and c_fa = %g must be finite and >= 0, p_target = %g in [0, 1]", c_miss, c_fa,
                           p_target);
    return XVEC_OK;
}

// trial_plan.h's check_trials in its pieces: this unit answers one unnamed "null pointer" for is_target and the workspace
// (include/xvec_eval.h), where the other units name them apart.
int check_trials(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                 const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, void* workspace, size_t workspace_bytes,
                 EvalPlan* plan) {
    Refusal why;
    bool too_large;
    if (trial_plan::check_trial_count(n_trials, why, &too_large) || trial_plan::check_matrix(scores, ld, n_rows, n_cols, why))
        return refused(why, too_large);
    if (!is_target || !workspace) return g_eerr.fail(XVEC_ERR_ARG, "null pointer");
    if (trial_plan::check_index_pair(row_idx, col_idx, why) ||
        trial_plan::check_vector_form(row_idx, n_rows, n_cols, n_trials, why))
        return refused(why);
    *plan = make_plan(workspace, n_trials);
    return workspace_ok(workspace_bytes, plan->total, g_eerr);
}

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_eval_last_error(void) { return g_eerr.c_str(); }

size_t xvec_eval_workspace_bytes(int64_t n_trials) {
    if (!trial_plan::count_ok(n_trials)) return 0;
    return make_plan(nullptr, n_trials).total;
}

int xvec_eval_trials(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                     const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, double c_miss, double c_fa,
                     double p_target, xvec_eval_result* out, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    EvalPlan p;
    int rc;
    if ((rc = check_trials(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, workspace, workspace_bytes, &p)))
        return rc;
    if (!out) return g_eerr.fail(XVEC_ERR_ARG, "null pointer: out");
    if ((rc = check_costs(c_miss, c_fa, p_target))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((rc = gather_and_sort(trial_args(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, false), false, p, s)))
        return rc;
    return sweep(p, c_miss, c_fa, p_target, out, s);
}

int xvec_eval_all_pairs(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_class,
                        const int32_t* col_class, int32_t skip_diagonal, double c_miss, double c_fa, double p_target,
                        xvec_eval_result* out, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    // trial_plan.h's check_all_pairs in its pieces, around this unit's one unnamed "null pointer"
    Refusal why;
    bool too_large;
    if (trial_plan::check_matrix(scores, ld, n_rows, n_cols, why)) return refused(why);
    if (!row_class || !col_class || !out || !workspace) return g_eerr.fail(XVEC_ERR_ARG, "null pointer");
    if (trial_plan::check_cell_count(n_rows, n_cols, why, &too_large)) return refused(why, too_large);
    int rc;
    if ((rc = check_costs(c_miss, c_fa, p_target))) return rc;
    const int64_t n = n_rows * n_cols;
    const EvalPlan p = make_plan(workspace, n);
    if ((rc = workspace_ok(workspace_bytes, p.total, g_eerr))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((rc = gather_and_sort(trial_args(scores, ld, n_rows, n_cols, row_class, col_class, nullptr, n, skip_diagonal != 0), true, p, s)))
        return rc;
    return sweep(p, c_miss, c_fa, p_target, out, s);
}

int xvec_eval_sorted_keys(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                          const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, uint32_t* keys_out,
                          uint8_t* bits_out, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    EvalPlan p;
    int rc;
    if ((rc = check_trials(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, workspace, workspace_bytes, &p)))
        return rc;
    if (!keys_out || !bits_out) return g_eerr.fail(XVEC_ERR_ARG, "null pointer: keys_out / bits_out");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((rc = gather_and_sort(trial_args(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, false), false, p, s)))
        return rc;
    hipError_t e = hipMemcpyAsync(keys_out, p.keys[0], (size_t)n_trials * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(bits_out, p.bits[0], (size_t)n_trials, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return g_eerr.fail(XVEC_ERR_HIP, "copying the sorted pairs failed: %s", hipGetErrorString(e));
    return XVEC_OK;
}

}  // extern "C"
