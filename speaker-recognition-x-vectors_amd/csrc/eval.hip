// Trial-list evaluation: EER and minDCF from scores that stay on the device.
//   reference: plda_score_stat.py:36-97 -> speechbrain 0.5.12 utils.metric_stats EER / minDCF (float32 tensors)
// C ABI and the algorithm: include/xvec_eval.h.  The score key, the trial reader, the block scan and the candidate records:
// trial_device.h; the argument checks: trial_plan.h (both shared with calib.hip and report.hip); the sort: trial_sort.h.  Stages, one kernel each:
//   gather + key   trial score -> fp32 (RNE) -> order-preserving 32-bit key, target bit next to it
//   sort           stable LSD radix sort, 4 passes of 8 bits (trial_sort.h, shared with boot.hip; here the payload is one byte)
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
#include "trial_sort.h"

namespace xvec {
namespace {

using namespace trial_device;
using namespace trial_sort;      // the tile (kThreads, kItems, kTile, kWaves, kRadix), the sort and its scan

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
    EerCand be = no_eer_cand();
    DcfCand bd = no_dcf_cand();
    if (P > 0 && N > 0) {
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const int64_t i = base + k;
            if (i >= m) break;
            tp += bit[k] == 1;
            if (i + 1 < m && key[k + 1] == key[k]) continue;      // inside a run of equal scores
            consider(i, tp, (i + 1) - tp, P, N, g.c_miss, g.c_fa, g.p_target, be, bd);
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
    EerCand be = no_eer_cand();
    DcfCand bd = no_dcf_cand();
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
        const Rates at = rates_at(be.tp, be.idx + 1, P, N);
        r.far = at.far;
        r.frr = at.frr;
        r.eer = at.eer;
        r.eer_threshold = (double)key_score(g.keys[be.idx]);
        r.min_dcf = bd.val;
        r.min_dcf_threshold = (double)key_score(g.keys[bd.idx]);
    }
    *out = r;
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_eerr;

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
    const SortBufs<uint8_t> bufs{{p.keys[0], p.keys[1]}, {p.bits[0], p.bits[1]}, p.hist, p.hist_sums};
    return sort_pairs(bufs, p.n, s, g_eerr);
}

int sweep(const EvalPlan& p, double c_miss, double c_fa, double p_target, xvec_eval_result* out, hipStream_t s) {
    const unsigned grid = (unsigned)p.tiles;
    int rc;
    eval_bit_sums_kernel<<<grid, kThreads, 0, s>>>(p.bits[0], p.n, p.tile_sums);
    if ((rc = g_eerr.launch_ok("eval_bit_sums_kernel"))) return rc;
    if ((rc = scan_in_place(p.tile_sums, p.tiles, p.tile_top, p.counters + kCntTargets, s, g_eerr))) return rc;
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

size_t xvec_eval_sorted_order_workspace_bytes(int64_t n_trials) {
    return trial_plan::count_ok(n_trials) ? trial_sort::sorted_order_bytes(n_trials) : 0;
}

int xvec_eval_sorted_order(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                           const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, uint32_t* keys_out,
                           uint32_t* order_out, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    Refusal why;
    bool too_large;
    if (trial_plan::check_trial_count(n_trials, why, &too_large) || trial_plan::check_matrix(scores, ld, n_rows, n_cols, why))
        return refused(why, too_large);
    if (!is_target || !workspace) return g_eerr.fail(XVEC_ERR_ARG, "null pointer");
    if (trial_plan::check_index_pair(row_idx, col_idx, why) ||
        trial_plan::check_vector_form(row_idx, n_rows, n_cols, n_trials, why))
        return refused(why);
    int rc;
    if ((rc = workspace_ok(workspace_bytes, trial_sort::sorted_order_bytes(n_trials), g_eerr))) return rc;
    if (!keys_out || !order_out) return g_eerr.fail(XVEC_ERR_ARG, "null pointer: keys_out / order_out");
    return trial_sort::sorted_order(trial_args(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, false), false,
                                    keys_out, order_out, workspace, static_cast<hipStream_t>(stream), g_eerr);
}

int xvec_eval_sorted_order_all_pairs(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_class,
                                     const int32_t* col_class, int32_t skip_diagonal, uint32_t* keys_out, uint32_t* order_out,
                                     void* workspace, size_t workspace_bytes, xvec_stream stream) {
    Refusal why;
    bool too_large;
    if (trial_plan::check_matrix(scores, ld, n_rows, n_cols, why)) return refused(why);
    if (!row_class || !col_class || !workspace) return g_eerr.fail(XVEC_ERR_ARG, "null pointer");
    if (trial_plan::check_cell_count(n_rows, n_cols, why, &too_large)) return refused(why, too_large);
    const int64_t n = n_rows * n_cols;
    int rc;
    if ((rc = workspace_ok(workspace_bytes, trial_sort::sorted_order_bytes(n), g_eerr))) return rc;
    if (!keys_out || !order_out) return g_eerr.fail(XVEC_ERR_ARG, "null pointer: keys_out / order_out");
    return trial_sort::sorted_order(trial_args(scores, ld, n_rows, n_cols, row_class, col_class, nullptr, n, skip_diagonal != 0), true,
                                    keys_out, order_out, workspace, static_cast<hipStream_t>(stream), g_eerr);
}

}  // extern "C"
