// Score calibration: prior-weighted linear logistic regression, the affine map, Cllr / actual DCF, and PAV minCllr.
// C ABI, the definitions, the stopping rule and the summation order: include/xvec_calib.h.  Plan and checks: calib_plan.h.
// The trial reader, the inverse of the score key and the block sums, counts and scans: trial_device.h, shared with eval.hip and
// report.hip, so that the three units leave out the same trials.
//   fit       gather (trial score and target bit into the workspace, block partials of the counts and of sum s)
//             -> mean (one block) -> sum (s - mu)^2 (block partials) -> start (one block: sd, the weights, the first point)
//             -> max_iter x [ pass (J, g_a, g_b, H_aa, H_ab, H_bb at the trial point: block partials)
//                             solve (one block: reduce, accept or halve, Newton step, convergence, next point) ]
//             -> finish (one block: the record).  Every kernel of the loop returns at once when the state says done.
//   apply     out = a s + b, tiles of 8 rows x 256 columns, a thread per column; a and b from the device record.
//   cllr      one fused pass (gather, softplus in bits, misses and false alarms at the Bayes threshold) -> one block.
//   min_cllr  xvec_eval_sorted_keys -> counts per block -> their scan (one block) -> hull level 1 (stacks in LDS)
//             -> hull levels 2.. (in place in global memory) -> final (one block: pairwise merge, origin, segments, sum).
// Only integer counts go through LDS atomics; every floating-point sum has the one order the header states.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "../../include/xvec_calib.h"
#include "../../include/xvec_eval.h"
#include "../../include/xvec_hip.h"
#include "calib_plan.h"
#include "host_support.h"
#include "trial_device.h"

// Every operation rounds on its own: apply's result is numpy's a * S + b bit for bit, and the error bounds of
// tests/test_calibrate_gpu.py count roundings.
#pragma clang fp contract(off)

namespace xvec {
namespace {

using namespace calib_plan;
using namespace trial_device;      // the trial reader (as eval.hip gathers the trials), key_score, the block primitives

constexpr int kWaves = kThreads / 64;
constexpr double kLn2 = 0.693147180559945309417232121458;
constexpr double kLog2e = 1.442695040888963407359924681002;
constexpr double kAcceptSlack = 0x1p-40;
constexpr double kStepCap = 8.0;

// softplus(x) / ln 2 with softplus(0) = ln 2 exactly (include/xvec_calib.h)
__device__ __forceinline__ double softplus_bits(double x) {
    if (x == 0.0) return 1.0;
    return (fmax(x, 0.0) + log1p(exp(-fabs(x)))) * kLog2e;
}

// ---------------------------------------------------------------- fit

// The Newton state, in the workspace (device only).
struct FitState {
    double x[2], jx;           // the last accepted point (standardised coordinates) and its objective
    double y[2];               // the trial point of the next pass
    double d[2];               // the step that led from x to y
    double mu, inv_sd, sd;
    double w_tar, w_non, tau;
    long long n_tar, n_non, n_nan, n_bad, n_inf;
    int32_t have_x, done, status, n_iter;
};
static_assert(sizeof(FitState) <= 256, "the state's slot in the workspace");

// partial words of a block
enum { kPJ = 0, kPGa = 1, kPGb = 2, kPHaa = 3, kPHab = 4, kPHbb = 5 };
enum { kCTar = 0, kCNon = 1, kCNan = 2, kCBad = 3, kCInf = 4, kCSum = 5 };      // gather: five counts (as int64 bits) and sum s

template <bool ALL_PAIRS>
__global__ __launch_bounds__(kThreads) void calib_gather_kernel(const TrialArgs g, double* __restrict__ fs,
                                                                uint8_t* __restrict__ fb, double* __restrict__ part) {
    __shared__ double wsum[kWaves];
    __shared__ long long wcnt[kWaves];
    long long c_tar = 0, c_non = 0, c_nan = 0, c_bad = 0, c_inf = 0;
    double sum = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kTile;
    for (int64_t base = (int64_t)blockIdx.x * kTile; base < g.n; base += stride) {
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const int64_t t = base + k * kThreads + threadIdx.x;
            if (t >= g.n) break;
            const Trial tr = read_trial<ALL_PAIRS>(g, t);
            double s = 0.0;
            uint8_t bit = kBitVoid;
            if (tr.what == kUse) {
                s = tr.score;
                bit = tr.target ? 1 : 0;
                c_tar += tr.target;
                c_non += !tr.target;
                c_inf += isinf(s) ? 1 : 0;
                sum += s;
            } else {
                c_nan += tr.what == kNan;
                c_bad += tr.what == kBad;
            }
            fs[t] = s;
            fb[t] = bit;
        }
    }
    long long* ipart = reinterpret_cast<long long*>(part) + (size_t)blockIdx.x * kPartialWords;
    const long long t0 = block_count(c_tar, wcnt), t1 = block_count(c_non, wcnt), t2 = block_count(c_nan, wcnt),
                    t3 = block_count(c_bad, wcnt), t4 = block_count(c_inf, wcnt);
    const double ts = block_sum(sum, wsum);
    if (threadIdx.x == 0) {
        ipart[kCTar] = t0;
        ipart[kCNon] = t1;
        ipart[kCNan] = t2;
        ipart[kCBad] = t3;
        ipart[kCInf] = t4;
        part[(size_t)blockIdx.x * kPartialWords + kCSum] = ts;
    }
}

// One block: the counts, the mean, the status of a set that cannot be fitted.
__global__ __launch_bounds__(kThreads) void calib_mean_kernel(const double* __restrict__ part, int blocks, FitState* st) {
    __shared__ double wsum[kWaves];
    __shared__ long long wcnt[kWaves];
    const long long* ipart = reinterpret_cast<const long long*>(part);
    long long c[5] = {0, 0, 0, 0, 0};
    double sum = 0.0;
    for (int b = threadIdx.x; b < blocks; b += kThreads) {
#pragma unroll
        for (int q = 0; q < 5; ++q) c[q] += ipart[(size_t)b * kPartialWords + q];
        sum += part[(size_t)b * kPartialWords + kCSum];
    }
    long long tot[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) tot[q] = block_count(c[q], wcnt);
    const double total = block_sum(sum, wsum);
    if (threadIdx.x != 0) return;
    FitState s{};
    s.n_tar = tot[kCTar];
    s.n_non = tot[kCNon];
    s.n_nan = tot[kCNan];
    s.n_bad = tot[kCBad];
    s.n_inf = tot[kCInf];
    if (s.n_tar == 0 || s.n_non == 0) {
        s.done = 1;
        s.status = XVEC_CALIB_ONE_CLASS;
    } else if (s.n_inf != 0) {
        s.done = 1;
        s.status = XVEC_CALIB_INF_SCORE;
    } else {
        s.mu = total / (double)(s.n_tar + s.n_non);
        s.status = XVEC_CALIB_MAX_ITER;
    }
    *st = s;
}

__global__ __launch_bounds__(kThreads) void calib_var_kernel(const double* __restrict__ fs, const uint8_t* __restrict__ fb,
                                                             int64_t n, const FitState* st, double* __restrict__ part) {
    __shared__ double wsum[kWaves];
    if (st->done) return;
    const double mu = st->mu;
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kTile;
    for (int64_t base = (int64_t)blockIdx.x * kTile; base < n; base += stride) {
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const int64_t t = base + k * kThreads + threadIdx.x;
            if (t < n && fb[t] != kBitVoid) {
                const double d = fs[t] - mu;
                acc += d * d;
            }
        }
    }
    const double total = block_sum(acc, wsum);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * kPartialWords] = total;
}

__global__ __launch_bounds__(kThreads) void calib_start_kernel(const double* __restrict__ part, int blocks, double p_target,
                                                               FitState* st) {
    __shared__ double wsum[kWaves];
    if (st->done) return;
    double acc = 0.0;
    for (int b = threadIdx.x; b < blocks; b += kThreads) acc += part[(size_t)b * kPartialWords];
    const double total = block_sum(acc, wsum);
    if (threadIdx.x != 0) return;
    double sd = sqrt(total / (double)(st->n_tar + st->n_non));
    if (!(sd > 0.0) || isinf(sd)) sd = 1.0;
    st->sd = sd;
    st->inv_sd = 1.0 / sd;
    st->w_tar = p_target / (double)st->n_tar;
    st->w_non = (1.0 - p_target) / (double)st->n_non;
    st->tau = log(p_target) - log1p(-p_target);
    st->x[0] = st->x[1] = st->y[0] = st->y[1] = st->d[0] = st->d[1] = 0.0;
    st->jx = 0.0;
    st->have_x = 0;
    st->n_iter = 0;
}

// J, the gradient and the Hessian at st->y, block partials
__global__ __launch_bounds__(kThreads) void calib_pass_kernel(const double* __restrict__ fs, const uint8_t* __restrict__ fb,
                                                              int64_t n, const FitState* st, double* __restrict__ part) {
    __shared__ double wsum[kWaves];
    if (st->done) return;
    const double mu = st->mu, inv_sd = st->inv_sd, a = st->y[0], b = st->y[1] + st->tau, w_tar = st->w_tar, w_non = st->w_non;
    double j = 0.0, ga = 0.0, gb = 0.0, haa = 0.0, hab = 0.0, hbb = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kTile;
    for (int64_t base = (int64_t)blockIdx.x * kTile; base < n; base += stride) {
        double s[kItems];
        uint8_t bit[kItems];
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const int64_t t = base + k * kThreads + threadIdx.x;
            bit[k] = t < n ? fb[t] : kBitVoid;
            s[k] = t < n ? fs[t] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            if (bit[k] == kBitVoid) continue;
            const bool tar = bit[k] == 1;
            const double z = (s[k] - mu) * inv_sd;
            const double x = a * z + b;
            const double u = tar ? -x : x;            // the term is w softplus(u)
            const double w = tar ? w_tar : w_non;
            const double e = exp(-fabs(u));
            const double q = 1.0 / (1.0 + e);
            const double sig = u >= 0.0 ? q : e * q;  // logistic(u)
            const double dj = tar ? -(w * sig) : w * sig;     // d term / d x
            const double h = w * (e * q * q);         // d2 term / d x2 = w logistic(u) logistic(-u)
            j += w * (fmax(u, 0.0) + log1p(e));
            ga += dj * z;
            gb += dj;
            const double hz = h * z;
            haa += hz * z;
            hab += hz;
            hbb += h;
        }
    }
    double* out = part + (size_t)blockIdx.x * kPartialWords;
    const double v[6] = {j, ga, gb, haa, hab, hbb};
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double total = block_sum(v[q], wsum);
        if (threadIdx.x == 0) out[q] = total;
    }
}

__device__ __forceinline__ bool finite2(double a, double b) { return isfinite(a) && isfinite(b); }

__global__ __launch_bounds__(kThreads) void calib_solve_kernel(const double* __restrict__ part, int blocks, FitState* st) {
    __shared__ double wsum[kWaves];
    if (st->done) return;
    double tot[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        double acc = 0.0;
        for (int b = threadIdx.x; b < blocks; b += kThreads) acc += part[(size_t)b * kPartialWords + q];
        tot[q] = block_sum(acc, wsum);
    }
    if (threadIdx.x != 0) return;
    st->n_iter += 1;
    const double jy = tot[kPJ];
    const bool accept = isfinite(jy) && (!st->have_x || jy <= st->jx + kAcceptSlack * fabs(st->jx));
    if (!accept) {                             // the objective rose (or left the finite range): half the step from x
        st->d[0] *= 0.5;
        st->d[1] *= 0.5;
        st->y[0] = st->x[0] + st->d[0];
        st->y[1] = st->x[1] + st->d[1];
        return;
    }
    st->x[0] = st->y[0];
    st->x[1] = st->y[1];
    st->jx = jy;
    st->have_x = 1;
    const double ga = tot[kPGa], gb = tot[kPGb];
    double haa = tot[kPHaa], hab = tot[kPHab], hbb = tot[kPHbb];
    double det = haa * hbb - hab * hab;
    if (!(det > 1e-12 * (haa * hbb))) {        // singular to working precision: damped
        const double lam = 1e-12 * (haa + hbb) + 1e-300;
        haa += lam;
        hbb += lam;
        det = haa * hbb - hab * hab;
    }
    double da = -(hbb * ga - hab * gb) / det, db = -(haa * gb - hab * ga) / det;
    if (!finite2(da, db)) {                    // nothing left to solve with (a separable set driven to saturation)
        st->done = 1;
        return;                                // status stays XVEC_CALIB_MAX_ITER; x is the last finite point
    }
    const double big = fmax(fabs(da), fabs(db));
    if (big > kStepCap) {
        da *= kStepCap / big;
        db *= kStepCap / big;
    }
    const double ya = st->x[0] + da, yb = st->x[1] + db;
    if (big <= XVEC_CALIB_STEP_TOL * fmax(1.0, fmax(fabs(st->x[0]), fabs(st->x[1])))) {
        st->x[0] = ya;                         // the reported point; jx stays J of the point the step was taken from
        st->x[1] = yb;
        st->done = 1;
        st->status = XVEC_CALIB_CONVERGED;
        return;
    }
    st->d[0] = da;
    st->d[1] = db;
    st->y[0] = ya;
    st->y[1] = yb;
}

__global__ void calib_finish_kernel(const FitState* st, xvec_calib_fit_result* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    xvec_calib_fit_result r;
    r.a = r.b = r.objective_bits = nan;
    r.n_target = st->n_tar;
    r.n_nontarget = st->n_non;
    r.n_nan = st->n_nan;
    r.n_bad_index = st->n_bad;
    r.n_iter = st->n_iter;
    r.status = st->status;
    if (st->status == XVEC_CALIB_CONVERGED || (st->status == XVEC_CALIB_MAX_ITER && st->have_x)) {
        const double a = st->x[0] / st->sd;
        r.a = a;
        r.b = st->x[1] - a * st->mu;
        r.objective_bits = st->jx / kLn2;
    } else if (st->status == XVEC_CALIB_MAX_ITER) {      // not one pass accepted (max_iter passes of a non-finite objective)
        r.a = 0.0;
        r.b = 0.0;
        r.objective_bits = nan;
    }
    *out = r;
}

// ---------------------------------------------------------------- apply

struct ApplyArgs {
    const double* scores;
    double* out;
    int64_t ld, ld_out, n_rows, n_cols, col_tiles;
    const xvec_calib_fit_result* fit;
};

__global__ __launch_bounds__(XVEC_CALIB_APPLY_COLS) void calib_apply_kernel(const ApplyArgs g) {
    const int64_t tile_r = blockIdx.x / g.col_tiles, tile_c = blockIdx.x - tile_r * g.col_tiles;
    const int64_t j = tile_c * XVEC_CALIB_APPLY_COLS + threadIdx.x;
    if (j >= g.n_cols) return;
    const double a = g.fit->a, b = g.fit->b;
    const int64_t i0 = tile_r * XVEC_CALIB_APPLY_ROWS;
    double s[XVEC_CALIB_APPLY_ROWS];
#pragma unroll
    for (int r = 0; r < XVEC_CALIB_APPLY_ROWS; ++r)
        if (i0 + r < g.n_rows) s[r] = g.scores[(i0 + r) * g.ld + j];
#pragma unroll
    for (int r = 0; r < XVEC_CALIB_APPLY_ROWS; ++r)
        if (i0 + r < g.n_rows) {
            const double p = a * s[r];         // (rounded on its own: contraction is off in this file)
            g.out[(i0 + r) * g.ld_out + j] = p + b;
        }
}

// ---------------------------------------------------------------- Cllr and the actual DCF

enum { kLTar = 0, kLNon = 1, kLNan = 2, kLBad = 3, kLMiss = 4, kLFa = 5, kLSumTar = 6, kLSumNon = 7 };

template <bool ALL_PAIRS>
__global__ __launch_bounds__(kThreads) void calib_cllr_kernel(const TrialArgs g, double threshold, double* __restrict__ part) {
    __shared__ double wsum[kWaves];
    __shared__ long long wcnt[kWaves];
    long long c[6] = {0, 0, 0, 0, 0, 0};
    double st = 0.0, sn = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kTile;
    for (int64_t base = (int64_t)blockIdx.x * kTile; base < g.n; base += stride) {
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const int64_t t = base + k * kThreads + threadIdx.x;
            if (t >= g.n) break;
            const Trial tr = read_trial<ALL_PAIRS>(g, t);
            const double l = tr.score;
            if (tr.what == kUse) {
                const bool rejected = l <= threshold;
                if (tr.target) {
                    c[kLTar] += 1;
                    c[kLMiss] += rejected;
                    st += softplus_bits(-l);
                } else {
                    c[kLNon] += 1;
                    c[kLFa] += !rejected;
                    sn += softplus_bits(l);
                }
            } else {
                c[kLNan] += tr.what == kNan;
                c[kLBad] += tr.what == kBad;
            }
        }
    }
    long long* ipart = reinterpret_cast<long long*>(part) + (size_t)blockIdx.x * kPartialWords;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const long long total = block_count(c[q], wcnt);
        if (threadIdx.x == 0) ipart[q] = total;
    }
    const double t0 = block_sum(st, wsum), t1 = block_sum(sn, wsum);
    if (threadIdx.x == 0) {
        part[(size_t)blockIdx.x * kPartialWords + kLSumTar] = t0;
        part[(size_t)blockIdx.x * kPartialWords + kLSumNon] = t1;
    }
}

__global__ __launch_bounds__(kThreads) void calib_cllr_final_kernel(const double* __restrict__ part, int blocks, double c_miss,
                                                                    double c_fa, double p_target, double threshold,
                                                                    xvec_calib_cllr_result* out) {
    __shared__ double wsum[kWaves];
    __shared__ long long wcnt[kWaves];
    const long long* ipart = reinterpret_cast<const long long*>(part);
    long long c[6] = {0, 0, 0, 0, 0, 0};
    double st = 0.0, sn = 0.0;
    for (int b = threadIdx.x; b < blocks; b += kThreads) {
#pragma unroll
        for (int q = 0; q < 6; ++q) c[q] += ipart[(size_t)b * kPartialWords + q];
        st += part[(size_t)b * kPartialWords + kLSumTar];
        sn += part[(size_t)b * kPartialWords + kLSumNon];
    }
    long long tot[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) tot[q] = block_count(c[q], wcnt);
    const double sum_tar = block_sum(st, wsum), sum_non = block_sum(sn, wsum);
    if (threadIdx.x != 0) return;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    xvec_calib_cllr_result r;
    r.cllr = r.act_dcf = r.p_miss = r.p_fa = nan;
    r.threshold = threshold;
    r.n_target = tot[kLTar];
    r.n_nontarget = tot[kLNon];
    r.n_nan = tot[kLNan];
    r.n_bad_index = tot[kLBad];
    if (r.n_target > 0 && r.n_nontarget > 0) {
        const double P = (double)r.n_target, N = (double)r.n_nontarget;
        r.cllr = (sum_tar / P + sum_non / N) / 2.0;
        r.p_miss = (double)tot[kLMiss] / P;
        r.p_fa = (double)tot[kLFa] / N;
        r.act_dcf = c_miss * r.p_miss * p_target + c_fa * r.p_fa * (1.0 - p_target);      // as eval_sweep_kernel forms its DCF
    }
    *out = r;
}

// ---------------------------------------------------------------- PAV: the greatest convex minorant

struct Pt {
    int32_t k, tp;             // trials so far, targets so far
};
struct PavTotals {             // in the state slot of the workspace
    long long m, P;            // trials kept (the sorted prefix), targets among them
};

// > 0: a strict left turn at b (the slope rises).  Both factors of each product lie in [0, 2^31): exact in 64 bits.
__device__ __forceinline__ long long turn(const Pt a, const Pt b, const Pt c) {
    return (long long)(b.k - a.k) * (long long)(c.tp - a.tp) - (long long)(b.tp - a.tp) * (long long)(c.k - a.k);
}

// counts[0][blk] = targets, counts[1][blk] = kept trials among the kHullTile trials of block blk
__global__ __launch_bounds__(kThreads) void calib_pav_counts_kernel(const uint8_t* __restrict__ bits, int64_t n,
                                                                    uint32_t* __restrict__ counts, int64_t blocks) {
    __shared__ uint32_t wtot[kWaves];
    const int64_t base = (int64_t)blockIdx.x * kHullTile;
    uint32_t tar = 0, kept = 0;
#pragma unroll 4
    for (int k = 0; k < kChunk; ++k) {
        const int64_t i = base + k * kThreads + threadIdx.x;
        if (i < n) {
            const uint8_t b = bits[i];
            tar += b == 1;
            kept += b != kBitVoid;
        }
    }
    uint32_t t_tar, t_kept;
    block_excl_scan(tar, wtot, &t_tar);
    block_excl_scan(kept, wtot, &t_kept);
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = t_tar;
        counts[blocks + blockIdx.x] = t_kept;
    }
}

// One block: counts[0] <- its exclusive scan (the targets in front of every block); the totals.
__global__ __launch_bounds__(kThreads) void calib_pav_scan_kernel(uint32_t* __restrict__ counts, int64_t blocks, PavTotals* tot) {
    __shared__ uint32_t wtot[kWaves];
    const uint32_t targets = block_scan_array(counts, counts, blocks, wtot);
    const uint32_t kept = block_scan_array(counts + blocks, nullptr, blocks, wtot);      // at most n < 2^31
    if (threadIdx.x == 0) {
        tot->m = (long long)kept;
        tot->P = (long long)targets;
    }
}

// Level 1: thread t of block blk owns the trials [blk * kHullTile + t * kChunk, + kChunk).  The point of trial i (the last of
// its run of equal keys, i < m) is (i + 1, targets among the trials 0 .. i).  The thread's stack lives in LDS, kChunk + 1
// slots apart; the survivors go to the front of the chunk's own slots of `pts`.
__global__ __launch_bounds__(kThreads) void calib_hull_first_kernel(const uint32_t* __restrict__ keys,
                                                                    const uint8_t* __restrict__ bits, int64_t n,
                                                                    const uint32_t* __restrict__ tar_before,
                                                                    const PavTotals* tot, Pt* __restrict__ pts,
                                                                    uint32_t* __restrict__ group_cnt) {
    __shared__ Pt stack[kThreads * (kChunk + 1)];
    __shared__ uint32_t wtot[kWaves];
    const int64_t m = tot->m;
    const int64_t i0 = (int64_t)blockIdx.x * kHullTile + (int64_t)threadIdx.x * kChunk;
    uint32_t key[kChunk + 1];
    uint8_t bit[kChunk];
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
        const bool in = i0 + k < m;
        key[k] = in ? keys[i0 + k] : 0u;
        bit[k] = in ? bits[i0 + k] : (uint8_t)0;
        mine += bit[k] == 1;
    }
    key[kChunk] = i0 + kChunk < m ? keys[i0 + kChunk] : 0u;
    uint32_t tp = block_excl_scan(mine, wtot, nullptr) + tar_before[blockIdx.x];
    Pt* s = stack + threadIdx.x * (kChunk + 1);
    int sz = 0;
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
        const int64_t i = i0 + k;
        if (i < m) {
            tp += bit[k] == 1;
            if (i + 1 == m || key[k + 1] != key[k]) {      // the end of a tie group
                const Pt p{(int32_t)(i + 1), (int32_t)tp};
                while (sz >= 2 && turn(s[sz - 2], s[sz - 1], p) <= 0) --sz;
                s[sz++] = p;
            }
        }
    }
    if (i0 < n) {
        for (int q = 0; q < sz; ++q) pts[i0 + q] = s[q];
        group_cnt[i0 / kChunk] = (uint32_t)sz;
    }
}

// Appends the hull at src[0 .. cnt) to the stack dst[0 .. sz) (points to the right of it), in place: dst + sz <= src.
__device__ __forceinline__ int hull_append(Pt* dst, int sz, const Pt* src, int cnt) {
    for (int q = 0; q < cnt; ++q) {
        const Pt p = src[q];
        while (sz >= 2 && turn(dst[sz - 2], dst[sz - 1], p) <= 0) --sz;
        dst[sz++] = p;
    }
    return sz;
}

// Level l >= 2: thread g merges the groups g * kChunk .. of the level before (each `span_in` slots wide) into one.
__global__ __launch_bounds__(kThreads) void calib_hull_level_kernel(Pt* pts, const uint32_t* __restrict__ cnt_in,
                                                                    int64_t groups_in, int64_t span_in,
                                                                    uint32_t* __restrict__ cnt_out, int64_t groups_out) {
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= groups_out) return;
    const int64_t first = g * kChunk;
    Pt* dst = pts + first * span_in;
    int sz = (int)cnt_in[first];
    for (int j = 1; j < kChunk && first + j < groups_in; ++j)
        sz = hull_append(dst, sz, pts + (first + j) * span_in, (int)cnt_in[first + j]);
    cnt_out[g] = (uint32_t)sz;
}

struct PavOut {
    xvec_calib_pav_result* res;
    int64_t* k_end;
    int64_t* tp_end;
    float* score;
    double* llr;
    int64_t capacity;
};

// One block: the `groups` <= kFinal groups (each `span` slots wide) merged pairwise; the origin in front; the segments.
__global__ __launch_bounds__(kThreads) void calib_hull_final_kernel(Pt* pts, const uint32_t* __restrict__ cnt_in, int groups,
                                                                    int64_t span, const uint32_t* __restrict__ keys,
                                                                    int64_t n, const PavTotals* tot, const PavOut o) {
    __shared__ int cnt[kFinal];
    __shared__ double wsum[kWaves];
    __shared__ int s_first;
    const int t = threadIdx.x;
    if (t < kFinal) cnt[t] = t < groups ? (int)cnt_in[t] : 0;
    __syncthreads();
    for (int stride = 1; stride < groups; stride <<= 1) {
        if (t % (2 * stride) == 0 && t + stride < groups)
            cnt[t] = hull_append(pts + (int64_t)t * span, cnt[t], pts + (int64_t)(t + stride) * span, cnt[t + stride]);
        __syncthreads();
    }
    const int v = cnt[0];                      // the hull of the points; its first and last point always belong to it
    const long long m = tot->m, P = tot->P, N = m - P;
    // the origin in front: the vertices before the first strict left turn seen from it fall away
    if (t == 0) s_first = v > 0 ? v - 1 : 0;
    __syncthreads();
    const Pt origin{0, 0};
    for (int j = t; j + 1 < v; j += kThreads)
        if (turn(origin, pts[j], pts[j + 1]) > 0) atomicMin(&s_first, j);
    __syncthreads();
    const int first = s_first, segs = v > 0 ? v - first : 0;
    const double prior = log((double)P / (double)N);
    double acc = 0.0;
    for (int j = t; j < segs; j += kThreads) {
        const Pt hi = pts[first + j], lo = j == 0 ? origin : pts[first + j - 1];
        const long long tt = hi.tp - lo.tp, ff = (long long)(hi.k - lo.k) - tt;
        const double llr = log((double)tt / (double)ff) - prior;
        if (tt > 0 && ff > 0 && P > 0 && N > 0)
            acc += ((double)tt / (double)P * softplus_bits(-llr) + (double)ff / (double)N * softplus_bits(llr)) / 2.0;
        if (j < o.capacity) {
            o.k_end[j] = hi.k;
            o.tp_end[j] = hi.tp;
            o.score[j] = key_score(keys[hi.k - 1]);
            o.llr[j] = llr;
        }
    }
    const double total = block_sum(acc, wsum);
    if (t != 0) return;
    xvec_calib_pav_result r;
    r.min_cllr = P > 0 && N > 0 ? total : std::numeric_limits<double>::quiet_NaN();
    r.n_segments = segs;
    r.n_target = P;
    r.n_nontarget = N;
    r.n_left_out = n - m;
    *o.res = r;
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_cerr;

struct Buffers {
    Layout lay;
    FitState* state;
    PavTotals* totals;
    double* partials;
    double* fit_scores;
    uint8_t* fit_bits;
    void* eval;
    size_t eval_bytes;
    uint32_t* keys;
    uint8_t* bits;
    Pt* points;
    uint32_t* block_counts;
    uint32_t* group_counts;
};

Buffers carve(void* workspace, int64_t n) {
    Buffers b{};
    b.eval_bytes = xvec_eval_workspace_bytes(n);
    b.lay = make_layout(n, b.eval_bytes);
    char* base = static_cast<char*>(workspace);
    if (!base || b.lay.total == 0) return b;
    b.state = reinterpret_cast<FitState*>(base + b.lay.state);
    b.totals = reinterpret_cast<PavTotals*>(base + b.lay.state);
    b.partials = reinterpret_cast<double*>(base + b.lay.partials);
    b.fit_scores = reinterpret_cast<double*>(base + b.lay.fit_scores);
    b.fit_bits = reinterpret_cast<uint8_t*>(base + b.lay.fit_bits);
    b.eval = base + b.lay.eval;
    b.keys = reinterpret_cast<uint32_t*>(base + b.lay.keys);
    b.bits = reinterpret_cast<uint8_t*>(base + b.lay.bits);
    b.points = reinterpret_cast<Pt*>(base + b.lay.points);
    b.block_counts = reinterpret_cast<uint32_t*>(base + b.lay.block_counts);
    b.group_counts = reinterpret_cast<uint32_t*>(base + b.lay.group_counts);
    return b;
}

int refused(const Refusal& why, bool too_large, const char* call) {
    return g_cerr.refused(too_large ? XVEC_ERR_TOO_LARGE : XVEC_ERR_ARG, why, call);
}

int fit(const TrialArgs& g, bool all_pairs, double p_target, int32_t max_iter, xvec_calib_fit_result* out, void* workspace,
        size_t workspace_bytes, xvec_stream stream, const char* call) {
    Refusal why;
    if (check_fit(p_target, max_iter, why)) return refused(why, false, call);
    if (!out) return g_cerr.fail(XVEC_ERR_ARG, "%s: null pointer: out", call);
    const Buffers b = carve(workspace, g.n);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, b.lay.total, g_cerr))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)pass_blocks(g.n);
    if (all_pairs) calib_gather_kernel<true><<<grid, kThreads, 0, s>>>(g, b.fit_scores, b.fit_bits, b.partials);
    else calib_gather_kernel<false><<<grid, kThreads, 0, s>>>(g, b.fit_scores, b.fit_bits, b.partials);
    if ((rc = g_cerr.launch_ok("calib_gather_kernel"))) return rc;
    calib_mean_kernel<<<1, kThreads, 0, s>>>(b.partials, (int)grid, b.state);
    if ((rc = g_cerr.launch_ok("calib_mean_kernel"))) return rc;
    calib_var_kernel<<<grid, kThreads, 0, s>>>(b.fit_scores, b.fit_bits, g.n, b.state, b.partials);
    if ((rc = g_cerr.launch_ok("calib_var_kernel"))) return rc;
    calib_start_kernel<<<1, kThreads, 0, s>>>(b.partials, (int)grid, p_target, b.state);
    if ((rc = g_cerr.launch_ok("calib_start_kernel"))) return rc;
    for (int it = 0; it < max_iter; ++it) {
        calib_pass_kernel<<<grid, kThreads, 0, s>>>(b.fit_scores, b.fit_bits, g.n, b.state, b.partials);
        if ((rc = g_cerr.launch_ok("calib_pass_kernel"))) return rc;
        calib_solve_kernel<<<1, kThreads, 0, s>>>(b.partials, (int)grid, b.state);
        if ((rc = g_cerr.launch_ok("calib_solve_kernel"))) return rc;
    }
    calib_finish_kernel<<<1, 64, 0, s>>>(b.state, out);
    return g_cerr.launch_ok("calib_finish_kernel");
}

int cllr(const TrialArgs& g, bool all_pairs, double c_miss, double c_fa, double p_target, xvec_calib_cllr_result* out,
         void* workspace, size_t workspace_bytes, xvec_stream stream, const char* call) {
    Refusal why;
    if (check_costs(c_miss, c_fa, p_target, why)) return refused(why, false, call);
    if (!out) return g_cerr.fail(XVEC_ERR_ARG, "%s: null pointer: out", call);
    const Buffers b = carve(workspace, g.n);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, b.lay.total, g_cerr))) return rc;
    const double threshold = std::log((1.0 - p_target) * c_fa) - std::log(p_target * c_miss);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)pass_blocks(g.n);
    if (all_pairs) calib_cllr_kernel<true><<<grid, kThreads, 0, s>>>(g, threshold, b.partials);
    else calib_cllr_kernel<false><<<grid, kThreads, 0, s>>>(g, threshold, b.partials);
    if ((rc = g_cerr.launch_ok("calib_cllr_kernel"))) return rc;
    calib_cllr_final_kernel<<<1, kThreads, 0, s>>>(b.partials, (int)grid, c_miss, c_fa, p_target, threshold, out);
    return g_cerr.launch_ok("calib_cllr_final_kernel");
}

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_calib_last_error(void) { return g_cerr.c_str(); }

size_t xvec_calib_workspace_bytes(int64_t n_trials) {
    if (!count_ok(n_trials)) return 0;
    return make_layout(n_trials, xvec_eval_workspace_bytes(n_trials)).total;
}

int xvec_calib_fit(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                   const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, double p_target, int32_t max_iter,
                   xvec_calib_fit_result* out, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    Refusal why;
    bool too_large;
    if (check_trials(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, why, &too_large))
        return refused(why, too_large, "xvec_calib_fit");
    return fit(trial_args(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, 0), false, p_target, max_iter, out,
               workspace, workspace_bytes, stream, "xvec_calib_fit");
}

int xvec_calib_fit_all_pairs(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_class,
                             const int32_t* col_class, int32_t skip_diagonal, double p_target, int32_t max_iter,
                             xvec_calib_fit_result* out, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    Refusal why;
    bool too_large;
    if (check_all_pairs(scores, ld, n_rows, n_cols, row_class, col_class, why, &too_large))
        return refused(why, too_large, "xvec_calib_fit_all_pairs");
    return fit(trial_args(scores, ld, n_rows, n_cols, row_class, col_class, nullptr, n_rows * n_cols, skip_diagonal != 0), true,
               p_target, max_iter, out, workspace, workspace_bytes, stream, "xvec_calib_fit_all_pairs");
}

int xvec_calib_apply(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const xvec_calib_fit_result* fit_record,
                     double* out, int64_t ld_out, xvec_stream stream) {
    Refusal why;
    bool too_large;
    if (check_apply(scores, ld, n_rows, n_cols, fit_record, out, ld_out, why, &too_large))
        return refused(why, too_large, "xvec_calib_apply");
    ApplyArgs g{};
    g.scores = scores;
    g.out = out;
    g.ld = ld;
    g.ld_out = ld_out;
    g.n_rows = n_rows;
    g.n_cols = n_cols;
    g.col_tiles = apply_col_tiles(n_cols);
    g.fit = fit_record;
    calib_apply_kernel<<<(unsigned)apply_tiles(n_rows, n_cols), XVEC_CALIB_APPLY_COLS, 0, static_cast<hipStream_t>(stream)>>>(g);
    return g_cerr.launch_ok("calib_apply_kernel");
}

int xvec_calib_cllr(const double* llrs, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                    const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, double c_miss, double c_fa,
                    double p_target, xvec_calib_cllr_result* out, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    Refusal why;
    bool too_large;
    if (check_trials(llrs, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, why, &too_large))
        return refused(why, too_large, "xvec_calib_cllr");
    return cllr(trial_args(llrs, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, 0), false, c_miss, c_fa, p_target, out,
                workspace, workspace_bytes, stream, "xvec_calib_cllr");
}

int xvec_calib_cllr_all_pairs(const double* llrs, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_class,
                              const int32_t* col_class, int32_t skip_diagonal, double c_miss, double c_fa, double p_target,
                              xvec_calib_cllr_result* out, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    Refusal why;
    bool too_large;
    if (check_all_pairs(llrs, ld, n_rows, n_cols, row_class, col_class, why, &too_large))
        return refused(why, too_large, "xvec_calib_cllr_all_pairs");
    return cllr(trial_args(llrs, ld, n_rows, n_cols, row_class, col_class, nullptr, n_rows * n_cols, skip_diagonal != 0), true,
                c_miss, c_fa, p_target, out, workspace, workspace_bytes, stream, "xvec_calib_cllr_all_pairs");
}

int xvec_calib_min_cllr(const double* scores, int64_t ld, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                        const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, xvec_calib_pav_result* out,
                        int64_t* seg_k_end, int64_t* seg_tp_end, float* seg_score, double* seg_llr, int64_t seg_capacity,
                        void* workspace, size_t workspace_bytes, xvec_stream stream) {
    const char* call = "xvec_calib_min_cllr";
    Refusal why;
    bool too_large;
    if (check_trials(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, why, &too_large))
        return refused(why, too_large, call);
    if (check_segments(seg_k_end, seg_tp_end, seg_score, seg_llr, seg_capacity, why)) return refused(why, false, call);
    if (!out) return g_cerr.fail(XVEC_ERR_ARG, "%s: null pointer: out", call);
    const int64_t n = n_trials;
    const Buffers b = carve(workspace, n);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, b.lay.total, g_cerr))) return rc;
    HullPlan h;
    if (plan_hull(n, &h)) return g_cerr.fail(XVEC_ERR_ARG, "%s: no hull plan for %lld trials", call, (long long)n);
    if ((rc = xvec_eval_sorted_keys(scores, ld, n_rows, n_cols, row_idx, col_idx, is_target, n, b.keys, b.bits, b.eval, b.eval_bytes,
                                    stream)))
        return g_cerr.fail(rc, "%s: xvec_eval_sorted_keys: %s", call, xvec_eval_last_error());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t hb = b.lay.hull_blocks;
    calib_pav_counts_kernel<<<(unsigned)hb, kThreads, 0, s>>>(b.bits, n, b.block_counts, hb);
    if ((rc = g_cerr.launch_ok("calib_pav_counts_kernel"))) return rc;
    calib_pav_scan_kernel<<<1, kThreads, 0, s>>>(b.block_counts, hb, b.totals);
    if ((rc = g_cerr.launch_ok("calib_pav_scan_kernel"))) return rc;
    uint32_t* cnt[2] = {b.group_counts, b.group_counts + h.groups[1]};      // levels 1, 3, 5 | levels 2, 4, 6
    calib_hull_first_kernel<<<(unsigned)hb, kThreads, 0, s>>>(b.keys, b.bits, n, b.block_counts, b.totals, b.points, cnt[0]);
    if ((rc = g_cerr.launch_ok("calib_hull_first_kernel"))) return rc;
    for (int l = 2; l <= h.levels; ++l) {
        const unsigned grid = (unsigned)((h.groups[l] + kThreads - 1) / kThreads);
        calib_hull_level_kernel<<<grid, kThreads, 0, s>>>(b.points, cnt[l & 1], h.groups[l - 1], h.span[l - 1], cnt[(l & 1) ^ 1],
                                                          h.groups[l]);
        if ((rc = g_cerr.launch_ok("calib_hull_level_kernel"))) return rc;
    }
    PavOut o{out, seg_k_end, seg_tp_end, seg_score, seg_llr, seg_capacity};
    calib_hull_final_kernel<<<1, kThreads, 0, s>>>(b.points, cnt[(h.levels & 1) ^ 1], (int)h.groups[h.levels], h.span[h.levels],
                                                   b.keys, n, b.totals, o);
    return g_cerr.launch_ok("calib_hull_final_kernel");
}

}  // extern "C"
