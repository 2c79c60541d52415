// Score fusion: prior-weighted logistic regression over K terms per trial (score matrices and row / column quality measures)
// and the fused matrix.  C ABI, the definitions, the stopping and damping rules and the summation order: include/xvec_fuse.h.
// Plan and checks: fuse_plan.h.  The trial forms, the block sums and counts: trial_device.h, shared with eval.hip, calib.hip and
// report.hip; the blocks of a pass and the trial-to-thread map are calibration's (calib_plan.h).
//   fit       gather (the K values of every trial kept into K planes, the target bit; block partials of the counts and of every
//             term's sum, minimum and maximum) -> mean (one block: counts, constant terms, mu)
//             -> var (block partials of sum (f - mu)^2 per term) -> start (one block: sd, the weights of the classes, the first point)
//             -> max_iter x [ pass<K> (J, the K + 1 gradient components and the (K + 1)(K + 2) / 2 Hessian entries at the
//                                      trial point, all in registers: block partials)
//                             solve (one block: reduce, ridge, accept or halve, Cholesky with the damping rule, convergence) ]
//             -> finish (one block: the record).  Every kernel of the loop returns at once when the state says done.
//   apply     out = ((w_0 f_0 + w_1 f_1) + ...) + b, calibration's tiles of 8 rows x 256 columns, a thread per column.
// Only integer counts and extremes are order-free; every floating-point sum has the one order the header states.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "../../include/xvec_fuse.h"
#include "../../include/xvec_hip.h"
#include "fuse_plan.h"
#include "host_support.h"
#include "trial_device.h"

// Every operation rounds on its own: apply's result is numpy's w0 * S0 + w1 * S1 + ... + b bit for bit, and the error bounds
// of tests/test_fuse_gpu.py count roundings.
#pragma clang fp contract(off)

namespace xvec {
namespace {

using namespace fuse_plan;
using namespace trial_device;

constexpr int kWaves = kThreads / 64;
constexpr int kDim = kMaxTerms + 1;            // the weights and the bias
constexpr double kLn2 = 0.693147180559945309417232121458;
constexpr double kAcceptSlack = 0x1p-40;
constexpr double kStepCap = 8.0;
constexpr double kPivotTol = 1e-12;

// The terms of a call, by value in the kernel arguments.
struct Terms {
    xvec_fuse_term t[kMaxTerms];
    int k;
};

__device__ __forceinline__ double term_value(const xvec_fuse_term& t, int64_t row, int64_t col) {
    const int64_t at = t.kind == XVEC_FUSE_MATRIX ? row * t.ld + col : t.kind == XVEC_FUSE_ROW ? row : col;
    return t.data[at];
}

// ---------------------------------------------------------------- fit

// The Newton state, in the workspace (device only).  Index k < K is term k, index K the bias.
struct FuseState {
    double x[kDim], jx, jx_data, jx_pen;       // the last accepted point (standardised) and its objective: whole, data part, ridge
    double y[kDim];                            // the trial point of the next pass
    double d[kDim];                            // the step that led from x to y
    double mu[kMaxTerms], sd[kMaxTerms], inv_sd[kMaxTerms];
    double w_tar, w_non, tau, l2;
    long long n_tar, n_non, n_nan, n_bad, n_inf;
    int32_t have_x, done, status, n_iter, k, constant_mask;
};
static_assert(sizeof(FuseState) <= kStateBytes, "the state's slot in the workspace");

enum { kCTar = 0, kCNon = 1, kCNan = 2, kCBad = 3, kCInf = 4 };      // gather: the counts (as int64 bits), then sums, minima, maxima

template <bool ALL_PAIRS>
__global__ __launch_bounds__(kThreads) void fuse_gather_kernel(const TrialArgs g, const Terms tm, double* __restrict__ planes,
                                                               uint8_t* __restrict__ fb, double* __restrict__ part, int stride) {
    __shared__ double wsum[kWaves];
    __shared__ long long wcnt[kWaves];
    long long c_tar = 0, c_non = 0, c_nan = 0, c_bad = 0, c_inf = 0;
    double sum[kMaxTerms], lo[kMaxTerms], hi[kMaxTerms];
#pragma unroll
    for (int q = 0; q < kMaxTerms; ++q) {
        sum[q] = 0.0;
        lo[q] = std::numeric_limits<double>::infinity();
        hi[q] = -std::numeric_limits<double>::infinity();
    }
    const int64_t step = (int64_t)gridDim.x * kTile;
    for (int64_t base = (int64_t)blockIdx.x * kTile; base < g.n; base += step) {
#pragma unroll 2
        for (int k = 0; k < kItems; ++k) {
            const int64_t t = base + k * kThreads + threadIdx.x;
            if (t >= g.n) break;
            Trial tr = locate_trial<ALL_PAIRS>(g, t);
            double v[kMaxTerms];
            bool any_nan = false, any_inf = false;
#pragma unroll
            for (int q = 0; q < kMaxTerms; ++q) {
                v[q] = 0.0;
                if (q < tm.k && tr.what == kUse) {           // the cells of a bad index or a skipped trial are never read
                    v[q] = term_value(tm.t[q], tr.row, tr.col);
                    any_nan |= v[q] != v[q];
                    any_inf |= isinf(v[q]);
                }
            }
            if (tr.what == kUse && any_nan) tr.what = kNan;
            uint8_t bit = kBitVoid;
            if (tr.what == kUse) {
                bit = tr.target ? 1 : 0;
                c_tar += tr.target;
                c_non += !tr.target;
                c_inf += any_inf;
            } else {
                c_nan += tr.what == kNan;
                c_bad += tr.what == kBad;
            }
#pragma unroll
            for (int q = 0; q < kMaxTerms; ++q) {
                if (q < tm.k) {
                    if (tr.what == kUse) {
                        sum[q] += v[q];
                        lo[q] = fmin(lo[q], v[q]);
                        hi[q] = fmax(hi[q], v[q]);
                    }
                    planes[(size_t)q * (size_t)g.n + (size_t)t] = tr.what == kUse ? v[q] : 0.0;
                }
            }
            fb[t] = bit;
        }
    }
    double* out = part + (size_t)blockIdx.x * stride;
    long long* iout = reinterpret_cast<long long*>(out);
    const long long t0 = block_count(c_tar, wcnt), t1 = block_count(c_non, wcnt), t2 = block_count(c_nan, wcnt),
                    t3 = block_count(c_bad, wcnt), t4 = block_count(c_inf, wcnt);
    if (threadIdx.x == 0) {
        iout[kCTar] = t0;
        iout[kCNon] = t1;
        iout[kCNan] = t2;
        iout[kCBad] = t3;
        iout[kCInf] = t4;
    }
#pragma unroll
    for (int q = 0; q < kMaxTerms; ++q) {
        if (q < tm.k) {
            const double s = block_sum(sum[q], wsum);
            const double l = block_extreme<true>(lo[q], wsum);
            const double h = block_extreme<false>(hi[q], wsum);
            if (threadIdx.x == 0) {
                out[kGatherCounts + q] = s;
                out[kGatherCounts + tm.k + q] = l;
                out[kGatherCounts + 2 * tm.k + q] = h;
            }
        }
    }
}

// One block: the counts, the constant terms, the means, the status of a set that cannot be fitted.
__global__ __launch_bounds__(kThreads) void fuse_mean_kernel(const double* __restrict__ part, int blocks, int stride, int k_terms,
                                                             FuseState* st) {
    __shared__ double wsum[kWaves];
    __shared__ long long wcnt[kWaves];
    __shared__ long long cnt[kGatherCounts];
    __shared__ double tsum[kMaxTerms], tlo[kMaxTerms], thi[kMaxTerms];
    const long long* ipart = reinterpret_cast<const long long*>(part);
    for (int q = 0; q < kGatherCounts; ++q) {
        long long c = 0;
        for (int b = threadIdx.x; b < blocks; b += kThreads) c += ipart[(size_t)b * stride + q];
        const long long total = block_count(c, wcnt);
        if (threadIdx.x == 0) cnt[q] = total;
    }
    for (int q = 0; q < k_terms; ++q) {
        double s = 0.0, l = std::numeric_limits<double>::infinity(), h = -std::numeric_limits<double>::infinity();
        for (int b = threadIdx.x; b < blocks; b += kThreads) {
            const double* row = part + (size_t)b * stride + kGatherCounts;
            s += row[q];
            l = fmin(l, row[k_terms + q]);
            h = fmax(h, row[2 * k_terms + q]);
        }
        const double ts = block_sum(s, wsum);
        const double tl = block_extreme<true>(l, wsum);
        const double th = block_extreme<false>(h, wsum);
        if (threadIdx.x == 0) {
            tsum[q] = ts;
            tlo[q] = tl;
            thi[q] = th;
        }
    }
    if (threadIdx.x != 0) return;              // (thread 0 reads back only what it wrote itself)
    for (int q = 0; q < kDim; ++q) st->x[q] = st->y[q] = st->d[q] = 0.0;
    for (int q = 0; q < kMaxTerms; ++q) {
        st->mu[q] = 0.0;
        st->sd[q] = st->inv_sd[q] = 1.0;
    }
    st->jx = st->jx_data = st->jx_pen = 0.0;
    st->w_tar = st->w_non = st->tau = st->l2 = 0.0;
    st->n_tar = cnt[kCTar];
    st->n_non = cnt[kCNon];
    st->n_nan = cnt[kCNan];
    st->n_bad = cnt[kCBad];
    st->n_inf = cnt[kCInf];
    st->have_x = 0;
    st->n_iter = 0;
    st->k = k_terms;
    st->done = 0;
    st->status = XVEC_FUSE_MAX_ITER;
    int mask = 0;
    if (cnt[kCTar] == 0 || cnt[kCNon] == 0) {
        st->done = 1;
        st->status = XVEC_FUSE_ONE_CLASS;
    } else if (cnt[kCInf] != 0) {
        st->done = 1;
        st->status = XVEC_FUSE_INF_SCORE;
    } else {
        const double n = (double)(cnt[kCTar] + cnt[kCNon]);
        for (int q = 0; q < k_terms; ++q) {
            const bool constant = tlo[q] == thi[q];        // exact: include/xvec_fuse.h, STANDARDISE
            mask |= constant ? 1 << q : 0;
            st->mu[q] = constant ? tlo[q] : tsum[q] / n;
        }
    }
    st->constant_mask = mask;
}

__global__ __launch_bounds__(kThreads) void fuse_var_kernel(const double* __restrict__ planes, const uint8_t* __restrict__ fb,
                                                            int64_t n, int k_terms, const FuseState* st, double* __restrict__ part,
                                                            int stride) {
    __shared__ double wsum[kWaves];
    if (st->done) return;
    double acc[kMaxTerms];
#pragma unroll
    for (int q = 0; q < kMaxTerms; ++q) acc[q] = 0.0;
    const int64_t step = (int64_t)gridDim.x * kTile;
    for (int64_t base = (int64_t)blockIdx.x * kTile; base < n; base += step) {
#pragma unroll 2
        for (int k = 0; k < kItems; ++k) {
            const int64_t t = base + k * kThreads + threadIdx.x;
            if (t < n && fb[t] != kBitVoid) {
#pragma unroll
                for (int q = 0; q < kMaxTerms; ++q) {
                    if (q < k_terms) {
                        const double d = planes[(size_t)q * (size_t)n + (size_t)t] - st->mu[q];
                        acc[q] += d * d;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kMaxTerms; ++q) {
        if (q < k_terms) {
            const double total = block_sum(acc[q], wsum);
            if (threadIdx.x == 0) part[(size_t)blockIdx.x * stride + q] = total;
        }
    }
}

__global__ __launch_bounds__(kThreads) void fuse_start_kernel(const double* __restrict__ part, int blocks, int stride,
                                                              double p_target, double l2, FuseState* st) {
    __shared__ double wsum[kWaves];
    if (st->done) return;
    const int k_terms = st->k;
    const double n = (double)(st->n_tar + st->n_non);
    for (int q = 0; q < k_terms; ++q) {
        double acc = 0.0;
        for (int b = threadIdx.x; b < blocks; b += kThreads) acc += part[(size_t)b * stride + q];
        const double total = block_sum(acc, wsum);
        if (threadIdx.x == 0) {
            double sd = sqrt(total / n);
            if ((st->constant_mask >> q & 1) || !(sd > 0.0) || isinf(sd)) sd = 1.0;
            st->sd[q] = sd;
            st->inv_sd[q] = 1.0 / sd;
        }
    }
    if (threadIdx.x != 0) return;
    st->w_tar = p_target / (double)st->n_tar;
    st->w_non = (1.0 - p_target) / (double)st->n_non;
    st->tau = log(p_target) - log1p(-p_target);
    st->l2 = l2;
}

// J, the gradient and the Hessian of the data part at st->y: block partials, pass_words(K) sums.  The trial-to-thread map and
// the order in which a thread adds its trials are calib_pass_kernel's whatever K; only STAGE, the trials whose K values are in
// flight at once, falls as K grows.
template <int K>
__global__ __launch_bounds__(kThreads) void fuse_pass_kernel(const double* __restrict__ planes, const uint8_t* __restrict__ fb,
                                                             int64_t n, const FuseState* st, double* __restrict__ part, int stride) {
    constexpr int NW = pass_words(K);
    constexpr int STAGE = K <= 2 ? kItems : K <= 4 ? kItems / 2 : kItems / 4;
    __shared__ double wsum[kWaves];
    if (st->done) return;
    double mu[K], inv_sd[K], w[K];
#pragma unroll
    for (int q = 0; q < K; ++q) {
        mu[q] = st->mu[q];
        inv_sd[q] = st->inv_sd[q];
        w[q] = st->y[q];
    }
    const double bt = st->y[K] + st->tau, w_tar = st->w_tar, w_non = st->w_non;
    double acc[NW];
#pragma unroll
    for (int q = 0; q < NW; ++q) acc[q] = 0.0;
    const int64_t step = (int64_t)gridDim.x * kTile;
    for (int64_t base = (int64_t)blockIdx.x * kTile; base < n; base += step) {
#pragma unroll
        for (int k0 = 0; k0 < kItems; k0 += STAGE) {
            double f[STAGE][K];
            uint8_t bit[STAGE];
#pragma unroll
            for (int k = 0; k < STAGE; ++k) {
                const int64_t t = base + (k0 + k) * kThreads + threadIdx.x;
                bit[k] = t < n ? fb[t] : kBitVoid;
#pragma unroll
                for (int q = 0; q < K; ++q) f[k][q] = t < n ? planes[(size_t)q * (size_t)n + (size_t)t] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < STAGE; ++k) {
                if (bit[k] == kBitVoid) continue;
                const bool tar = bit[k] == 1;
                double z[K];
#pragma unroll
                for (int q = 0; q < K; ++q) z[q] = (f[k][q] - mu[q]) * inv_sd[q];
                double x = w[0] * z[0];
#pragma unroll
                for (int q = 1; q < K; ++q) x = x + w[q] * z[q];
                x = x + bt;
                const double u = tar ? -x : x;            // the term is wt softplus(u)
                const double wt = tar ? w_tar : w_non;
                const double e = exp(-fabs(u));
                const double r = 1.0 / (1.0 + e);
                const double sig = u >= 0.0 ? r : e * r;  // logistic(u)
                const double dj = tar ? -(wt * sig) : wt * sig;     // d term / d x
                const double h = wt * (e * r * r);        // d2 term / d x2
                acc[0] += wt * (fmax(u, 0.0) + log1p(e));
                double hz[K];
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    acc[1 + q] += dj * z[q];
                    hz[q] = h * z[q];
                }
                acc[1 + K] += dj;
#pragma unroll
                for (int i = 0; i < K; ++i) {
#pragma unroll
                    for (int j = 0; j <= i; ++j) acc[hess_word(K, i, j)] += hz[i] * z[j];
                }
#pragma unroll
                for (int j = 0; j < K; ++j) acc[hess_word(K, K, j)] += hz[j];
                acc[hess_word(K, K, K)] += h;
            }
        }
    }
    double* out = part + (size_t)blockIdx.x * stride;
#pragma unroll
    for (int q = 0; q < NW; ++q) {
        const double total = block_sum(acc[q], wsum);
        if (threadIdx.x == 0) out[q] = total;
    }
}

// L L^T = H + lam I over the leading m x m part (row stride kDim); with `test` it gives up (false) at the first pivot whose
// square is <= kPivotTol times its diagonal entry or not positive.
__device__ bool cholesky(const double* H, double* L, int m, double lam, bool test) {
    for (int j = 0; j < m; ++j) {
        const double hjj = H[j * kDim + j] + lam;
        double s = hjj;
        for (int p = 0; p < j; ++p) s -= L[j * kDim + p] * L[j * kDim + p];
        if (test && (!(s > kPivotTol * hjj) || !(s > 0.0))) return false;
        const double ljj = sqrt(s);
        L[j * kDim + j] = ljj;
        for (int i = j + 1; i < m; ++i) {
            double t = H[i * kDim + j];
            for (int p = 0; p < j; ++p) t -= L[i * kDim + p] * L[j * kDim + p];
            L[i * kDim + j] = t / ljj;
        }
    }
    return true;
}

__global__ __launch_bounds__(kThreads) void fuse_solve_kernel(const double* __restrict__ part, int blocks, int stride, FuseState* st) {
    __shared__ double wsum[kWaves];
    __shared__ double tot[pass_words(kMaxTerms)];
    __shared__ double H[kDim * kDim], L[kDim * kDim], gv[kDim], dv[kDim];
    __shared__ double sx[kDim], sy[kDim], sd[kDim];      // the state's x, y and d: read once, by a thread each
    __shared__ int act[kDim];
    if (st->done) return;
    const int K = st->k, words = (K + 1) * (K + 4) / 2 + 1, mask = st->constant_mask, have_x = st->have_x,
              n_iter = st->n_iter;
    const double l2 = st->l2, jx = st->jx;
    if ((int)threadIdx.x <= K) {
        sx[threadIdx.x] = st->x[threadIdx.x];
        sy[threadIdx.x] = st->y[threadIdx.x];
        sd[threadIdx.x] = st->d[threadIdx.x];
    }
    for (int q = 0; q < words; ++q) {
        double acc = 0.0;
        for (int b = threadIdx.x; b < blocks; b += kThreads) acc += part[(size_t)b * stride + q];
        const double total = block_sum(acc, wsum);      // (its barriers order sx, sy and sd for thread 0 too)
        if (threadIdx.x == 0) tot[q] = total;
    }
    if (threadIdx.x != 0) return;              // (tot: thread 0 reads back only what it wrote itself)
    st->n_iter = n_iter + 1;
    double sq = 0.0;
    for (int q = 0; q < K; ++q) sq += sy[q] * sy[q];
    const double pen = 0.5 * l2 * sq, jd = tot[0], jy = jd + pen;
    const bool accept = isfinite(jy) && (!have_x || jy <= jx + kAcceptSlack * fabs(jx));
    if (!accept) {                             // the objective rose (or left the finite range): half the step from x
        for (int q = 0; q <= K; ++q) {
            const double d = sd[q] * 0.5;
            st->d[q] = d;
            st->y[q] = sx[q] + d;
        }
        return;
    }
    for (int q = 0; q <= K; ++q) st->x[q] = sx[q] = sy[q];
    st->jx = jy;
    st->jx_data = jd;
    st->jx_pen = pen;
    st->have_x = 1;
    int m = 0;                                 // the terms that are not constant, then the bias
    for (int q = 0; q < K; ++q)
        if (!(mask >> q & 1)) act[m++] = q;
    act[m++] = K;
    double trace = 0.0;
    for (int a = 0; a < m; ++a) {
        const int i = act[a];
        gv[a] = i < K ? tot[1 + i] + l2 * sx[i] : tot[1 + i];
        for (int b = 0; b <= a; ++b) {
            const int j = act[b];
            double v = tot[1 + (K + 1) + i * (i + 1) / 2 + j];
            if (a == b && i < K) v += l2;
            H[a * kDim + b] = v;
        }
        trace += H[a * kDim + a];
    }
    if (!cholesky(H, L, m, 0.0, true)) cholesky(H, L, m, kPivotTol * trace + 1e-300, false);      // singular to working precision: damped
    for (int a = 0; a < m; ++a) {              // L v = -g
        double t = -gv[a];
        for (int p = 0; p < a; ++p) t -= L[a * kDim + p] * dv[p];
        dv[a] = t / L[a * kDim + a];
    }
    for (int a = m - 1; a >= 0; --a) {         // L^T d = v
        double t = dv[a];
        for (int p = a + 1; p < m; ++p) t -= L[p * kDim + a] * dv[p];
        dv[a] = t / L[a * kDim + a];
    }
    double big = 0.0, xmax = 0.0;
    bool finite = true;
    for (int a = 0; a < m; ++a) {
        finite = finite && isfinite(dv[a]);
        big = fmax(big, fabs(dv[a]));
        xmax = fmax(xmax, fabs(sx[act[a]]));
    }
    if (!finite) {                             // nothing left to solve with (a separable set driven to saturation)
        st->done = 1;
        return;                                // status stays XVEC_FUSE_MAX_ITER; x is the last finite point
    }
    if (big > kStepCap)
        for (int a = 0; a < m; ++a) dv[a] *= kStepCap / big;
    if (big <= XVEC_FUSE_STEP_TOL * fmax(1.0, xmax)) {
        for (int a = 0; a < m; ++a) st->x[act[a]] = sx[act[a]] + dv[a];      // the reported point; jx stays J of the point the step was taken from
        st->done = 1;
        st->status = XVEC_FUSE_CONVERGED;
        return;
    }
    for (int a = 0; a < m; ++a) {
        st->d[act[a]] = dv[a];
        st->y[act[a]] = sx[act[a]] + dv[a];
    }
}

__global__ void fuse_finish_kernel(const FuseState* st, xvec_fuse_result* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int K = st->k;
    const bool have = st->status == XVEC_FUSE_CONVERGED || (st->status == XVEC_FUSE_MAX_ITER && st->have_x);
    const bool none = st->status == XVEC_FUSE_MAX_ITER && !st->have_x;      // not one pass accepted
    double s = 0.0;
    for (int q = 0; q < kMaxTerms; ++q) {
        double w = q < K ? nan : 0.0;
        if (q < K && have) {
            w = (st->constant_mask >> q & 1) ? 0.0 : st->x[q] / st->sd[q];
            const double p = w * st->mu[q];
            s = q == 0 ? p : s + p;
        } else if (q < K && none) {
            w = 0.0;
        }
        out->w[q] = w;
    }
    out->b = have ? st->x[K] - s : none ? 0.0 : nan;
    out->objective_bits = have ? st->jx_data / kLn2 : nan;
    out->penalty_bits = have ? st->jx_pen / kLn2 : nan;
    out->n_target = st->n_tar;
    out->n_nontarget = st->n_non;
    out->n_nan = st->n_nan;
    out->n_bad_index = st->n_bad;
    out->n_terms = (int16_t)K;
    out->n_iter = (int16_t)st->n_iter;
    out->status = (int16_t)st->status;
    out->constant_mask = (uint16_t)st->constant_mask;
}

// ---------------------------------------------------------------- apply

struct ApplyArgs {
    Terms tm;
    double* out;
    int64_t ld_out, n_rows, n_cols, col_tiles;
    const xvec_fuse_result* fit;
};

__global__ __launch_bounds__(XVEC_CALIB_APPLY_COLS) void fuse_apply_kernel(const ApplyArgs g) {
    const int64_t tile_r = blockIdx.x / g.col_tiles, tile_c = blockIdx.x - tile_r * g.col_tiles;
    const int64_t j = tile_c * XVEC_CALIB_APPLY_COLS + threadIdx.x;
    if (j >= g.n_cols) return;
    const int64_t i0 = tile_r * XVEC_CALIB_APPLY_ROWS;
    double acc[XVEC_CALIB_APPLY_ROWS];
#pragma unroll
    for (int q = 0; q < kMaxTerms; ++q) {
        if (q < g.tm.k) {
            const double w = g.fit->w[q];
            double f[XVEC_CALIB_APPLY_ROWS];
#pragma unroll
            for (int r = 0; r < XVEC_CALIB_APPLY_ROWS; ++r)
                if (i0 + r < g.n_rows) f[r] = term_value(g.tm.t[q], i0 + r, j);
#pragma unroll
            for (int r = 0; r < XVEC_CALIB_APPLY_ROWS; ++r)
                if (i0 + r < g.n_rows) {
                    const double p = w * f[r];          // (rounded on its own: contraction is off in this file)
                    acc[r] = q == 0 ? p : acc[r] + p;
                }
        }
    }
    const double b = g.fit->b;
    // every cell a thread writes it has read above, in every term: out may be a MATRIX term's own data
#pragma unroll
    for (int r = 0; r < XVEC_CALIB_APPLY_ROWS; ++r)
        if (i0 + r < g.n_rows) g.out[(i0 + r) * g.ld_out + j] = acc[r] + b;
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_ferr;

int refused(const Refusal& why, bool too_large, const char* call) {
    return g_ferr.refused(too_large ? XVEC_ERR_TOO_LARGE : XVEC_ERR_ARG, why, call);
}

Terms terms_of(const xvec_fuse_term* terms, int32_t n_terms) {
    Terms tm{};
    for (int k = 0; k < n_terms; ++k) tm.t[k] = terms[k];
    tm.k = n_terms;
    return tm;
}

template <int K>
int launch_pass(unsigned grid, hipStream_t s, const double* planes, const uint8_t* fb, int64_t n, const FuseState* st, double* part,
                int stride) {
    fuse_pass_kernel<K><<<grid, kThreads, 0, s>>>(planes, fb, n, st, part, stride);
    return g_ferr.launch_ok("fuse_pass_kernel");
}

int fit(const TrialArgs& g, const Terms& tm, bool all_pairs, double p_target, double l2, int32_t max_iter, xvec_fuse_result* out,
        void* workspace, size_t workspace_bytes, xvec_stream stream, const char* call) {
    Refusal why;
    if (check_fit(p_target, max_iter, why) || check_ridge(l2, why)) return refused(why, false, call);
    if (!out) return g_ferr.fail(XVEC_ERR_ARG, "%s: null pointer: out", call);
    const Layout lay = make_layout(g.n, tm.k);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, lay.total, g_ferr))) return rc;
    FuseState* st = part<FuseState>(workspace, lay.state);
    double* partials = part<double>(workspace, lay.partials);
    double* planes = part<double>(workspace, lay.planes);
    uint8_t* bits = part<uint8_t>(workspace, lay.fit_bits);
    const int stride = partial_stride(tm.k);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)pass_blocks(g.n);
    if (all_pairs) fuse_gather_kernel<true><<<grid, kThreads, 0, s>>>(g, tm, planes, bits, partials, stride);
    else fuse_gather_kernel<false><<<grid, kThreads, 0, s>>>(g, tm, planes, bits, partials, stride);
    if ((rc = g_ferr.launch_ok("fuse_gather_kernel"))) return rc;
    fuse_mean_kernel<<<1, kThreads, 0, s>>>(partials, (int)grid, stride, tm.k, st);
    if ((rc = g_ferr.launch_ok("fuse_mean_kernel"))) return rc;
    fuse_var_kernel<<<grid, kThreads, 0, s>>>(planes, bits, g.n, tm.k, st, partials, stride);
    if ((rc = g_ferr.launch_ok("fuse_var_kernel"))) return rc;
    fuse_start_kernel<<<1, kThreads, 0, s>>>(partials, (int)grid, stride, p_target, l2, st);
    if ((rc = g_ferr.launch_ok("fuse_start_kernel"))) return rc;
    for (int it = 0; it < max_iter; ++it) {
        switch (tm.k) {
            case 1: rc = launch_pass<1>(grid, s, planes, bits, g.n, st, partials, stride); break;
            case 2: rc = launch_pass<2>(grid, s, planes, bits, g.n, st, partials, stride); break;
            case 3: rc = launch_pass<3>(grid, s, planes, bits, g.n, st, partials, stride); break;
            case 4: rc = launch_pass<4>(grid, s, planes, bits, g.n, st, partials, stride); break;
            case 5: rc = launch_pass<5>(grid, s, planes, bits, g.n, st, partials, stride); break;
            case 6: rc = launch_pass<6>(grid, s, planes, bits, g.n, st, partials, stride); break;
            case 7: rc = launch_pass<7>(grid, s, planes, bits, g.n, st, partials, stride); break;
            default: rc = launch_pass<8>(grid, s, planes, bits, g.n, st, partials, stride); break;
        }
        if (rc) return rc;
        fuse_solve_kernel<<<1, kThreads, 0, s>>>(partials, (int)grid, stride, st);
        if ((rc = g_ferr.launch_ok("fuse_solve_kernel"))) return rc;
    }
    fuse_finish_kernel<<<1, 64, 0, s>>>(st, out);
    return g_ferr.launch_ok("fuse_finish_kernel");
}

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_fuse_last_error(void) { return g_ferr.c_str(); }

size_t xvec_fuse_workspace_bytes(int64_t n_trials, int32_t n_terms) { return make_layout(n_trials, n_terms).total; }

int xvec_fuse_fit(const xvec_fuse_term* terms, int32_t n_terms, int64_t n_rows, int64_t n_cols, const int32_t* row_idx,
                  const int32_t* col_idx, const uint8_t* is_target, int64_t n_trials, double p_target, double l2,
                  int32_t max_iter, xvec_fuse_result* out, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    Refusal why;
    bool too_large;
    if (check_fit_trials(terms, n_terms, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, why, &too_large))
        return refused(why, too_large, "xvec_fuse_fit");
    return fit(trial_args(nullptr, 0, n_rows, n_cols, row_idx, col_idx, is_target, n_trials, 0), terms_of(terms, n_terms), false,
               p_target, l2, max_iter, out, workspace, workspace_bytes, stream, "xvec_fuse_fit");
}

int xvec_fuse_fit_all_pairs(const xvec_fuse_term* terms, int32_t n_terms, int64_t n_rows, int64_t n_cols,
                            const int32_t* row_class, const int32_t* col_class, int32_t skip_diagonal, double p_target,
                            double l2, int32_t max_iter, xvec_fuse_result* out, void* workspace, size_t workspace_bytes,
                            xvec_stream stream) {
    Refusal why;
    bool too_large;
    if (check_fit_all_pairs(terms, n_terms, n_rows, n_cols, row_class, col_class, why, &too_large))
        return refused(why, too_large, "xvec_fuse_fit_all_pairs");
    return fit(trial_args(nullptr, 0, n_rows, n_cols, row_class, col_class, nullptr, n_rows * n_cols, skip_diagonal != 0),
               terms_of(terms, n_terms), true, p_target, l2, max_iter, out, workspace, workspace_bytes, stream,
               "xvec_fuse_fit_all_pairs");
}

int xvec_fuse_apply(const xvec_fuse_term* terms, int32_t n_terms, int64_t n_rows, int64_t n_cols, const xvec_fuse_result* fit_record,
                    double* out, int64_t ld_out, xvec_stream stream) {
    Refusal why;
    bool too_large;
    if (check_fuse_apply(terms, n_terms, n_rows, n_cols, fit_record, out, ld_out, why, &too_large))
        return refused(why, too_large, "xvec_fuse_apply");
    ApplyArgs g{};
    g.tm = terms_of(terms, n_terms);
    g.out = out;
    g.ld_out = ld_out;
    g.n_rows = n_rows;
    g.n_cols = n_cols;
    g.col_tiles = apply_col_tiles(n_cols);
    g.fit = fit_record;
    fuse_apply_kernel<<<(unsigned)apply_tiles(n_rows, n_cols), XVEC_CALIB_APPLY_COLS, 0, static_cast<hipStream_t>(stream)>>>(g);
    return g_ferr.launch_ok("fuse_apply_kernel");
}

}  // extern "C"
