// Exact t-SNE, fp64: squared distances, scikit-learn's perplexity search and joint probabilities, and the gradient-descent
// iterations on the KL divergence (two launches each).  C ABI, the arithmetic and the order of every sum: include/xvec_tsne.h.
//   reference: plda_score_stat.py plot_images -> sklearn.manifold.TSNE(2) (Barnes-Hut there; the exact method here)
// The checks, the workspace layout and the pair pass's plan are csrc/tsne_plan.h (host only).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/xvec_hip.h"
#include "../../include/xvec_score.h"
#include "../../include/xvec_tsne.h"
#include "host_support.h"
#include "tsne_plan.h"

// every operation is rounded on its own: the sums below have the order the header states, and the two forms of the pair pass
// (16-byte and 8-byte loads of P) give the same bits
#pragma clang fp contract(off)

namespace xvec {
namespace {

constexpr int kThreads = XVEC_TSNE_THREADS;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 32;      // the symmetrising kernel's tile

// lane[l] += lane[l ^ stride], stride = 32 .. 1: every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// The block's sum of v: the lanes of a wave as above, the four waves added in order.  Every thread gets it.  `red` is kWaves
// doubles of LDS, free again when the call returns.
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += red[w];
    __syncthreads();
    return s;
}

// ---------------------------------------------------------------- squared distances

// A wave per row: the row widened to fp64, and the sum of its squares.
template <typename T>
__global__ __launch_bounds__(kThreads) void tsne_widen_kernel(const T* __restrict__ x, int n, int d, int64_t ldx,
                                                              double* __restrict__ x64, double* __restrict__ sqnorm) {
    const int i = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const T* row = x + (int64_t)i * ldx;
    double* out = x64 + (int64_t)i * d;
    double acc = 0.0;
    for (int c = lane; c < d; c += 64) {
        const double v = (double)row[c];
        out[c] = v;
        acc += v * v;
    }
    acc = wave_sum(acc);
    if (lane == 0) sqnorm[i] = acc;
}

// d2 holds the Gram matrix; in place: (-2 g + |x_i|^2) + |x_j|^2, clamped at 0, the diagonal 0, rounded to float32 if asked.
__global__ __launch_bounds__(kThreads) void tsne_sqdist_kernel(double* __restrict__ d2, int64_t ldd, int n,
                                                               const double* __restrict__ sqnorm, int round_f32) {
    const int i = blockIdx.y, j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    double* at = d2 + (int64_t)i * ldd + j;
    double v = (-2.0 * *at + sqnorm[i]) + sqnorm[j];
    v = v < 0.0 ? 0.0 : v;          // (a NaN stays one, as in numpy's maximum)
    if (i == j) v = 0.0;
    if (round_f32) v = (double)(float)v;
    *at = v;
}

// ---------------------------------------------------------------- affinities

// A block per row.  Thread t keeps the distances of columns t, t + 256, ... in registers for all the steps of the search.
template <int ITEMS>
__global__ __launch_bounds__(kThreads) void tsne_affinity_kernel(const double* __restrict__ d2, int64_t ldd, int n,
                                                                 double log_perplexity, double* __restrict__ p, int64_t ldp,
                                                                 double* __restrict__ betas, double* __restrict__ row_sum) {
    __shared__ double red[2][kWaves][2];
    __shared__ double red_row[kWaves];
    const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double* row = d2 + (int64_t)i * ldd;
    double dist[ITEMS];
    uint32_t valid = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int j = t + k * kThreads;
        const bool ok = j < n && j != i;
        dist[k] = ok ? row[j] : 0.0;
        valid |= (uint32_t)ok << k;
    }
    const double floor_sum = (double)1e-8f, tolerance = (double)1e-5f;      // scikit-learn's `cdef float` constants
    double beta = 1.0, lo = -INFINITY, hi = INFINITY, used = 1.0, S = 1.0;
    for (int step = 0; step < XVEC_TSNE_SEARCH_STEPS; ++step) {
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const double e = (valid >> k & 1u) ? exp(-dist[k] * beta) : 0.0;
            s1 += e;
            s2 += dist[k] * e;
        }
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        double(*buf)[2] = red[step & 1];      // two buffers: a wave may enter the next step while another still reads this one
        if (lane == 0) {
            buf[wave][0] = s1;
            buf[wave][1] = s2;
        }
        __syncthreads();
        s1 = buf[0][0];
        s2 = buf[0][1];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            s1 += buf[w][0];
            s2 += buf[w][1];
        }
        if (s1 == 0.0) s1 = floor_sum;
        used = beta;
        S = s1;
        const double diff = (log(s1) + beta * (s2 / s1)) - log_perplexity;
        if (fabs(diff) <= tolerance) break;      // the same bits in every thread: the whole block leaves together
        if (diff > 0.0) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
        } else {
            hi = beta;
            beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
        }
    }
    double acc = 0.0;
    double* out = p + (int64_t)i * ldp;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int j = t + k * kThreads;
        const double c = (valid >> k & 1u) ? exp(-dist[k] * used) / S : 0.0;
        if (j < n) out[j] = c;
        acc += c;
    }
    acc = block_sum(acc, red_row);
    if (t == 0) {
        row_sum[i] = acc;
        if (betas) betas[i] = used;
    }
}

// One block: out[0] = the sum of v[0 .. n - 1], thread t adding t, t + 256, ... ascending.
__global__ __launch_bounds__(kThreads) void tsne_total_kernel(const double* __restrict__ v, int n, double* __restrict__ out) {
    __shared__ double red[kWaves];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads) acc += v[i];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) out[0] = acc;
}

// In place, a block per pair of mirrored 32 x 32 tiles (bi <= bj): P = max((C + C^T) / max(2 sum C, eps), eps), 0 on the diagonal.
__global__ __launch_bounds__(kThreads) void tsne_symmetrize_kernel(double* __restrict__ p, int64_t ldp, int n,
                                                                   const double* __restrict__ total) {
    __shared__ double a[kTile][kTile + 1], b[kTile][kTile + 1];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
    const int r0 = bi * kTile, c0 = bj * kTile;
    for (int r = ty; r < kTile; r += kThreads / kTile) {
        const bool in_a = r0 + r < n && c0 + tx < n, in_b = c0 + r < n && r0 + tx < n;
        a[r][tx] = in_a ? p[(int64_t)(r0 + r) * ldp + c0 + tx] : 0.0;
        b[r][tx] = in_b ? p[(int64_t)(c0 + r) * ldp + r0 + tx] : 0.0;
    }
    __syncthreads();
    const double two = 2.0 * total[0];
    const double denom = two > DBL_EPSILON ? two : DBL_EPSILON;
    for (int r = ty; r < kTile; r += kThreads / kTile) {
        if (r0 + r < n && c0 + tx < n) {
            const double v = (a[r][tx] + b[tx][r]) / denom;
            p[(int64_t)(r0 + r) * ldp + c0 + tx] = r0 + r == c0 + tx ? 0.0 : (v > DBL_EPSILON ? v : DBL_EPSILON);
        }
        if (bi != bj && c0 + r < n && r0 + tx < n) {
            const double v = (b[r][tx] + a[tx][r]) / denom;
            p[(int64_t)(c0 + r) * ldp + r0 + tx] = v > DBL_EPSILON ? v : DBL_EPSILON;
        }
    }
}

// ---------------------------------------------------------------- iterations

struct StepArgs {
    const double* p;
    int64_t ldp, ldy;
    double *y, *update, *gains;
    int n, rows, slices, slice_cols;
    double exaggeration, momentum, learning_rate, min_gain;
    double *partials, *kl_part, *norm_part, *scalars;      // workspace
};

// What a wave does with its row's share of a slice: lane l walks the slice's columns 2l, 2l + 1, 2l + 128, 2l + 129, ...
// VEC reads the two neighbours as one 16-byte load (the caller has checked the alignment).
template <bool VEC>
__device__ __forceinline__ void load_pair(const double* at, bool second, double& p0, double& p1) {
    if (VEC && second) {
        const double2 v = *reinterpret_cast<const double2*>(at);
        p0 = v.x;
        p1 = v.y;
    } else {
        p0 = at[0];
        p1 = second ? at[1] : 0.0;
    }
}

// The pair pass: block (slice, group).  The five sums of every (row, slice) go to partials[slice][row][5]:
// attraction x, y; repulsion numerator x, y; sum of w.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void tsne_pair_kernel(const StepArgs g) {
    __shared__ double2 ys[XVEC_TSNE_SLICE_MAX];
    const int slice = blockIdx.x, group = blockIdx.y;
    const int c0 = slice * g.slice_cols;
    const int cw = min(g.n - c0, g.slice_cols);
    for (int q = threadIdx.x; q < cw; q += kThreads) {
        const double* yj = g.y + (int64_t)(c0 + q) * g.ldy;
        ys[q] = make_double2(yj[0], yj[1]);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < g.rows; r += kWaves) {
        const int i = group * g.rows + r;
        if (i >= g.n) break;
        const double yi0 = g.y[(int64_t)i * g.ldy], yi1 = g.y[(int64_t)i * g.ldy + 1];
        const double* prow = g.p + (int64_t)i * g.ldp + c0;
        double ax = 0.0, ay = 0.0, rx = 0.0, ry = 0.0, sw = 0.0;
#pragma unroll 4
        for (int q = 2 * lane; q < cw; q += XVEC_TSNE_SLICE_STEP) {
            const bool second = q + 1 < cw;
            double p0, p1;
            load_pair<VEC>(prow + q, second, p0, p1);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (h == 1 && !second) break;
                const double2 yj = ys[q + h];
                const double dx = yi0 - yj.x, dy = yi1 - yj.y;
                const double w = 1.0 / (1.0 + (dx * dx + dy * dy));
                const double pw = (g.exaggeration * (h ? p1 : p0)) * w;
                const double ww = w * w;
                ax += pw * dx;
                ay += pw * dy;
                rx += ww * dx;
                ry += ww * dy;
                sw += c0 + q + h == i ? 0.0 : w;      // (the self term's other four sums are exact zeros)
            }
        }
        ax = wave_sum(ax);
        ay = wave_sum(ay);
        rx = wave_sum(rx);
        ry = wave_sum(ry);
        sw = wave_sum(sw);
        if (lane == 0) {
            double* out = g.partials + ((int64_t)slice * g.n + i) * 5;
            out[0] = ax;
            out[1] = ay;
            out[2] = rx;
            out[3] = ry;
            out[4] = sw;
        }
    }
}

// Z = sum_i (sum_s partials[s][i][4]): a row's slices in order, thread t the rows t, t + 256, ... ascending, then block_sum.
__device__ __forceinline__ double sum_of_w(const StepArgs& g, double* red) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < g.n; i += kThreads) {
        double r = 0.0;
        for (int s = 0; s < g.slices; ++s) r += g.partials[((int64_t)s * g.n + i) * 5 + 4];
        acc += r;
    }
    return block_sum(acc, red);
}

// The update: a thread per row.  Every block forms Z for itself (the same bits in each).
__global__ __launch_bounds__(kThreads) void tsne_update_kernel(const StepArgs g) {
    __shared__ double red[kWaves];
    const double Z = sum_of_w(g, red);
    const int i = blockIdx.x * kThreads + threadIdx.x;
    double grad[2] = {0.0, 0.0};
    if (i < g.n) {
        double a[2] = {0.0, 0.0}, rep[2] = {0.0, 0.0};
        for (int s = 0; s < g.slices; ++s) {
            const double* part = g.partials + ((int64_t)s * g.n + i) * 5;
            a[0] += part[0];
            a[1] += part[1];
            rep[0] += part[2];
            rep[1] += part[3];
        }
        grad[0] = 4.0 * (a[0] - rep[0] / Z);
        grad[1] = 4.0 * (a[1] - rep[1] / Z);
    }
    const double sq = block_sum(grad[0] * grad[0] + grad[1] * grad[1], red);
    if (threadIdx.x == 0) g.norm_part[blockIdx.x] = sq;
    if (i >= g.n) return;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int64_t at = (int64_t)i * g.ldy + c;
        double u = g.update[at], gain = g.gains[at];
        gain = u * grad[c] < 0.0 ? gain + 0.2 : gain * 0.8;
        gain = gain > g.min_gain ? gain : g.min_gain;
        u = g.momentum * u - g.learning_rate * (grad[c] * gain);
        g.update[at] = u;
        g.gains[at] = gain;
        g.y[at] += u;
    }
}

// One block: scalars[1] = Z, for the KL pass.
__global__ __launch_bounds__(kThreads) void tsne_z_kernel(const StepArgs g) {
    __shared__ double red[kWaves];
    const double Z = sum_of_w(g, red);
    if (threadIdx.x == 0) g.scalars[1] = Z;
}

// The KL pass, on the pair pass's grid and walk: kl_part[slice][row] = the sum over the slice's columns j > row of
// cP log(max(cP, eps) / max(w / Z, eps)).
template <bool VEC>
__global__ __launch_bounds__(kThreads) void tsne_kl_kernel(const StepArgs g) {
    __shared__ double2 ys[XVEC_TSNE_SLICE_MAX];
    const int slice = blockIdx.x, group = blockIdx.y;
    const int c0 = slice * g.slice_cols;
    const int cw = min(g.n - c0, g.slice_cols);
    for (int q = threadIdx.x; q < cw; q += kThreads) {
        const double* yj = g.y + (int64_t)(c0 + q) * g.ldy;
        ys[q] = make_double2(yj[0], yj[1]);
    }
    __syncthreads();
    const double Z = g.scalars[1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < g.rows; r += kWaves) {
        const int i = group * g.rows + r;
        if (i >= g.n) break;
        const double yi0 = g.y[(int64_t)i * g.ldy], yi1 = g.y[(int64_t)i * g.ldy + 1];
        const double* prow = g.p + (int64_t)i * g.ldp + c0;
        double kl = 0.0;
        if (c0 + cw - 1 > i) {      // (wave-uniform) the slice has columns past the row
#pragma unroll 4
            for (int q = 2 * lane; q < cw; q += XVEC_TSNE_SLICE_STEP) {
                const bool second = q + 1 < cw;
                double p0, p1;
                load_pair<VEC>(prow + q, second, p0, p1);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (h == 1 && !second) break;
                    if (c0 + q + h <= i) continue;
                    const double2 yj = ys[q + h];
                    const double dx = yi0 - yj.x, dy = yi1 - yj.y;
                    const double w = 1.0 / (1.0 + (dx * dx + dy * dy));
                    const double cp = g.exaggeration * (h ? p1 : p0);
                    const double qq = w / Z;
                    kl += cp * log((cp > DBL_EPSILON ? cp : DBL_EPSILON) / (qq > DBL_EPSILON ? qq : DBL_EPSILON));
                }
            }
        }
        kl = wave_sum(kl);
        if (lane == 0) g.kl_part[(int64_t)slice * g.n + i] = kl;
    }
}

// One block, after the last update: kl_out = 2 sum_i (sum_s kl_part[s][i]), grad_norm_out = sqrt(sum_b norm_part[b]).
__global__ __launch_bounds__(kThreads) void tsne_finish_kernel(const StepArgs g, int blocks, double* __restrict__ kl_out,
                                                               double* __restrict__ grad_norm_out) {
    __shared__ double red[kWaves];
    if (kl_out) {
        double acc = 0.0;
        for (int i = threadIdx.x; i < g.n; i += kThreads) {
            double r = 0.0;
            for (int s = 0; s < g.slices; ++s) r += g.kl_part[(int64_t)s * g.n + i];
            acc += r;
        }
        acc = block_sum(acc, red);
        if (threadIdx.x == 0) kl_out[0] = 2.0 * acc;
    }
    if (grad_norm_out) {
        double acc = 0.0;
        for (int b = threadIdx.x; b < blocks; b += kThreads) acc += g.norm_part[b];
        acc = block_sum(acc, red);
        if (threadIdx.x == 0) grad_norm_out[0] = sqrt(acc);
    }
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_terr;

}  // namespace
}  // namespace xvec

using namespace xvec;
namespace tp = xvec::tsne_plan;

extern "C" {

const char* xvec_tsne_last_error(void) { return g_terr.c_str(); }

size_t xvec_tsne_workspace_bytes(int32_t n, int32_t d) {
    if (n < 2 || n > XVEC_TSNE_MAX_POINTS || d < 0 || d > XVEC_TSNE_MAX_DIM) return 0;
    return tp::make_layout(n, d).total;
}

int xvec_tsne_plan(int32_t n, int32_t cus, int32_t* rows_per_block, int32_t* slices, int32_t* slice_cols) {
    const char* what = "xvec_tsne_plan";
    Refusal why;
    if (tp::check_points(n, why)) return g_terr.refused(XVEC_ERR_ARG, why, what);
    if (!rows_per_block || !slices || !slice_cols) return g_terr.fail(XVEC_ERR_ARG, "%s: null pointer", what);
    const tp::Plan p = tp::make_plan(n, cus < 1 ? device_cu_count() : cus);
    *rows_per_block = p.rows;
    *slices = p.slices;
    *slice_cols = p.slice_cols;
    return XVEC_OK;
}

// Launches: the widening, the Gram product (xvec_gemm_nt_f64's kernel), the epilogue.
int xvec_tsne_sqdist(const void* x, int32_t x_dtype, int32_t n, int32_t d, int64_t ldx, int32_t round_f32, double* d2,
                     int64_t ldd, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    const char* what = "xvec_tsne_sqdist";
    Refusal why;
    if (tp::check_points(n, why) || tp::check_x(x, x_dtype, d, ldx, why) || tp::check_matrix(d2, ldd, n, "d2", why))
        return g_terr.refused(XVEC_ERR_ARG, why, what);
    const tp::Layout l = tp::make_layout(n, d);
    if (const int rc = workspace_arg_ok(workspace, workspace_bytes, l.total, g_terr, XVEC_ERR_WORKSPACE, what, 8)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* x64 = part<double>(workspace, l.x64);
    double* sqnorm = part<double>(workspace, l.sqnorm);
    const unsigned row_blocks = (unsigned)tp::ceil_div(n, kWaves);
    if (x_dtype == XVEC_TSNE_X_F32) tsne_widen_kernel<float><<<row_blocks, kThreads, 0, s>>>(static_cast<const float*>(x), n, d, ldx, x64, sqnorm);
    else tsne_widen_kernel<double><<<row_blocks, kThreads, 0, s>>>(static_cast<const double*>(x), n, d, ldx, x64, sqnorm);
    if (const int rc = g_terr.launch_ok("tsne_widen_kernel")) return rc;
    if (const int rc = xvec_gemm_nt_f64(x64, d, x64, d, n, n, d, nullptr, nullptr, 0.0, 1.0, d2, ldd, stream))
        return g_terr.fail(rc, "%s: the Gram product: %s", what, xvec_score_last_error());
    tsne_sqdist_kernel<<<dim3((unsigned)tp::ceil_div(n, kThreads), (unsigned)n), kThreads, 0, s>>>(d2, ldd, n, sqnorm, round_f32 != 0);
    return g_terr.launch_ok("tsne_sqdist_kernel");
}

// Launches: the rows' searches, the sum of C, the symmetrising.
int xvec_tsne_affinities(const double* d2, int64_t ldd, int32_t n, double perplexity, double* p, int64_t ldp, double* betas,
                         void* workspace, size_t workspace_bytes, xvec_stream stream) {
    const char* what = "xvec_tsne_affinities";
    Refusal why;
    if (tp::check_points(n, why) || tp::check_perplexity(perplexity, n, why) || tp::check_matrix(d2, ldd, n, "d2", why) ||
        tp::check_matrix(p, ldp, n, "p", why))
        return g_terr.refused(XVEC_ERR_ARG, why, what);
    if (betas && reinterpret_cast<uintptr_t>(betas) % 8 != 0) return g_terr.fail(XVEC_ERR_ARG, "%s: betas is not 8-byte aligned", what);
    const tp::Layout l = tp::make_layout(n, 0);
    if (const int rc = workspace_arg_ok(workspace, workspace_bytes, l.total, g_terr, XVEC_ERR_WORKSPACE, what, 8)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* row_sum = part<double>(workspace, l.row_sum);
    double* scalars = part<double>(workspace, l.scalars);
    const double log_perplexity = std::log(perplexity);
    if (n <= 8 * kThreads) tsne_affinity_kernel<8><<<(unsigned)n, kThreads, 0, s>>>(d2, ldd, n, log_perplexity, p, ldp, betas, row_sum);
    else tsne_affinity_kernel<XVEC_TSNE_ROW_ITEMS><<<(unsigned)n, kThreads, 0, s>>>(d2, ldd, n, log_perplexity, p, ldp, betas, row_sum);
    if (const int rc = g_terr.launch_ok("tsne_affinity_kernel")) return rc;
    tsne_total_kernel<<<1, kThreads, 0, s>>>(row_sum, n, scalars);
    if (const int rc = g_terr.launch_ok("tsne_total_kernel")) return rc;
    const unsigned tiles = (unsigned)tp::ceil_div(n, kTile);
    tsne_symmetrize_kernel<<<dim3(tiles, tiles), kThreads, 0, s>>>(p, ldp, n, scalars);
    return g_terr.launch_ok("tsne_symmetrize_kernel");
}

// Launches per iteration: the pair pass, the update.  In the last one, with kl_out: Z and the KL pass between the two.  With
// kl_out or grad_norm_out: the finish, once.
int xvec_tsne_steps(const double* p, int64_t ldp, int32_t n, int32_t n_components, double* y, double* update, double* gains,
                    int64_t ldy, int32_t n_steps, double exaggeration, double momentum, double learning_rate, double min_gain,
                    double* kl_out, double* grad_norm_out, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    const char* what = "xvec_tsne_steps";
    Refusal why;
    if (tp::check_points(n, why) || tp::check_steps(n_components, n_steps, exaggeration, momentum, learning_rate, min_gain, why) ||
        tp::check_matrix(p, ldp, n, "p", why) || tp::check_matrix(y, ldy, 2, "y", why) ||
        tp::check_matrix(update, ldy, 2, "update", why) || tp::check_matrix(gains, ldy, 2, "gains", why))
        return g_terr.refused(XVEC_ERR_ARG, why, what);
    if ((kl_out && reinterpret_cast<uintptr_t>(kl_out) % 8 != 0) || (grad_norm_out && reinterpret_cast<uintptr_t>(grad_norm_out) % 8 != 0))
        return g_terr.fail(XVEC_ERR_ARG, "%s: kl_out or grad_norm_out is not 8-byte aligned", what);
    const tp::Layout l = tp::make_layout(n, 0);
    if (const int rc = workspace_arg_ok(workspace, workspace_bytes, l.total, g_terr, XVEC_ERR_WORKSPACE, what, 8)) return rc;
    const tp::Plan plan = tp::make_plan(n, device_cu_count());
    hipStream_t s = static_cast<hipStream_t>(stream);
    StepArgs g{};
    g.p = p; g.ldp = ldp; g.ldy = ldy; g.y = y; g.update = update; g.gains = gains;
    g.n = n; g.rows = plan.rows; g.slices = plan.slices; g.slice_cols = plan.slice_cols;
    g.exaggeration = exaggeration; g.momentum = momentum; g.learning_rate = learning_rate; g.min_gain = min_gain;
    g.partials = part<double>(workspace, l.partials);
    g.kl_part = part<double>(workspace, l.kl_part);
    g.norm_part = part<double>(workspace, l.norm_part);
    g.scalars = part<double>(workspace, l.scalars);
    // a row's slice starts slice_cols (even) doubles into the row: 16-byte loads need an even stride and an aligned base
    const bool vec = ldp % 2 == 0 && reinterpret_cast<uintptr_t>(p) % 16 == 0;
    const dim3 pair_grid((unsigned)plan.slices, (unsigned)plan.groups);
    const unsigned blocks = (unsigned)tp::update_blocks(n);
    for (int32_t it = 0; it < n_steps; ++it) {
        if (vec) tsne_pair_kernel<true><<<pair_grid, kThreads, 0, s>>>(g);
        else tsne_pair_kernel<false><<<pair_grid, kThreads, 0, s>>>(g);
        if (const int rc = g_terr.launch_ok("tsne_pair_kernel")) return rc;
        if (kl_out && it == n_steps - 1) {
            tsne_z_kernel<<<1, kThreads, 0, s>>>(g);
            if (const int rc = g_terr.launch_ok("tsne_z_kernel")) return rc;
            if (vec) tsne_kl_kernel<true><<<pair_grid, kThreads, 0, s>>>(g);
            else tsne_kl_kernel<false><<<pair_grid, kThreads, 0, s>>>(g);
            if (const int rc = g_terr.launch_ok("tsne_kl_kernel")) return rc;
        }
        tsne_update_kernel<<<blocks, kThreads, 0, s>>>(g);
        if (const int rc = g_terr.launch_ok("tsne_update_kernel")) return rc;
    }
    if (kl_out || grad_norm_out) {
        tsne_finish_kernel<<<1, kThreads, 0, s>>>(g, (int)blocks, kl_out, grad_norm_out);
        return g_terr.launch_ok("tsne_finish_kernel");
    }
    return XVEC_OK;
}

}  // extern "C"
