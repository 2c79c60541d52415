// VBx, diarization's refinement step: a Bayesian HMM over a recording's x-vectors, run by variational Bayes from the labels
// the clustering left.  C ABI, the algorithm and its rules: include/xvec_vbx.h; the host-only half (checks, workspace layout,
// launch plan): vbx_plan.h.
//   init     a thread per row: gamma from the labels, pi uniform.
//   run      one block per recording, persistent over ALL its iterations; the stop test runs in the block.  An iteration:
//              1. gamma^T rho [S, D + 1] on v_mfma_f64_16x16x4_f64: a wave per 16 columns of rho, the T-sum in frame order,
//                 four frames an instruction; the column of ones behind rho makes the last column N_s;
//              2. a wave per speaker turns its row into alpha and folds the speaker's two constants (the emission's and the
//                 ELBO's) over the dimensions: lanes stride the row, then a butterfly;
//              3. rho alpha^T [T, S] on the matrix pipe: a wave per 16 frames, the D-sum in order; the epilogue adds the
//                 constants;
//              4. a thread per frame: the row maximum over the live speakers and b = exp(logp - max);
//              5. wave 0 walks the forward and the backward recurrence with a lane per speaker: one butterfly over the
//                 speakers per frame, the rows of b (and backwards of a and c) loaded XVEC_VBX_PREFETCH frames ahead;
//              6. tll = sum_t (log c_t + max_t): a thread per stride of frames, then a tree over the block; the ELBO.
//            Operands stream from the workspace (L2): rho of a long recording does not fit LDS and need not.
// Every loop's trip count is fixed by T, S, D and max_iter when the block starts.  No block waits on another, there are no
// flags and no grid sync; every index is derived from a loop counter, never from data, except the raw label, which the block
// wrote itself from a loop counter below S.  The one LDS atomic is an integer minimum (a speaker's first frame).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <limits>

#include "../../include/xvec_hip.h"
#include "../../include/xvec_vbx.h"
#include "host_support.h"
#include "vbx_plan.h"

namespace xvec {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = XVEC_VBX_THREADS;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxSpk = XVEC_VBX_MAX_SPEAKERS;
constexpr int kMaxDim = XVEC_VBX_MAX_DIM;
constexpr int kMaxFrames = XVEC_VBX_MAX_FRAMES;
constexpr int kPF = XVEC_VBX_PREFETCH;
constexpr int kSpkTiles = kMaxSpk / 16;
constexpr double kLog2Pi = 1.8378770664093453;      // log(2 pi)
static_assert(kMaxSpk == 64 && kThreads % 64 == 0 && (kThreads & (kThreads - 1)) == 0, "a lane per speaker, whole waves, a tree");

struct VbxArgs {
    const double* X;
    int64_t ldx;
    int dim;
    const double* phi;
    const int64_t* rec_start;      // the workspace copy
    int n_spk;
    double loop_prob, Fa, Fb, epsilon;
    int max_iter;
    double* gamma;
    int64_t ldg;
    double* pi;
    double* elbo;
    int* iters;
    int* labels;                   // may be null
    int* n_speakers;               // may be null
    double* rho;                   // the workspace's parts (vbx_plan.h)
    double* g;
    double* em;
    double* fw;
    double* c;
    double* mx;
    int* raw;
    double* model;
};

__device__ __forceinline__ bool finite(double v) { return v * 0.0 == 0.0; }

// The value of another lane of the row of 16, by a DPP move of either half (no LDS crossbar): quad_perm [1, 0, 3, 2] = 0xB1,
// quad_perm [2, 3, 0, 1] = 0x4E, row_half_mirror = 0x141, row_mirror = 0x140.
template <int CTRL>
__device__ __forceinline__ double row_peer(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// The sum of the wave's first `span` lanes (a power of two), in every one of them: a butterfly, whose pairs add the same two
// values in either lane, so all `span` lanes hold one bit pattern.  Inside a row of 16 the partner comes by DPP: the lane next
// door, the pair next door, then the mirrored lane of the other quad and of the other half, whose sums are already equal
// across their lanes.  Only the stages over 16 and 32 lanes cross the LDS crossbar.
__device__ __forceinline__ double wave_sum(double v, int span) {
    if (span > 1) v += row_peer<0xB1>(v);
    if (span > 2) v += row_peer<0x4E>(v);
    if (span > 4) v += row_peer<0x141>(v);
    if (span > 8) v += row_peer<0x140>(v);
    if (span > 16) v += __shfl_xor(v, 16);
    if (span > 32) v += __shfl_xor(v, 32);
    return v;
}

// ---------------------------------------------------------------- the initial assignment

__global__ __launch_bounds__(kThreads) void vbx_init_kernel(const int* __restrict__ labels, int64_t n_frames, int n_rec, int n_spk,
                                                            double on, double off, double uniform, double* __restrict__ gamma,
                                                            int64_t ldg, double* __restrict__ pi) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n_frames) {
        const int lab = labels[i];
        const bool known = lab >= 0 && lab < n_spk;
        for (int s = 0; s < n_spk; ++s) gamma[i * ldg + s] = known ? (s == lab ? on : off) : uniform;
    }
    if (i < n_rec)
        for (int s = 0; s < n_spk; ++s) pi[i * n_spk + s] = uniform;
}

// ---------------------------------------------------------------- the iterations

__global__ __launch_bounds__(kThreads) void vbx_run_kernel(const VbxArgs a) {
    __shared__ double sSq[kMaxDim];        // sqrt(phi)
    __shared__ double sPi[kMaxSpk];        // pi on entry to the iteration (0 behind the last speaker)
    __shared__ double sK[kMaxSpk];         // -0.5 sum_d (invL_sd + alpha_sd^2) phi_d
    __shared__ double sE[kMaxSpk];         // sum_d (log invL_sd - invL_sd - alpha_sd^2 + 1)
    __shared__ double sRed[kThreads];
    __shared__ int sFirst[kMaxSpk];        // the first frame that carries the raw label
    __shared__ int sNew[kMaxSpk];          // the raw label's number in the order of first appearance
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int r = (int)blockIdx.x;
    const int64_t start = a.rec_start[r];
    const int T = (int)(a.rec_start[r + 1] - start);
    const int S = a.n_spk, D = a.dim, Dp = D + 1;
    if (T < 1 || T > kMaxFrames || S < 1 || S > kMaxSpk || D < 1 || D > kMaxDim) return;      // never, behind the host's checks
    const int ST = (S + 15) / 16, DT = (Dp + 15) / 16, TT = (T + 15) / 16;
    int span = 1;
    while (span < S) span <<= 1;
    const double* __restrict__ X = a.X + start * a.ldx;
    double* gam = a.gamma + start * a.ldg;
    const int64_t ldg = a.ldg;
    double* rho = a.rho + start * Dp;
    double* G = a.g + start;
    double* em = a.em + start * S;
    double* fw = a.fw + start * S;
    double* cs = a.c + start;
    double* mx = a.mx + start;
    int* raw = a.raw + start;
    double* model = a.model + (int64_t)r * S * Dp;
    double* pi = a.pi + (int64_t)r * S;
    double* elbo = a.elbo + (int64_t)r * a.max_iter;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double lp = a.loop_prob, fafb = a.Fa / a.Fb;

    // the constants, and whether the recording's inputs are finite
    int bad = 0;
    for (int d = tid; d < D; d += kThreads) {
        const double p = a.phi[d];
        if (!(p > 0.0) || !finite(p)) bad = 1;
        sSq[d] = sqrt(p);
    }
    for (int s = tid; s < S; s += kThreads)
        if (!finite(pi[s])) bad = 1;
    for (int k = tid; k < a.max_iter; k += kThreads) elbo[k] = nan;
    __syncthreads();
    for (int t = wave; t < T; t += kWaves) {
        double sq = 0.0;
        for (int d = lane; d < D; d += 64) {
            const double x = X[(int64_t)t * a.ldx + d];
            rho[(int64_t)t * Dp + d] = x * sSq[d];
            sq += x * x;
        }
        sq = wave_sum(sq, 64);
        if (!finite(sq)) bad = 1;
        if (lane == 0) {
            rho[(int64_t)t * Dp + D] = 1.0;
            G[t] = -0.5 * (sq + (double)D * kLog2Pi);
        }
        for (int s = lane; s < S; s += 64)
            if (!finite(gam[(int64_t)t * ldg + s])) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        for (int t = wave; t < T; t += kWaves)
            for (int s = lane; s < S; s += 64) gam[(int64_t)t * ldg + s] = nan;
        for (int s = tid; s < S; s += kThreads) pi[s] = nan;
        for (int t = tid; t < T; t += kThreads)
            if (a.labels) a.labels[start + t] = -1;
        if (tid == 0) {
            a.iters[r] = 0;
            if (a.n_speakers) a.n_speakers[r] = 0;
        }
        return;
    }

    int it = 0;
    double prev = 0.0;
    for (; it < a.max_iter; ++it) {
        if (tid < kMaxSpk) sPi[tid] = tid < S ? pi[tid] : 0.0;

        // 1. gamma^T rho: A[s][t] = gamma (lane: row l15, k = l4), B[t][d] = rho (lane: k = l4, column l15)
        for (int dt = wave; dt < DT; dt += kWaves) {
            const int d = dt * 16 + l15;
            const bool dv = d < Dp;
            f64x4 acc[kSpkTiles];
#pragma unroll
            for (int st = 0; st < kSpkTiles; ++st) acc[st] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
            for (int t0 = 0; t0 < T; t0 += 4) {
                const int t = t0 + l4;
                const bool tv = t < T;
                const double b = tv && dv ? rho[(int64_t)t * Dp + d] : 0.0;
#pragma unroll
                for (int st = 0; st < kSpkTiles; ++st)
                    if (st < ST) {
                        const int s = st * 16 + l15;
                        const double av = tv && s < S ? gam[(int64_t)t * ldg + s] : 0.0;
                        acc[st] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b, acc[st], 0, 0, 0);
                    }
            }
            // C/D of the f64 MFMA: column lane & 15, row (lane >> 4) + 4 reg
#pragma unroll
            for (int st = 0; st < kSpkTiles; ++st)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int s = st * 16 + l4 + 4 * q;
                    if (st < ST && s < S && dv) model[(int64_t)s * Dp + d] = acc[st][q];
                }
        }
        __syncthreads();

        // 2. the speaker models
        for (int s = wave; s < S; s += kWaves) {
            double* row = model + (int64_t)s * Dp;
            const double ns = row[D];
            double kacc = 0.0, eacc = 0.0;
            for (int d = lane; d < D; d += 64) {
                const double p = a.phi[d];
                const double invl = 1.0 / (1.0 + fafb * ns * p);
                const double al = fafb * invl * row[d];
                row[d] = al;
                kacc += (invl + al * al) * p;
                eacc += log(invl) - invl - al * al + 1.0;
            }
            kacc = wave_sum(kacc, 64);
            eacc = wave_sum(eacc, 64);
            if (lane == 0) {
                sK[s] = -0.5 * kacc;
                sE[s] = eacc;
            }
        }
        __syncthreads();

        // 3. rho alpha^T: A[t][d] = rho (lane: row l15, k = l4), B[d][s] = alpha^T (lane: k = l4, column l15)
        for (int tt = wave; tt < TT; tt += kWaves) {
            const int t = tt * 16 + l15;
            const bool tv = t < T;
            f64x4 acc[kSpkTiles];
#pragma unroll
            for (int st = 0; st < kSpkTiles; ++st) acc[st] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
            for (int d0 = 0; d0 < D; d0 += 4) {
                const int d = d0 + l4;
                const bool dv = d < D;
                const double av = tv && dv ? rho[(int64_t)t * Dp + d] : 0.0;
#pragma unroll
                for (int st = 0; st < kSpkTiles; ++st)
                    if (st < ST) {
                        const int s = st * 16 + l15;
                        const double bv = dv && s < S ? model[(int64_t)s * Dp + d] : 0.0;
                        acc[st] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[st], 0, 0, 0);
                    }
            }
#pragma unroll
            for (int st = 0; st < kSpkTiles; ++st)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int tr = tt * 16 + l4 + 4 * q, s = st * 16 + l15;
                    if (st < ST && tr < T && s < S) em[(int64_t)tr * S + s] = a.Fa * ((acc[st][q] + sK[s]) + G[tr]);
                }
        }
        __syncthreads();

        // 4. the scaled emissions: a dead speaker takes no part in the maximum and emits nothing
        for (int t = tid; t < T; t += kThreads) {
            double* row = em + (int64_t)t * S;
            double m = -std::numeric_limits<double>::infinity();
            for (int s = 0; s < S; ++s)
                if (sPi[s] != 0.0) m = fmax(m, row[s]);
            for (int s = 0; s < S; ++s) row[s] = sPi[s] != 0.0 ? exp(row[s] - m) : 0.0;
            mx[t] = m;
        }
        __syncthreads();

        // 5. the two recurrences: wave 0, a lane per speaker
        if (wave == 0) {
            const int s = lane;
            const bool sv = s < S;
            const double p = sPi[s], q = (1.0 - lp) * p;
            double cur[kPF], nxt[kPF];
            double an = 0.0;
#pragma unroll
            for (int u = 0; u < kPF; ++u) cur[u] = sv && u < T ? em[(int64_t)u * S + s] : 0.0;
            for (int t0 = 0; t0 < T; t0 += kPF) {
#pragma unroll
                for (int u = 0; u < kPF; ++u) {
                    const int t = t0 + kPF + u;
                    nxt[u] = sv && t < T ? em[(int64_t)t * S + s] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < kPF; ++u) {
                    const int t = t0 + u;
                    if (t < T) {
                        const double v = (t == 0 ? p : lp * an + q) * cur[u];
                        const double cc = wave_sum(v, span);
                        an = v / cc;
                        if (sv) fw[(int64_t)t * S + s] = an;
                        if (lane == 0) cs[t] = cc;
                    }
                }
#pragma unroll
                for (int u = 0; u < kPF; ++u) cur[u] = nxt[u];
            }
            __threadfence_block();      // c_t is written by lane 0 and read back by every lane

            double beta = 1.0, pacc = 0.0, g0 = 0.0;
            double cb[kPF], ca[kPF], cc[kPF], nb[kPF], na[kPF], nc[kPF];
#pragma unroll
            for (int u = 0; u < kPF; ++u) {
                const int t = T - 1 - u;
                const bool tv = t >= 0;
                cb[u] = sv && tv ? em[(int64_t)t * S + s] : 0.0;
                ca[u] = sv && tv ? fw[(int64_t)t * S + s] : 0.0;
                cc[u] = tv ? cs[t] : 1.0;
            }
            for (int i0 = 0; i0 < T; i0 += kPF) {
#pragma unroll
                for (int u = 0; u < kPF; ++u) {
                    const int t = T - 1 - (i0 + kPF + u);
                    const bool tv = t >= 0;
                    nb[u] = sv && tv ? em[(int64_t)t * S + s] : 0.0;
                    na[u] = sv && tv ? fw[(int64_t)t * S + s] : 0.0;
                    nc[u] = tv ? cs[t] : 1.0;
                }
#pragma unroll
                for (int u = 0; u < kPF; ++u) {
                    const int t = T - 1 - (i0 + u);
                    if (t >= 0) {
                        const double gm = ca[u] * beta;
                        if (sv) gam[(int64_t)t * ldg + s] = gm;
                        if (t > 0) {
                            const double w = cb[u] * beta, term = q * w;
                            const double rs = wave_sum(term, span);
                            const double ic = 1.0 / cc[u];
                            pacc += term * ic;
                            beta = (lp * w + rs) * ic;
                        } else {
                            g0 = gm;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < kPF; ++u) {
                    cb[u] = nb[u];
                    ca[u] = na[u];
                    cc[u] = nc[u];
                }
            }
            const double pn = sv ? g0 + pacc : 0.0;
            const double tot = wave_sum(pn, span);
            if (sv) pi[s] = pn / tot;
        }
        __syncthreads();

        // 6. the total log-likelihood and the ELBO
        double part = 0.0;
        for (int t = tid; t < T; t += kThreads) part += log(cs[t]) + mx[t];
        sRed[tid] = part;
        __syncthreads();
        for (int off = kThreads / 2; off >= 1; off >>= 1) {
            if (tid < off) sRed[tid] += sRed[tid + off];
            __syncthreads();
        }
        double e = 0.0;
        for (int s = 0; s < S; ++s) e += sE[s];
        const double now = sRed[0] + a.Fb * 0.5 * e;
        if (tid == 0) elbo[it] = now;
        const bool stop = it >= 1 && now - prev < a.epsilon;
        prev = now;
        __syncthreads();
        if (stop) {
            ++it;
            break;
        }
    }
    if (tid == 0) a.iters[r] = it;
    if (!a.labels && !a.n_speakers) return;

    // the labels: argmax over the speakers (ties to the lowest), renumbered in the order of first appearance
    if (tid < kMaxSpk) sFirst[tid] = INT_MAX;
    __syncthreads();
    for (int t = tid; t < T; t += kThreads) {
        const double* row = gam + (int64_t)t * ldg;
        int best = 0;
        double bv = row[0];
        for (int s = 1; s < S; ++s) {
            const double v = row[s];
            if (v > bv) {
                bv = v;
                best = s;
            }
        }
        raw[t] = best;
        atomicMin(&sFirst[best], t);
    }
    __syncthreads();
    if (tid < kMaxSpk) {
        const int mine = sFirst[tid];
        int rank = 0;
        for (int u = 0; u < S; ++u) rank += sFirst[u] < mine ? 1 : 0;
        sNew[tid] = rank;
        const unsigned long long used = __ballot(tid < S && mine != INT_MAX);
        if (tid == 0 && a.n_speakers) a.n_speakers[r] = __popcll(used);
    }
    __syncthreads();
    if (a.labels)
        for (int t = tid; t < T; t += kThreads) a.labels[start + t] = sNew[raw[t]];
}

// ---------------------------------------------------------------- host side

thread_local ErrorChannel g_verr;

}  // namespace
}  // namespace xvec

using namespace xvec;

extern "C" {

const char* xvec_vbx_last_error(void) { return g_verr.c_str(); }

size_t xvec_vbx_workspace_bytes(const int64_t* rec_start_host, int32_t n_rec, int32_t dim, int32_t n_spk) {
    Refusal why;
    if (vbx_plan::check_rec_start(rec_start_host, n_rec, why) || vbx_plan::check_shape(dim, n_spk, why)) return 0;
    return vbx_plan::make_layout(rec_start_host, n_rec, dim, n_spk).total;
}

int xvec_vbx_init(const int32_t* labels, const int64_t* rec_start_host, int32_t n_rec, int32_t n_spk, double smoothing,
                  double* gamma, int64_t ldg, double* pi, xvec_stream stream) {
    Refusal why;
    if (vbx_plan::check_rec_start(rec_start_host, n_rec, why) || vbx_plan::check_shape(1, n_spk, why))
        return g_verr.refused(XVEC_ERR_ARG, why);
    if (!(smoothing * 0.0 == 0.0)) return g_verr.fail(XVEC_ERR_ARG, "smoothing = %g must be finite", smoothing);
    if (ldg < n_spk) return g_verr.fail(XVEC_ERR_ARG, "ldg = %lld is smaller than the %d speakers", (long long)ldg, n_spk);
    if (!labels || !gamma || !pi) return g_verr.fail(XVEC_ERR_ARG, "null pointer: labels / gamma / pi");
    const int64_t N = rec_start_host[n_rec];
    const double e = std::exp(smoothing), rest = e + (double)(n_spk - 1);
    const vbx_plan::Launch l = vbx_plan::init_launch(N, n_rec);
    vbx_init_kernel<<<(unsigned)l.blocks, l.threads, 0, static_cast<hipStream_t>(stream)>>>(labels, N, n_rec, n_spk, e / rest, 1.0 / rest,
                                                                                          1.0 / (double)n_spk, gamma, ldg, pi);
    return g_verr.launch_ok("vbx_init_kernel");
}

int xvec_vbx_run(const double* X, int64_t ldx, int32_t dim, const double* phi, const int64_t* rec_start_host, int32_t n_rec,
                 int32_t n_spk, const xvec_vbx_options* options, double* gamma, int64_t ldg, double* pi, double* elbo,
                 int32_t* iters, int32_t* labels, int32_t* n_speakers, void* workspace, size_t workspace_bytes,
                 xvec_stream stream) {
    Refusal why;
    if (vbx_plan::check_rec_start(rec_start_host, n_rec, why) || vbx_plan::check_shape(dim, n_spk, why) ||
        vbx_plan::check_options(options, why))
        return g_verr.refused(XVEC_ERR_ARG, why);
    if (ldx < dim) return g_verr.fail(XVEC_ERR_ARG, "ldx = %lld is smaller than dim = %d", (long long)ldx, dim);
    if (ldg < n_spk) return g_verr.fail(XVEC_ERR_ARG, "ldg = %lld is smaller than the %d speakers", (long long)ldg, n_spk);
    if (!X || !phi || !gamma || !pi || !elbo || !iters) return g_verr.fail(XVEC_ERR_ARG, "null pointer: X / phi / gamma / pi / elbo / iters");
    const vbx_plan::Layout l = vbx_plan::make_layout(rec_start_host, n_rec, dim, n_spk);
    int rc;
    if ((rc = workspace_arg_ok(workspace, workspace_bytes, l.total, g_verr))) return rc;

    VbxArgs g{};
    g.X = X;
    g.ldx = ldx;
    g.dim = dim;
    g.phi = phi;
    g.rec_start = part<const int64_t>(workspace, l.rec_start);
    g.n_spk = n_spk;
    g.loop_prob = options->loop_prob;
    g.Fa = options->Fa;
    g.Fb = options->Fb;
    g.epsilon = options->epsilon;
    g.max_iter = options->max_iter;
    g.gamma = gamma;
    g.ldg = ldg;
    g.pi = pi;
    g.elbo = elbo;
    g.iters = iters;
    g.labels = labels;
    g.n_speakers = n_speakers;
    g.rho = part<double>(workspace, l.rho);
    g.g = part<double>(workspace, l.g);
    g.em = part<double>(workspace, l.em);
    g.fw = part<double>(workspace, l.fw);
    g.c = part<double>(workspace, l.c);
    g.mx = part<double>(workspace, l.mx);
    g.raw = part<int>(workspace, l.raw);
    g.model = part<double>(workspace, l.model);

    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((rc = upload(part<int64_t>(workspace, l.rec_start), rec_start_host, (size_t)n_rec + 1, "rec_start", s, g_verr)))
        return rc;
    const vbx_plan::Launch run = vbx_plan::run_launch(n_rec);
    vbx_run_kernel<<<(unsigned)run.blocks, run.threads, 0, s>>>(g);
    return g_verr.launch_ok("vbx_run_kernel");
}

}  // extern "C"
