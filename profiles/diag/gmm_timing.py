"""Times the GMM-UBM unit (csrc/gmm.hip) on one device: python profiles/diag/gmm_timing.py profiles/gmm_timing.txt

N = 1 M frames, D = 24 and 72, C = 512 and 2048: pass 1 (xvec_gmm_loglik), one E-step (xvec_gmm_accumulate, global form; pass 2
is the difference), a full EM iteration (xvec_gmm_em, one iteration), the per-utterance statistics of 4874 utterances, MAP and
linear scoring for 1251 x 4874 -- against the same arithmetic in torch fp64 ops on the same device, chunked so that its ll
block fits.  hipEvents, 7 interleaved rounds, medians.  And scikit-learn on the host (as many threads as the process is given) at
a size it can finish: one EM iteration of GaussianMixture('diag') on N / 16 frames, wall clock, median of 3, SCALED by 16 to
N and labelled as such (an iteration is linear in N)."""
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import xvector_amd as xa
from xvector_amd import gmm, hip

DEV = torch.device("cuda:0")
ROUNDS = 7


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_estep(x, w, mu, v, chunk):
    P = torch.cat([mu / v, -0.5 / v], dim=1)
    g = torch.log(w) - 0.5 * (mu.shape[1] * np.log(2 * np.pi) + torch.log(v).sum(1) + (mu * mu / v).sum(1))
    n = torch.zeros_like(w)
    f = torch.zeros_like(mu)
    s = torch.zeros_like(mu)
    ll_sum = torch.zeros((), dtype=torch.float64, device=x.device)
    for i in range(0, x.shape[0], chunk):
        xc = x[i:i + chunk].to(torch.float64)
        x2 = xc * xc
        ll = torch.cat([xc, x2], dim=1) @ P.T + g
        lse = torch.logsumexp(ll, dim=1)
        gam = torch.exp(ll - lse[:, None])
        n += gam.sum(0)
        f += gam.T @ xc
        s += gam.T @ x2
        ll_sum += lse.sum()
    return n, f, s, ll_sum


def sklearn_iteration(x, w, mu, v, shrink=16, rounds=3):
    """(ms scaled to all of x, frames timed, threads) of one EM iteration of scikit-learn on every `shrink`-th frame; None where
    scikit-learn is not installed."""
    import os
    import time
    import warnings
    try:
        from sklearn.mixture import GaussianMixture
    except ImportError:
        return None
    xs = np.ascontiguousarray(x[::shrink].cpu().numpy().astype(np.float64))
    gm = GaussianMixture(len(w), covariance_type="diag", tol=0.0, max_iter=1, weights_init=w, means_init=mu, precisions_init=1.0 / v)
    times = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gm.fit(xs)
        times.append((time.perf_counter() - t0) * 1e3)
    threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    return statistics.median(times) * x.shape[0] / xs.shape[0], xs.shape[0], int(os.environ.get("OMP_NUM_THREADS", threads))


def main(out_path):
    lines = [f"GMM-UBM timing, build {hip.version()}, {torch.cuda.get_device_name(0)}, hipEvents, {ROUNDS} interleaved rounds, medians (ms)"]
    N, U = 1 << 20, 4874
    rng = np.random.default_rng(0)
    for D in (24, 72):
        for C_ in (512, 2048):
            centres = rng.normal(0.0, 2.0, (C_, D))
            x = torch.from_numpy((centres[rng.integers(0, C_, N)] + rng.normal(0.0, 1.0, (N, D))).astype(np.float32)).to(DEV)
            m = gmm.DiagGmm(np.full(C_, 1.0 / C_), centres + 0.3, np.ones((C_, D)), device=DEV)
            count = np.full(U, N // U, dtype=np.int64)
            first = np.arange(U, dtype=np.int64) * (N // U)
            chunk = max(4096, (1 << 27) // C_)
            w, mu, v = m.weights.clone(), m.means.clone(), m.variances.clone()
            calls = {
                "pass 1 (loglik)": lambda: m.log_likelihood(x),
                "E-step (passes 1 + 2)": lambda: m.estep(x),
                "EM iteration": lambda: gmm.DiagGmm(w, mu, v, device=DEV).em(x, n_iter=1),
                f"statistics of {U} utterances": lambda: m.stats(x, (first, count)),
                "torch fp64 E-step": lambda: torch_estep(x, w, mu, v, chunk),
            }
            for fn in calls.values():
                fn()
            t = {k: [] for k in calls}
            for _ in range(ROUNDS):
                for k, fn in calls.items():
                    t[k].append(timed(fn))
            med = {k: statistics.median(vs) for k, vs in t.items()}
            p = gmm.plan(N, C_, D)
            flop1 = 2.0 * N * C_ * 2 * D
            flop2 = flop1 * p["col_tiles"] + 2.0 * N * C_ * 64 * p["col_tiles"]
            lines.append(f"N = {N}, C = {C_}, D = {D}: slices {p['slices']}, column tiles {p['col_tiles']}")
            for k, vms in med.items():
                lines.append(f"  {k:<34} {vms:10.3f}")
            e, p1 = med["E-step (passes 1 + 2)"], med["pass 1 (loglik)"]
            lines.append(f"  pass 2 (E-step - pass 1)           {e - p1:10.3f}")
            lines.append(f"  pass 1: {flop1 / p1 / 1e9:.1f} TF of 78.6 in the product, {N * C_ / p1 / 1e6:.1f} G exp/s; "
                         f"pass 2: {flop2 / max(e - p1, 1e-9) / 1e9:.1f} TF in its two products; x read: {N * D * 4 / p1 / 1e9:.3f} TB/s of 8.0")
            lines.append(f"  E-step against torch: {med['torch fp64 E-step'] / e:.2f} x" + ("" if e <= med["torch fp64 E-step"] else "   ** LOSES TO TORCH **"))
            sk = sklearn_iteration(x, w.cpu().numpy(), mu.cpu().numpy(), v.cpu().numpy())
            if sk is None:
                lines.append("  scikit-learn is not installed: no host baseline")
            else:
                lines.append(f"  scikit-learn EM iteration, host     {sk[0]:10.1f}   (SCALED: {sk[1]} frames timed, x {N // sk[1]}; {sk[2]} threads; "
                             f"{sk[0] / med['EM iteration']:.0f} x the unit's)")
            if D == 24 and C_ == 512:
                st = m.stats(x, (first, count))
                enrol = gmm.GmmStats(st.n[:1251].contiguous(), st.f[:1251].contiguous())
                sc = {"MAP of 1251 models": lambda: gmm.map_adapt(m, enrol),
                      "linear scores 1251 x 4874": lambda: gmm.linear_scores(m, models, st)}
                models = gmm.map_adapt(m, enrol)
                def torch_scores():
                    a = ((models - m.means) / m.variances).reshape(1251, -1)
                    b = ((st.f - st.n[:, :, None] * m.means) / st.n.sum(1)[:, None, None]).reshape(U, -1)
                    return a @ b.T
                sc["torch linear scores"] = torch_scores
                for fn in sc.values():
                    fn()
                ts = {k: [] for k in sc}
                for _ in range(ROUNDS):
                    for k, fn in sc.items():
                        ts[k].append(timed(fn))
                for k, vs in ts.items():
                    lines.append(f"  {k:<34} {statistics.median(vs):10.3f}")
                ms = statistics.median(ts["linear scores 1251 x 4874"])
                lines.append(f"  linear scores: {2.0 * 1251 * U * C_ * D / ms / 1e9:.1f} TF of 78.6 in the product" +
                             ("" if ms <= statistics.median(ts["torch linear scores"]) else "   ** LOSES TO TORCH **"))
                del st, enrol, models
            del x, m
            torch.cuda.empty_cache()
            open(out_path, "w").write("\n".join(lines) + "\n")      # (kept as far as it got)
    print("\n".join(lines))


if __name__ == "__main__":
    main(sys.argv[1])
