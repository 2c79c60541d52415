"""Timing of score normalisation (xvector_amd.snorm) at the reference's test-set size: cohort statistics of 4874 rows against
cohorts of 2000 and 10 000 (top_k 0 and 300), apply on the 4874 x 4874 score matrix, and the whole chain
score -> stats -> apply -> evaluate_trials against the raw score -> evaluate_trials.  Device time from hipEvents around 5 calls,
7 rounds with the library and the torch baseline interleaved (the baseline: torch.topk(S, k, dim=1, sorted=False) followed by
torch.std_mean, torch.std_mean alone for top_k = 0, broadcasting ops for apply), medians over the rounds, one box.  Writes
profiles-style text to the path given as the first argument (default: standard output only)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from xvector_amd import evaluate as ev, hip, scoring, snorm

dev = "cuda:0"
n, dim, n_trials, ROUNDS, CALLS, HBM = 4874, 512, 37720, 7, 5, 8.0e12
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS


def interleaved(fns):
    """Median, min and max over ROUNDS of the per-call device time (ms) of every function, one after the other in each round."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(ROUNDS):
        for t, fn in zip(ts, fns):
            t.append(once(fn))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


fmt = lambda t: f"{t[0]:8.3f} ms ({t[1]:.3f}, {t[2]:.3f})"
say(f"Score normalisation timing: one MI355X, build {hip.version().split()[-1]} (xvec_version()), `python profiles/diag/snorm_timing.py`.")
say(f"{n} rows (the reference's test set), fp64 N(0, 1) cohort scores; device time per call from hipEvents around {CALLS} calls,")
say(f"{ROUNDS} rounds with the library and the torch baseline interleaved, medians (min, max).  Rates: one read of S over the time,")
say("against the 8.0 TB/s HBM figure.")
say()
say("cohort statistics (xvec_snorm_row_stats through snorm.cohort_stats; torch: topk(sorted=False) + std_mean, std_mean for top_k = 0)")
gen = torch.Generator(device=dev).manual_seed(0)
for C in (2000, 10000):
    S = torch.randn((n, C), dtype=torch.float64, device=dev, generator=gen)
    ws = torch.empty(int(hip.lib.xvec_snorm_workspace_bytes(n, C)), dtype=torch.uint8, device=dev)
    for top_k in (0, 300):
        ours = lambda: snorm.cohort_stats(S, top_k, workspace=ws)
        base = (lambda: torch.std_mean(S, dim=1)) if top_k == 0 else (lambda: torch.std_mean(torch.topk(S, top_k, dim=1, sorted=False).values, dim=1))
        t_o, t_b = interleaved([ours, base])
        st, (bs, bm) = ours(), base()
        err = max(float(((st.mean - bm).abs() / bm.abs().clamp_min(1e-3)).max()), float(((st.std - bs).abs() / bs).max()))
        rate = n * C * 8 / (t_o[0] * 1e-3)
        say(f"  C = {C:5d}, top_k = {top_k:3d}: library {fmt(t_o)}   torch {fmt(t_b)}   torch / library {t_b[0] / t_o[0]:6.2f} x   "
            f"{rate / 1e12:.2f} TB/s = {100 * rate / HBM:.0f} % of HBM   (largest relative difference to torch {err:.1e})")
    del S
say()
say(f"apply on {n} x {n} (xvec_snorm_apply, S-norm, out of place; torch: 0.5 (S - m[:, None]) / s[:, None] + 0.5 (S - m[None, :]) / s[None, :])")
S = torch.randn((n, n), dtype=torch.float64, device=dev, generator=gen)
m, s = torch.randn(n, dtype=torch.float64, device=dev, generator=gen), torch.rand(n, dtype=torch.float64, device=dev, generator=gen) + 0.5
out = torch.empty_like(S)
ours = lambda: snorm.apply_norm(S, (m, s), (m, s), out=out)
base = lambda: 0.5 * (S - m[:, None]) / s[:, None] + 0.5 * (S - m[None, :]) / s[None, :]
t_o, t_b = interleaved([ours, base])
rate = 2 * n * n * 8 / (t_o[0] * 1e-3)
say(f"  library {fmt(t_o)}   torch {fmt(t_b)}   torch / library {t_b[0] / t_o[0]:6.2f} x   read + write {rate / 1e12:.2f} TB/s = {100 * rate / HBM:.0f} % of HBM")
del S, out
say()
say(f"the chain at {n} x-vectors of {dim} dimensions, rank-200 PLDA model, {n_trials} trials, cohort of 2000 x-vectors, top_k = 300")
rng = np.random.default_rng(0)
mean = rng.normal(0, 1, dim)
F = rng.normal(0, 1 / np.sqrt(dim), (dim, 200))
A = rng.normal(0, 1 / np.sqrt(dim), (dim, dim))
Sigma = A @ A.T + 0.5 * np.eye(dim)
labels = np.arange(n) % 40
chol = np.linalg.cholesky(Sigma).T
x = mean + rng.normal(0, 1, (40, 200))[labels] @ F.T + rng.normal(0, 1, (n, dim)) @ chol
cohort = mean + rng.normal(0, 1, (2000, 200)) @ F.T + rng.normal(0, 1, (2000, dim)) @ chol
scorer = scoring.PldaScorer(mean, F, Sigma)
xd = torch.from_numpy(x).to(dev)
rows, cols = rng.integers(0, n, n_trials), rng.integers(0, n, n_trials)
trials = ev.TrialList(rows, cols, labels[rows] == labels[cols])
norm = snorm.ScoreNormalizer(scorer, cohort, top_k=300)
row_d, col_d, tgt_d = trials.on(dev)
res = torch.empty(10, dtype=torch.float64, device=dev)
ws_e = torch.empty(int(hip.lib.xvec_eval_workspace_bytes(n_trials)), dtype=torch.uint8, device=dev)
stream = lambda: torch.cuda.current_stream(dev).cuda_stream


def evaluate(S):        # the library call alone: evaluate_trials' 80-byte read-back would end the timed region in a synchronise
    hip.lib.xvec_eval_trials(S.data_ptr(), n, n, n, row_d.data_ptr(), col_d.data_ptr(), tgt_d.data_ptr(), n_trials, 1.0, 1.0, 0.5,
                             res.data_ptr(), ws_e.data_ptr(), ws_e.numel(), stream())


def raw_chain():
    evaluate(scorer.score(xd))


def norm_chain():
    S = scorer.score(xd)
    evaluate(norm.normalize(S, xd, mode="s", out=S))


t_raw, t_norm, t_stats = interleaved([raw_chain, norm_chain, lambda: norm.stats(xd)])
say(f"  score -> evaluate_trials                        {fmt(t_raw)}")
say(f"  score -> stats -> apply -> evaluate_trials      {fmt(t_norm)}   {t_norm[0] / t_raw[0]:.2f} x the raw chain")
say(f"  of it ScoreNormalizer.stats (score against the cohort + row stats)  {fmt(t_stats)}")
r_raw = ev.evaluate_trials(scorer.score(xd), trials)
S = scorer.score(xd)
r_norm = ev.evaluate_trials(norm.normalize(S, xd, out=S), trials)
say(f"  EER raw {r_raw.eer:.4f}, S-normalised {r_norm.eer:.4f}; minDCF raw {r_raw.min_dcf:.4f}, S-normalised {r_norm.min_dcf:.4f} (synthetic speakers)")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
