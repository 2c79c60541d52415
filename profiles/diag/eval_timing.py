"""Timing of the trial evaluation (xvector_amd.evaluate) at the reference's sizes: 4874 test x-vectors, the 37 720-trial list
and all 4874 x 4874 pairs.  Device time per call (median of 20, hipEvents around the library call alone), the whole Python
call including the 80-byte read-back (host clock, ends in a synchronise), the 190 MB device-to-host copy of the score matrix
the device path replaces, and the baseline the package offered before: copy the matrix, gather on the host, sort there
(tests/eer_ref.by_sort).  `--profile` runs a few calls only, as the subject of `rocprofv3 --kernel-trace --stats`."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import xvector_amd as xa
from xvector_amd import evaluate as ev, hip, scoring
import eer_ref

dev = "cuda:0"
n, dim, n_spk, n_trials = 4874, 512, 40, 37720
rng = np.random.default_rng(0)
mean = rng.normal(0, 1, dim)
F = rng.normal(0, 1 / np.sqrt(dim), (dim, 200))
A = rng.normal(0, 1 / np.sqrt(dim), (dim, dim))
Sigma = A @ A.T + 0.5 * np.eye(dim)
labels = np.arange(n) % n_spk
x = mean + rng.normal(0, 1, (n_spk, 200))[labels] @ F.T + rng.normal(0, 1, (n, dim)) @ np.linalg.cholesky(Sigma).T
scorer = scoring.PldaScorer(mean, F, Sigma)
xd = torch.from_numpy(x).to(dev)
S = scorer.score(xd)
rows, cols = rng.integers(0, n, n_trials), rng.integers(0, n, n_trials)
trials = ev.TrialList(rows, cols, labels[rows] == labels[cols])
print(f"build {hip.version()}; {n} x-vectors, {n_trials} trials ({int(trials.is_target.sum())} targets), {n_spk} speakers")

if "--profile" in sys.argv:
    for _ in range(5):
        ev.evaluate_trials(S, trials)
        ev.evaluate_all_pairs(S, labels)
    torch.cuda.synchronize()
    sys.exit(0)


def ev_time(fn, reps=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def wall(fn, reps=10):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


L = hip.lib
out = torch.empty(10, dtype=torch.float64, device=dev)
row_d, col_d, tgt_d = trials.on(dev)
ws_t = torch.empty(int(L.xvec_eval_workspace_bytes(n_trials)), dtype=torch.uint8, device=dev)
ws_a = torch.empty(int(L.xvec_eval_workspace_bytes(n * n)), dtype=torch.uint8, device=dev)
lab_d = torch.from_numpy(labels.astype(np.int32)).to(dev)
stream = lambda: torch.cuda.current_stream(dev).cuda_stream
lib_trials = lambda: L.xvec_eval_trials(S.data_ptr(), n, n, n, row_d.data_ptr(), col_d.data_ptr(), tgt_d.data_ptr(), n_trials, 1.0,
                                        1.0, 0.5, out.data_ptr(), ws_t.data_ptr(), ws_t.numel(), stream())
lib_pairs = lambda: L.xvec_eval_all_pairs(S.data_ptr(), n, n, n, lab_d.data_ptr(), lab_d.data_ptr(), 1, 1.0, 1.0, 0.5,
                                          out.data_ptr(), ws_a.data_ptr(), ws_a.numel(), stream())
fmt = lambda t: f"{t[0]:.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"
t_score = ev_time(lambda: scorer.score(xd))
t_trials = ev_time(lib_trials)
t_pairs = ev_time(lib_pairs)
print(f"score matrix {n} x {n}, device time:                         {fmt(t_score)}")
print(f"xvec_eval_trials, {n_trials} trials, device time:              {fmt(t_trials)}")
print(f"xvec_eval_all_pairs, {n * n} cells, device time:            {fmt(t_pairs)}   workspace {ws_a.numel() / 2**20:.0f} MiB")
w_trials = wall(lambda: ev.evaluate_trials(S, trials))
w_pairs = wall(lambda: ev.evaluate_all_pairs(S, labels))
print(f"evaluate_trials, whole call with read-back, host clock:        {fmt(w_trials)}")
print(f"evaluate_all_pairs, whole call with read-back, host clock:     {fmt(w_pairs)}")
pinned = torch.empty((n, n), dtype=torch.float64).pin_memory()
w_copy_pinned = wall(lambda: pinned.copy_(S, non_blocking=True))
w_copy = wall(lambda: S.cpu())
print(f"device-to-host copy of the matrix ({S.numel() * 8 / 1e6:.0f} MB), pinned target:  {fmt(w_copy_pinned)}")
print(f"device-to-host copy of the matrix, S.cpu():                    {fmt(w_copy)}")


def baseline_trials():
    host = scorer.score(xd).cpu().numpy()
    picked = host[trials.row_idx, trials.col_idx]
    m = trials.is_target.astype(bool)
    return eer_ref.by_sort(picked[m], picked[~m])


def baseline_pairs():
    host = scorer.score(xd).cpu().numpy()
    same = labels[:, None] == labels[None, :]
    off = ~np.eye(n, dtype=bool)
    return eer_ref.by_sort(host[same & off], host[~same])


def device_trials():
    return ev.evaluate_trials(scorer.score(xd), trials)


def device_pairs():
    return ev.evaluate_all_pairs(scorer.score(xd), labels)


b_trials, d_trials = wall(baseline_trials, 5), wall(device_trials, 5)
b_pairs, d_pairs = wall(baseline_pairs, 3), wall(device_pairs, 5)
print(f"baseline (score, copy, host gather, host sort), trial list:    {fmt(b_trials)}")
print(f"device path (score, evaluate_trials), trial list:              {fmt(d_trials)}   ratio {b_trials[0] / d_trials[0]:.1f}x")
print(f"baseline, all pairs:                                           {fmt(b_pairs)}")
print(f"device path, all pairs:                                        {fmt(d_pairs)}   ratio {b_pairs[0] / d_pairs[0]:.1f}x")
r, b = device_trials(), baseline_trials()
print(f"same numbers: eer {r.eer!r} / {b.eer!r}, min_dcf {r.min_dcf!r} / {b.min_dcf!r}, thresholds {r.eer_th == b.eer_th} {r.min_dcf_th == b.min_dcf_th}")
ok = t_trials[0] < w_copy_pinned[0]
print(f"sanity: evaluating the trial list on the device ({t_trials[0]:.3f} ms) takes {'less' if ok else 'MORE'} time than the copy it "
      f"replaces ({w_copy_pinned[0]:.3f} ms pinned, {w_copy[0]:.3f} ms pageable)")
