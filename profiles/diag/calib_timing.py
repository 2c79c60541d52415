"""Timing of score calibration (xvector_amd.calibrate) at the reference's test-set size: the 37 720-trial list over the
4874 x 4874 score matrix and all 4874^2 cells as trials.  The fit per Newton iteration and in total, apply, Cllr, and minCllr split
into the sort (xvec_eval_sorted_keys) and the hull reduction.  Device time from hipEvents around 3 calls, 7 rounds with the
library and the torch baseline (the same arithmetic in torch ops on the same device) interleaved, medians over the rounds, one
box; the host path (copy, then scipy / scikit-learn) in wall-clock time, once at the large size.  Writes profiles-style text to
the path given as the first argument (default: standard output only)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from xvector_amd import calibrate as cal, evaluate as ev, hip

dev = "cuda:0"
n, n_trials, ROUNDS, CALLS, HBM, FP64 = 4874, 37720, 7, 3, 8.0e12, 78.6e12
FLOPS_PER_TRIAL = 30          # the pass kernel's explicit fp64 operations per trial, exp / log1p / the reciprocal counted as one each
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
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(ROUNDS):
        for t, fn in zip(ts, fns):
            t.append(once(fn))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


fmt = lambda t: f"{t[0]:9.3f} ms ({t[1]:.3f}, {t[2]:.3f})"
stream = lambda: torch.cuda.current_stream(dev).cuda_stream
say(f"Score calibration timing: one MI355X, build {hip.version().split()[-1]} (xvec_version()), `python profiles/diag/calib_timing.py`.")
say(f"{n} x {n} fp64 score matrix (the reference's test set), target scores N(-22, 24), non-target scores N(-50, 27), 40 speakers;")
say(f"device time per call from hipEvents around {CALLS} calls, {ROUNDS} rounds with the library and the torch baseline interleaved, medians")
say("(min, max).  Host path: wall-clock time of the copy to the host and of scipy.optimize.minimize (BFGS with the gradient, on")
say("standardised scores) / sklearn.isotonic.IsotonicRegression there.  Rates against the 8.0 TB/s HBM and 78.6 TF fp64 vector figures.")
say()
rng = np.random.default_rng(0)
labels = np.arange(n) % 40
same = labels[:, None] == labels[None, :]
host = np.where(same, rng.normal(-22.0, 24.0, (n, n)), rng.normal(-50.0, 27.0, (n, n)))
host = np.triu(host) + np.triu(host, 1).T
S = torch.from_numpy(host).to(dev)
lab_d = torch.from_numpy(labels.astype(np.int32)).to(dev)
rows, cols = rng.integers(0, n, n_trials), rng.integers(0, n, n_trials)
small = ev.TrialList(rows, cols, labels[rows] == labels[cols])
ii, jj = np.nonzero(~np.eye(n, dtype=bool))
large = ev.TrialList(ii, jj, labels[ii] == labels[jj])
del ii, jj


def torch_newton_pass(s, t, w, a, b):
    """The pass kernel's arithmetic in torch ops: J, the gradient and the Hessian at (a, b) over standardised scores."""
    x = a * s + b
    u = torch.where(t, -x, x)
    sig = torch.sigmoid(u)
    dj = torch.where(t, -w * sig, w * sig)
    h = w * sig * (1 - sig)
    return ((w * torch.nn.functional.softplus(u)).sum(), (dj * s).sum(), dj.sum(), (h * s * s).sum(), (h * s).sum(), h.sum())


def torch_cllr(l, t):
    sp = torch.nn.functional.softplus
    return (sp(-l[t]).mean() + sp(l[~t]).mean()) / (2 * np.log(2))


def host_fit(s, t):
    from scipy.optimize import minimize
    from scipy.special import expit
    z = (s - s.mean()) / s.std()
    w = np.where(t, 0.5 / t.sum(), 0.5 / (~t).sum())

    def f(ab):
        x = ab[0] * z + ab[1]
        u = np.where(t, -x, x)
        dj = np.where(t, -1.0, 1.0) * w * expit(u)
        return (w * np.logaddexp(0.0, u)).sum(), np.array([(dj * z).sum(), dj.sum()])
    return minimize(f, np.zeros(2), jac=True, method="BFGS")


for name, trials, pairs in ((f"the {n_trials}-trial list", small, False), (f"all {n}^2 cells ({n * n - n} trials off the diagonal)", large, True)):
    say(name)
    row_d, col_d, tgt_d = trials.on(dev)
    m = n * n if pairs else len(trials)
    ws = torch.empty(int(hip.lib.xvec_calib_workspace_bytes(m)), dtype=torch.uint8, device=dev)
    frec = torch.empty(8, dtype=torch.float64, device=dev)
    if pairs:           # the library calls themselves: no label look-up, no read-back inside the timed region
        fit = lambda it: hip.lib.xvec_calib_fit_all_pairs(S.data_ptr(), n, n, n, lab_d.data_ptr(), lab_d.data_ptr(), 1, 0.5, it, frec.data_ptr(),
                                                          ws.data_ptr(), ws.numel(), stream())
    else:
        fit = lambda it: hip.lib.xvec_calib_fit(S.data_ptr(), n, n, n, row_d.data_ptr(), col_d.data_ptr(), tgt_d.data_ptr(), len(trials), 0.5, it,
                                                frec.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    assert fit(50) == 0
    r = cal.Calibration(frec).result()
    k = r.n_iter
    # torch: the gather once, then k passes
    gathered = lambda: (S[row_d.long(), col_d.long()], tgt_d.bool())

    def torch_fit():
        s, t = gathered()
        s = (s - s.mean()) / s.std()
        w = torch.where(t, 0.5 / t.sum(), 0.5 / (~t).sum())
        for _ in range(k):
            torch_newton_pass(s, t, w, 1.0, 0.0)
    t_1, t_k, t_50, t_torch = interleaved([lambda: fit(1), lambda: fit(k), lambda: fit(50), torch_fit])
    per = (t_k[0] - t_1[0]) / max(1, k - 1)
    kept = r.n_target + r.n_nontarget
    say(f"  fit ({k} passes to converge, status {r.status}, a = {r.a:.6f}, b = {r.b:.6f}, {r.objective_bits:.4f} bits)")
    say(f"    max_iter = 1 (gather, mean, variance, one pass)   {fmt(t_1)}")
    say(f"    max_iter = {k:2d}                                     {fmt(t_k)}   {per * 1e3:8.1f} us per Newton iteration (pass + solve)")
    say(f"    max_iter = 50 (the default: {50 - k} passes return at once) {fmt(t_50)}")
    say(f"    torch, gather + standardise + {k} passes              {fmt(t_torch)}   torch / library(max_iter = {k}) {t_torch[0] / t_k[0]:6.2f} x")
    say(f"    a pass reads 9 bytes per trial: {kept * 9 / (per * 1e-3) / 1e12:.3f} TB/s = {100 * kept * 9 / (per * 1e-3) / HBM:.1f} % of HBM; "
        f"{FLOPS_PER_TRIAL} explicit fp64 operations per trial: {100 * kept * FLOPS_PER_TRIAL / (per * 1e-3) / FP64:.1f} % of the fp64 vector figure")
    # Cllr
    ours = (lambda: cal.cllr_all_pairs(S, labels, workspace=ws)) if pairs else (lambda: cal.cllr(S, trials, workspace=ws))
    rec = torch.empty(9, dtype=torch.float64, device=dev)
    if pairs:
        rc_d = lab_d
        raw = lambda: hip.lib.xvec_calib_cllr_all_pairs(S.data_ptr(), n, n, n, rc_d.data_ptr(), rc_d.data_ptr(), 1, 1.0, 1.0, 0.5, rec.data_ptr(),
                                                        ws.data_ptr(), ws.numel(), stream())
    else:
        raw = lambda: hip.lib.xvec_calib_cllr(S.data_ptr(), n, n, n, row_d.data_ptr(), col_d.data_ptr(), tgt_d.data_ptr(), len(trials), 1.0, 1.0,
                                              0.5, rec.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    t_c, t_ct = interleaved([raw, lambda: torch_cllr(*gathered())])
    say(f"  cllr (one fused pass; the library call without the 72-byte read-back)   {fmt(t_c)}   torch (gather + softplus means) {fmt(t_ct)}   "
        f"torch / library {t_ct[0] / t_c[0]:6.2f} x")
    # minCllr: the sort alone, the whole call
    keys = torch.empty(len(trials), dtype=torch.int32, device=dev)
    bits = torch.empty(len(trials), dtype=torch.uint8, device=dev)
    ws_e = torch.empty(int(hip.lib.xvec_eval_workspace_bytes(len(trials))), dtype=torch.uint8, device=dev)
    ws_t = torch.empty(int(hip.lib.xvec_calib_workspace_bytes(len(trials))), dtype=torch.uint8, device=dev)
    pav = torch.empty(5, dtype=torch.float64, device=dev)
    sort = lambda: hip.lib.xvec_eval_sorted_keys(S.data_ptr(), n, n, n, row_d.data_ptr(), col_d.data_ptr(), tgt_d.data_ptr(), len(trials),
                                                 keys.data_ptr(), bits.data_ptr(), ws_e.data_ptr(), ws_e.numel(), stream())
    whole = lambda: hip.lib.xvec_calib_min_cllr(S.data_ptr(), n, n, n, row_d.data_ptr(), col_d.data_ptr(), tgt_d.data_ptr(), len(trials),
                                                pav.data_ptr(), None, None, None, None, 0, ws_t.data_ptr(), ws_t.numel(), stream())
    t_s, t_w, t_ts = interleaved([sort, whole, lambda: torch.sort(gathered()[0].float())])
    seg = cal.pav_segments(S, trials, capacity=0, workspace=ws_t)
    say(f"  min_cllr {fmt(t_w)}: the sort {fmt(t_s)}, the hull reduction and the sum {t_w[0] - t_s[0]:8.3f} ms ({seg.n_segments} segments, "
        f"{seg.min_cllr:.4f} bits); torch has no PAV: its gather + sort of the fp32 scores alone {fmt(t_ts)}")
    # the host path
    t0 = time.perf_counter()
    s_h = S.cpu().numpy()[trials.row_idx, trials.col_idx]
    t_h = trials.is_target.astype(bool)
    t1 = time.perf_counter()
    res = host_fit(s_h, t_h)
    t2 = time.perf_counter()
    from sklearn.isotonic import IsotonicRegression
    IsotonicRegression(increasing=True).fit_transform(s_h.astype(np.float32).astype(np.float64), t_h.astype(np.float64))
    t3 = time.perf_counter()
    say(f"  host path: copy of the matrix + gather {1e3 * (t1 - t0):9.1f} ms, scipy BFGS ({res.nit} iterations, {res.nfev} evaluations) "
        f"{1e3 * (t2 - t1):9.1f} ms, sklearn isotonic {1e3 * (t3 - t2):9.1f} ms")
    say()
    del ws, ws_e, ws_t, keys, bits

say(f"apply on {n} x {n} (xvec_calib_apply, out of place; torch: a * S + b with a and b device scalars)")
c = cal.fit_calibration(S, small)
out = torch.empty_like(S)
ab = c.record[:2]
t_o, t_b = interleaved([lambda: c.apply(S, out=out), lambda: torch.add(torch.mul(S, ab[0]), ab[1], out=out)])
rate = 2 * n * n * 8 / (t_o[0] * 1e-3)
say(f"  library {fmt(t_o)}   torch {fmt(t_b)}   torch / library {t_b[0] / t_o[0]:6.2f} x   read + write {rate / 1e12:.2f} TB/s = {100 * rate / HBM:.0f} % of HBM")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
