"""Timing of score fusion (xvector_amd.fuse) at the reference's test-set size: the 37 720-trial list over 4874 x 4874 score
matrices and all 4874^2 cells as trials, at K = 1, 2, 4 and 8 terms (K = 4: two matrices, a ROW and a COL term; the others
matrices only).  The fit per Newton iteration and in total against the same arithmetic in torch ops on the same device, at K = 1
also against xvec_calib_fit in the same rounds; the apply against torch's expression.  Device time from hipEvents around 3 calls,
7 rounds with the candidates interleaved, medians over the rounds, one box.  Writes profiles-style text to the path given as
the first argument (default: standard output only)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from xvector_amd import calibrate as cal, evaluate as ev, fuse, hip

dev = "cuda:0"
n, n_trials, ROUNDS, CALLS, HBM, FP64 = 4874, 37720, 7, 3, 8.0e12, 78.6e12
lines = []


def flops_per_trial(k):
    """The pass kernel's explicit fp64 operations per trial: 2 K of z, 2 K of the argument, 18 of the logistic part (exp,
    log1p and the reciprocal counted as one each), 3 K + 1 of the gradient and hz, (K + 1)(K + 2) - 1 - K of the Hessian."""
    return 7 * k + 19 + (k + 1) * (k + 2) - 1 - k


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
say(f"Score fusion timing: one MI355X, build {hip.version().split()[-1]} (xvec_version()), `python profiles/diag/fuse_timing.py`.")
say(f"{n} x {n} fp64 score matrices (the reference's test set; the first: target scores N(-22, 24), non-target scores N(-50, 27), 40")
say("speakers; the others: it, scaled, plus noise of their own), log durations of 200 .. 1000 frames as the ROW and COL terms of K = 4;")
say(f"device time per call from hipEvents around {CALLS} calls, {ROUNDS} rounds with the candidates interleaved, medians (min, max).")
say("Rates against the 8.0 TB/s HBM and 78.6 TF fp64 vector figures.")
say()
rng = np.random.default_rng(0)
labels = np.arange(n) % 40
same = labels[:, None] == labels[None, :]
host = np.where(same, rng.normal(-22.0, 24.0, (n, n)), rng.normal(-50.0, 27.0, (n, n)))
host = np.triu(host) + np.triu(host, 1).T
S = torch.from_numpy(host).to(dev)
del host
gen = torch.Generator(device=dev).manual_seed(1)
mats = [S] + [S * (0.02 * q) + torch.randn((n, n), dtype=torch.float64, device=dev, generator=gen) for q in range(1, 6)]
logdur = torch.log(torch.from_numpy(rng.integers(200, 1001, n)).to(dev).to(torch.float64))
ALL = [fuse.matrix(mats[0]), fuse.matrix(mats[1]), fuse.row_quality(logdur), fuse.col_quality(logdur)] + [fuse.matrix(m) for m in mats[2:]]
lab_d = torch.from_numpy(labels.astype(np.int32)).to(dev)
rows, cols = rng.integers(0, n, n_trials), rng.integers(0, n, n_trials)
small = ev.TrialList(rows, cols, labels[rows] == labels[cols])
off = ~torch.eye(n, dtype=torch.bool, device=dev)


def torch_pass(Z, t, w, x, b):
    """The pass kernel's arithmetic in torch ops: J, the gradient and the Hessian at (x, b) over standardised terms Z [K, m]."""
    a = x @ Z + b
    u = torch.where(t, -a, a)
    sig = torch.sigmoid(u)
    dj = torch.where(t, -w * sig, w * sig)
    h = w * sig * (1 - sig)
    Zh = Z * h
    return (w * torch.nn.functional.softplus(u)).sum(), Z @ dj, dj.sum(), Zh @ Z.T, Zh.sum(dim=1), h.sum()


def gather(terms, row_d, col_d):
    return torch.stack([t.data[row_d, col_d] if t.kind == fuse.MATRIX else t.data[row_d] if t.kind == fuse.ROW else t.data[col_d]
                        for t in terms])


for name, pairs in ((f"the {n_trials}-trial list", False), (f"all {n}^2 cells ({n * n - n} trials off the diagonal)", True)):
    say(name)
    row_d, col_d, tgt_d = small.on(dev)
    m = n * n if pairs else n_trials
    if pairs:
        ii, jj = off.nonzero(as_tuple=True)
    else:
        ii, jj = row_d.long(), col_d.long()
    for k in (1, 2, 4, 8):
        terms = ALL[:k]
        arr = fuse._term_array(terms)
        ws = torch.empty(int(hip.lib.xvec_fuse_workspace_bytes(m, k)), dtype=torch.uint8, device=dev)
        rec = torch.empty(16, dtype=torch.float64, device=dev)
        if pairs:           # the library calls themselves: no label look-up, no read-back inside the timed region
            fit = lambda it: hip.lib.xvec_fuse_fit_all_pairs(arr, k, n, n, lab_d.data_ptr(), lab_d.data_ptr(), 1, 0.5, 0.0, it, rec.data_ptr(),
                                                             ws.data_ptr(), ws.numel(), stream())
        else:
            fit = lambda it: hip.lib.xvec_fuse_fit(arr, k, n, n, row_d.data_ptr(), col_d.data_ptr(), tgt_d.data_ptr(), n_trials, 0.5, 0.0, it,
                                                   rec.data_ptr(), ws.data_ptr(), ws.numel(), stream())
        assert fit(50) == 0
        r = fuse.Fusion(rec, k).result()
        it_k = r.n_iter
        tgt_b = (lab_d[ii] == lab_d[jj]) if pairs else tgt_d.bool()

        def torch_fit():
            Z = gather(terms, ii, jj)
            Z = (Z - Z.mean(dim=1, keepdim=True)) / Z.std(dim=1, keepdim=True)
            w = torch.where(tgt_b, 0.5 / tgt_b.sum(), 0.5 / (~tgt_b).sum())
            x = torch.zeros(k, dtype=torch.float64, device=dev)
            for _ in range(it_k):
                torch_pass(Z, tgt_b, w, x, 0.0)
        cands = [lambda: fit(1), lambda: fit(it_k), lambda: fit(50), torch_fit]
        if k == 1:
            ws_c = torch.empty(int(hip.lib.xvec_calib_workspace_bytes(m)), dtype=torch.uint8, device=dev)
            crec = torch.empty(8, dtype=torch.float64, device=dev)
            if pairs:
                cfit = lambda it: hip.lib.xvec_calib_fit_all_pairs(S.data_ptr(), n, n, n, lab_d.data_ptr(), lab_d.data_ptr(), 1, 0.5, it,
                                                                   crec.data_ptr(), ws_c.data_ptr(), ws_c.numel(), stream())
            else:
                cfit = lambda it: hip.lib.xvec_calib_fit(S.data_ptr(), n, n, n, row_d.data_ptr(), col_d.data_ptr(), tgt_d.data_ptr(), n_trials, 0.5,
                                                         it, crec.data_ptr(), ws_c.data_ptr(), ws_c.numel(), stream())
            assert cfit(50) == 0 and cal.Calibration(crec).result().n_iter == it_k
            cands += [lambda: cfit(1), lambda: cfit(it_k)]
        ts = interleaved(cands)
        t_1, t_k, t_50, t_torch = ts[:4]
        per = (t_k[0] - t_1[0]) / max(1, it_k - 1)
        kept = r.n_target + r.n_nontarget
        by = 8 * k + 1
        say(f"  K = {k}: {it_k} passes to converge, status {r.status}, {r.objective_bits:.4f} bits, workspace {ws.numel() / 2 ** 20:.1f} MiB")
        say(f"    max_iter = 1 (gather, mean, variance, one pass)   {fmt(t_1)}")
        say(f"    max_iter = {it_k:2d}                                     {fmt(t_k)}   {per * 1e3:8.1f} us per Newton iteration (pass + solve)")
        say(f"    max_iter = 50 (the default)                        {fmt(t_50)}")
        say(f"    torch, gather + standardise + {it_k} passes              {fmt(t_torch)}   torch / library(max_iter = {it_k}) {t_torch[0] / t_k[0]:6.2f} x")
        say(f"    a pass reads {by} bytes per trial: {kept * by / (per * 1e-3) / 1e12:.3f} TB/s = {100 * kept * by / (per * 1e-3) / HBM:.1f} % of HBM; "
            f"{flops_per_trial(k)} explicit fp64 operations per trial: {100 * kept * flops_per_trial(k) / (per * 1e-3) / FP64:.1f} % of the fp64 vector figure")
        if k == 1:
            c_1, c_k = ts[4:]
            cper = (c_k[0] - c_1[0]) / max(1, it_k - 1)
            say(f"    xvec_calib_fit, the same rounds: max_iter = 1 {fmt(c_1)}, max_iter = {it_k} {fmt(c_k)}, {cper * 1e3:8.1f} us per Newton iteration; "
                f"fusion / calibration per iteration {per / cper:5.2f} x, whole fit {t_k[0] / c_k[0]:5.2f} x")
            del ws_c
        del ws
    say()

say(f"apply on {n} x {n} (xvec_fuse_apply, out of place; torch: w0 * S0 + w1 * S1 + ... + b with device scalars)")
out = torch.empty_like(S)
for k in (1, 2, 4, 8):
    terms = ALL[:k]
    fus = fuse.fit_fusion(terms, small)
    wb = fus.record[:9]

    def torch_apply():
        acc = None
        for q, t in enumerate(terms):
            f = t.data if t.kind == fuse.MATRIX else t.data[:, None] if t.kind == fuse.ROW else t.data[None, :]
            p = f * wb[q]
            acc = p if acc is None else acc + p
        torch.add(acc, wb[8], out=out)
    t_o, t_b = interleaved([lambda: fus.apply(terms, out=out), torch_apply])
    nm = sum(t.kind == fuse.MATRIX for t in terms)
    rate = (nm + 1) * n * n * 8 / (t_o[0] * 1e-3)
    say(f"  K = {k} ({nm} matrices)   library {fmt(t_o)}   torch {fmt(t_b)}   torch / library {t_b[0] / t_o[0]:6.2f} x   read + write "
        f"{rate / 1e12:.2f} TB/s = {100 * rate / HBM:.0f} % of HBM")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
