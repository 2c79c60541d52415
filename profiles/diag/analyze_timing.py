"""Timing of score analysis (xvector_amd.analyze, include/xvec_analyze.h) at the reference's test-set size: the 37 720-trial
list over the 4874 x 4874 score matrix, and all 23.75 M cells off the diagonal.  The summary without a histogram, with 256
RINT bins of width 1 (the plan's LDS copies against one table per block), the hardest lists at k = 200 and 2048; against
(a) the same work in torch ops on the same device (masked min / max / var_mean, bincount of the rounded scores, topk),
(b) a copy to the host plus numpy, with a literal run of the reference's hardest-pair loop at k = 200, and (c) for the
hardest lists xvec_eval_sorted_order plus a gather of its ends; xvec_report_range in the same run.  A second file records the
distance of the kernel's and of numpy's moments to np.longdouble.  Device time from hipEvents around the calls, 7 rounds with
the candidates interleaved, medians, one box.
    python profiles/diag/analyze_timing.py [timing.txt [errors.txt]]"""
import ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch

import analyze_ref as ar
from xvector_amd import analyze, hip

dev = "cuda:0"
n, n_trials, ROUNDS, HBM = 4874, 37720, 7, 8.0e12
stream = lambda: torch.cuda.current_stream(dev).cuda_stream
lines, err_lines = [], []


def say(s="", to=lines):
    print(s, flush=True)
    to.append(s)


def once(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def interleaved(fns, calls=1):
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(ROUNDS):
        for t, fn in zip(ts, fns):
            t.append(once(fn, calls))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


fmt = lambda t: f"{t[0]:10.4f} ms ({t[1]:.4f}, {t[2]:.4f})"
say(f"Score analysis timing: one MI355X, build {hip.version().split()[-1]} (xvec_version()), `python profiles/diag/analyze_timing.py`.")
say(f"{n} x {n} fp64 score matrix (target scores N(-22, 24), non-target scores N(-50, 27), 1251 speakers); device time per call from")
say(f"hipEvents, {ROUNDS} rounds with the candidates interleaved, medians (min, max).  The library calls themselves: no label look-up, no")
say("read-back inside the timed region.  HBM figure: 8.0 TB/s.")
say()
rng = np.random.default_rng(0)
speakers = 1251
labels = np.arange(n) % speakers
same = labels[:, None] == labels[None, :]
host = np.where(same, rng.normal(-22.0, 24.0, (n, n)), rng.normal(-50.0, 27.0, (n, n)))
S = torch.from_numpy(host).to(dev)
lab_d = torch.from_numpy(labels.astype(np.int32)).to(dev)
rows, cols = rng.integers(0, n, n_trials), rng.integers(0, n, n_trials)
tgt = (labels[rows] == labels[cols]).astype(np.uint8)
rows[: n_trials // 2] = (cols[: n_trials // 2] + speakers) % n                # about half the list are targets, as in the reference's file
tgt = (labels[rows] == labels[cols]).astype(np.uint8)
row_d, col_d, tgt_d = (torch.from_numpy(a).to(dev) for a in (rows.astype(np.int32), cols.astype(np.int32), tgt))
BINS = dict(first=-200, n_bins=256)

# xvec_report_range: the one-pass reader the README has at 3.3 TB/s
rng_ws = torch.empty(int(hip.lib.xvec_report_range_workspace_bytes()), dtype=torch.uint8, device=dev)
rng_out = torch.empty(3, dtype=torch.float64, device=dev)
report_range = lambda: hip.lib.xvec_report_range(S.data_ptr(), n, n, n, rng_out.data_ptr(), rng_ws.data_ptr(), rng_ws.numel(), stream())
assert report_range() == 0

for pairs in (False, True):
    m = n * n if pairs else n_trials
    read = (m - n if pairs else m) * 8
    stats = torch.empty(26, dtype=torch.float64, device=dev)
    counts = torch.empty((2, 258), dtype=torch.int64, device=dev)
    ws_s = torch.empty(int(hip.lib.xvec_analyze_summary_workspace_bytes(m, 256)), dtype=torch.uint8, device=dev)

    def summary(bins=None):
        b = None if bins is None else C.byref(bins)
        if pairs:
            return hip.lib.xvec_analyze_summary_all_pairs(S.data_ptr(), n, n, n, lab_d.data_ptr(), lab_d.data_ptr(), 1, 0, b, stats.data_ptr(),
                                                          counts.data_ptr(), ws_s.data_ptr(), ws_s.numel(), stream())
        return hip.lib.xvec_analyze_summary(S.data_ptr(), n, n, n, row_d.data_ptr(), col_d.data_ptr(), tgt_d.data_ptr(), n_trials, b,
                                            stats.data_ptr(), counts.data_ptr(), ws_s.data_ptr(), ws_s.numel(), stream())
    plan_copies = analyze.plan(m, 256)["hist_copies"]
    b_plan = hip.AnalyzeBins(1.0, BINS["first"], 256, 1, 0, 0)
    b_one = hip.AnalyzeBins(1.0, BINS["first"], 256, 1, 1, 0)
    assert summary() == 0 and summary(b_plan) == 0 and summary(b_one) == 0, hip.lib.xvec_analyze_last_error().decode()

    lists = torch.zeros((2, 2048, 24), dtype=torch.uint8, device=dev)
    found = torch.empty(4, dtype=torch.int64, device=dev)
    ws_h = {(k, cap): torch.empty(int(hip.lib.xvec_analyze_hardest_workspace_bytes(m, k, cap)), dtype=torch.uint8, device=dev)
            for k, cap in ((200, 0), (2048, 0), (200, 65536))}

    def hardest(k, cap=0):
        sel, w = hip.AnalyzeSelect(k, cap), ws_h[(k, cap)]
        if pairs:
            return hip.lib.xvec_analyze_hardest_all_pairs(S.data_ptr(), n, n, n, lab_d.data_ptr(), lab_d.data_ptr(), 1, 0, C.byref(sel),
                                                          lists[0].data_ptr(), lists[1].data_ptr(), found.data_ptr(), w.data_ptr(), w.numel(), stream())
        return hip.lib.xvec_analyze_hardest(S.data_ptr(), n, n, n, row_d.data_ptr(), col_d.data_ptr(), tgt_d.data_ptr(), n_trials, C.byref(sel),
                                            lists[0].data_ptr(), lists[1].data_ptr(), found.data_ptr(), w.data_ptr(), w.numel(), stream())
    assert hardest(200) == 0 and hardest(2048) == 0 and hardest(200, 65536) == 0, hip.lib.xvec_analyze_last_error().decode()

    # baseline (a): torch ops on the same device
    if pairs:
        off = ~torch.eye(n, dtype=torch.bool, device=dev)
        tmask = (lab_d[:, None] == lab_d[None, :]) & off
        nmask = ~(lab_d[:, None] == lab_d[None, :])
        pick = lambda: S
    else:
        ri, ci = row_d.long(), col_d.long()
        tmask, nmask = tgt_d.bool(), ~tgt_d.bool()
        off = None
        pick = lambda: S[ri, ci]

    def torch_summary():
        x = pick()
        out = []
        for mask in (nmask, tmask) + ((off,) if pairs else (None,)):
            v = x[mask] if mask is not None else x
            out.append((v.min(), v.max(), torch.var_mean(v, unbiased=False)))
        return out

    def torch_hist():
        x = pick()
        out = []
        for mask in (nmask, tmask):
            r = torch.round(x[mask]).to(torch.int64) - BINS["first"]
            out.append(torch.bincount(r.clamp_(-1, 256) + 1, minlength=258))
        return out

    def torch_topk(k):
        x = pick()
        return torch.topk(x[nmask], k).values, torch.topk(x[tmask], k, largest=False).values

    # baseline (c): the evaluation's sort and a gather of its ends
    keys = torch.empty(m, dtype=torch.int32, device=dev)
    order = torch.empty(m, dtype=torch.int32, device=dev)
    ws_o = torch.empty(int(hip.lib.xvec_eval_sorted_order_workspace_bytes(m)), dtype=torch.uint8, device=dev)

    def sorted_ends(k):
        if pairs:
            rc = hip.lib.xvec_eval_sorted_order_all_pairs(S.data_ptr(), n, n, n, lab_d.data_ptr(), lab_d.data_ptr(), 1, keys.data_ptr(),
                                                          order.data_ptr(), ws_o.data_ptr(), ws_o.numel(), stream())
        else:
            rc = hip.lib.xvec_eval_sorted_order(S.data_ptr(), n, n, n, row_d.data_ptr(), col_d.data_ptr(), tgt_d.data_ptr(), n_trials,
                                                keys.data_ptr(), order.data_ptr(), ws_o.data_ptr(), ws_o.numel(), stream())
        o = order.long()
        flat_t = tmask.reshape(-1)
        # the first k targets from the low end and the first k non-targets from the high end of the sorted order (a window of
        # 64 k positions at either end holds them here)
        w = min(m, 64 * k)
        end = m - n if pairs else m                                # the skipped diagonal sorts last
        lo, hi = o[:w], o[end - w:end].flip(0)
        return rc, lo[flat_t[lo]][:k], hi[~flat_t[hi]][:k]
    assert sorted_ends(200)[0] == 0

    t = interleaved([lambda: summary(), lambda: summary(b_plan), lambda: summary(b_one), lambda: hardest(200), lambda: hardest(2048),
                     lambda: hardest(200, 65536), report_range, torch_summary, torch_hist, lambda: torch_topk(200), lambda: torch_topk(2048),
                     lambda: sorted_ends(200)], calls=3 if pairs else 10)
    t_sum, t_hist, t_hist1, t_h200, t_h2048, t_h200big, t_range, t_tsum, t_thist, t_ttop200, t_ttop2048, t_sort = t
    what = f"all {n}^2 cells ({m - n} trials off the diagonal)" if pairs else f"the {m}-trial list ({int(tgt.sum())} targets)"
    say(f"{what}: the scores of the trials are {read / 2 ** 20:.1f} MiB; workspace {ws_s.numel()} bytes (summary), "
        f"{ws_h[(200, 0)].numel() / 2 ** 10:.0f} KiB (hardest, cand_cap {analyze.plan(m)['cand_cap']}), {ws_h[(200, 65536)].numel() / 2 ** 10:.0f} KiB (cand_cap 65536)")
    tb = lambda t, passes: f"{passes} reads of the scores: {passes * read / (t[0] * 1e-3) / 1e12:6.3f} TB/s = {100 * passes * read / (t[0] * 1e-3) / HBM:5.1f} % of HBM"
    say(f"    summary, no histogram (two passes)                {fmt(t_sum)}   {tb(t_sum, 2)}")
    say(f"    summary, 256 RINT bins, {plan_copies} LDS copies (the plan)     {fmt(t_hist)}   histogram costs {t_hist[0] - t_sum[0]:8.4f} ms")
    say(f"    summary, 256 RINT bins, 1 LDS copy                {fmt(t_hist1)}   histogram costs {t_hist1[0] - t_sum[0]:8.4f} ms")
    say(f"    hardest, k =  200                                 {fmt(t_h200)}")
    say(f"    hardest, k = 2048                                 {fmt(t_h2048)}")
    say(f"    hardest, k =  200, cand_cap = 65536               {fmt(t_h200big)}")
    if pairs:
        # the contention path: every score in one bin, so all 64 lanes of every wave hit one slot
        keep = S.clone()
        S.fill_(3.25)
        t_c, t_c1, t_c0 = interleaved([lambda: summary(b_plan), lambda: summary(b_one), lambda: summary()], calls=3)
        S.copy_(keep)
        del keep
        say(f"    every score in ONE bin: {plan_copies} LDS copies / 1 copy / none   {fmt(t_c)} / {fmt(t_c1)} / {fmt(t_c0)}   histogram costs "
            f"{t_c[0] - t_c0[0]:8.4f} / {t_c1[0] - t_c0[0]:8.4f} ms")
        say(f"    xvec_report_range (one pass, no classes)          {fmt(t_range)}   {tb(t_range, 1)}; summary / range = {t_sum[0] / t_range[0]:5.2f}")
    say(f"    (a) torch: masked min / max / var_mean            {fmt(t_tsum)}   torch / library {t_tsum[0] / t_sum[0]:7.2f} x")
    share = f"{t_thist[0] / (t_hist[0] - t_sum[0]):7.2f} x" if t_hist[0] - t_sum[0] > 0.002 else "(the share is inside the spread of the rounds)"
    say(f"    (a) torch: bincount of the rounded scores         {fmt(t_thist)}   torch / (library's histogram share) {share}; "
        f"torch summary + bincount / library {(t_tsum[0] + t_thist[0]) / t_hist[0]:7.2f} x")
    say(f"    (a) torch: topk, k = 200 / 2048                   {fmt(t_ttop200)} / {fmt(t_ttop2048)}   torch / library {t_ttop200[0] / t_h200[0]:7.2f} x / {t_ttop2048[0] / t_h2048[0]:7.2f} x")
    say(f"    (c) xvec_eval_sorted_order + gather of the ends   {fmt(t_sort)}   sort / library {t_sort[0] / t_h200[0]:7.2f} x")
    # (b) the host, wall clock
    t0 = time.perf_counter()
    hs = S.cpu().numpy()
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    if pairs:
        pos = same & ~np.eye(n, dtype=bool)
        neg = ~same
        xs = (hs[neg], hs[pos], hs[~np.eye(n, dtype=bool)])
    else:
        x = hs[rows, cols]
        xs = (x[tgt == 0], x[tgt == 1], x)
    ref = [(np.max(v), np.min(v), np.mean(v), np.var(v)) for v in xs]
    t_np = time.perf_counter() - t0
    t0 = time.perf_counter()
    hh = [np.bincount((np.clip(np.rint(v) - BINS["first"], -1, 256) + 1).astype(np.int64), minlength=258) for v in xs[:2]]
    t_nph = time.perf_counter() - t0
    say(f"    (b) host: copy of the matrix {t_copy * 1e3:8.1f} ms + numpy max / min / mean / var {t_np * 1e3:8.1f} ms + rint and bincount {t_nph * 1e3:8.1f} ms "
        f"(wall clock)   host / library {(t_copy + t_np + t_nph) * 1e3 / t_hist[0]:8.1f} x")
    if pairs:
        t0 = time.perf_counter()
        hits = ar.reference_false_positives(np.where(neg, hs, 0.0), 200)
        t_loop = time.perf_counter() - t0
        say(f"    (b) host: the reference's hardest-pair loop, 200 hits (np.max + np.where over the matrix per hit) {t_loop * 1e3:9.1f} ms (wall clock)   "
            f"host / library {(t_copy + t_loop) * 1e3 / t_h200[0]:8.1f} x")
    # the library's answers against the host's
    assert summary(b_plan) == 0 and hardest(200) == 0
    torch.cuda.synchronize()
    got = analyze._read_summary(stats, counts, analyze.Bins(**BINS))
    u = ar.usable_all_pairs(hs, labels, labels, True, False) if pairs else ar.usable_trials(hs, rows, cols, tgt)
    want = ar.summary(u)
    assert np.array_equal(got.histogram.nontarget, hh[0][1:-1]) and np.array_equal(got.histogram.target, hh[1][1:-1])
    rec = lists.cpu().numpy().view(analyze.RECORD).reshape(2, 2048)[:, :200]
    oracle = ar.hardest(u, 200)
    assert rec[0].tobytes() == oracle[0].tobytes() and rec[1].tobytes() == oracle[1].tobytes()
    if pairs:
        assert [h[0] for h in hits] == rec[0]["score"].tolist()
    say("    (checked: the histogram equals numpy's, the k = 200 lists equal the oracle's record for record" + (", the loop's scores equal the list's)" if pairs else ")"))
    say()
    say(f"{what}: distance to np.longdouble, depth of the summation tree {analyze.plan(m)['sum_depth']}", err_lines)
    for name, g_, w, (mx, mn, mean, var) in zip(("non-target", "target", "all"), (got.nontarget, got.target, got.all), want, ref):
        assert g_.max == mx and g_.min == mn and g_.n == w["n"]
        say(f"    {name:10s} n {w['n']:9d}   mean {float(w['mean']):+.15e}   kernel {abs(float(np.longdouble(g_.mean) - w['mean'])):.3e}   numpy "
            f"{abs(float(np.longdouble(mean) - w['mean'])):.3e}      var {float(w['var']):.15e}   kernel {abs(float(np.longdouble(g_.var) - w['var'])):.3e}   "
            f"numpy {abs(float(np.longdouble(var) - w['var'])):.3e}", err_lines)
    say("", err_lines)
    del ws_s, ws_o, keys, order

if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
if len(sys.argv) > 2:
    head = [f"Score analysis, moments against np.longdouble: one MI355X, build {hip.version().split()[-1]}, `python profiles/diag/analyze_timing.py`.",
            "The matrix and the lists of profiles/analyze_timing.txt.  |kernel - longdouble| and |numpy - longdouble| side by side (numpy: np.mean and",
            "np.var of the host copy, pairwise sums).", ""]
    with open(sys.argv[2], "w") as f:
        f.write("\n".join(head + err_lines) + "\n")
