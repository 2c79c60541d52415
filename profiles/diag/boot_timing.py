"""Timing of the bootstrap (xvector_amd.bootstrap, include/xvec_boot.h) at the reference's test-set size: the 37 720-trial list
over the 4874 x 4874 score matrix at n_boot = 1000 with 40 and with 1251 speaker groups (joint), and all 4874^2 cells as trials
at n_boot = 100; the split between the sort and the replicate passes; against (a) the same arithmetic in torch ops on the same
device -- one sort, then per batch of replicates a gather of the weights and cumsum -- and (b) a copy to the host plus the
numpy restatement (tests/boot_ref.py).  Because csrc/eval.hip moved its sort into a shared header: xvec_eval_trials and
xvec_eval_all_pairs at both sizes on this build against the parent commit's library (second argument; a fresh process per
library and round).  Device time from hipEvents around the calls, 7 rounds with the candidates interleaved, medians, one box.
    python profiles/diag/boot_timing.py [out.txt [parent_library.so]]"""
import ctypes as C, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch

dev = "cuda:0"
n, n_trials, ROUNDS, HBM = 4874, 37720, 7, 8.0e12
stream = lambda: torch.cuda.current_stream(dev).cuda_stream


def eval_child(path):
    """One process on one library (opened as it is: the parent's has none of the new exports the binding asks for): medians of
    xvec_eval_trials and xvec_eval_all_pairs at both sizes, as JSON."""
    lib = C.CDLL(path)
    vp, i64, f64 = C.c_void_p, C.c_int64, C.c_double
    lib.xvec_eval_workspace_bytes.restype, lib.xvec_eval_workspace_bytes.argtypes = C.c_size_t, [i64]
    lib.xvec_eval_trials.argtypes = [vp, i64, i64, i64, vp, vp, vp, i64, f64, f64, f64, vp, vp, C.c_size_t, vp]
    lib.xvec_eval_all_pairs.argtypes = [vp, i64, i64, i64, vp, vp, C.c_int32, f64, f64, f64, vp, vp, C.c_size_t, vp]
    lib.xvec_version.restype = C.c_char_p
    g = torch.Generator(device=dev).manual_seed(0)
    S = torch.randn((n, n), dtype=torch.float64, device=dev, generator=g)
    lab = (torch.arange(n, device=dev) % 40).to(torch.int32)
    rows = torch.randint(0, n, (n_trials,), device=dev, generator=g).to(torch.int32)
    cols = torch.randint(0, n, (n_trials,), device=dev, generator=g).to(torch.int32)
    tgt = (lab[rows.long()] == lab[cols.long()]).to(torch.uint8)
    out = torch.empty(10, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.xvec_eval_workspace_bytes(n * n), dtype=torch.uint8, device=dev)
    small = lambda: lib.xvec_eval_trials(S.data_ptr(), n, n, n, rows.data_ptr(), cols.data_ptr(), tgt.data_ptr(), n_trials, 1.0, 1.0, 0.5,
                                             out.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    big = lambda: lib.xvec_eval_all_pairs(S.data_ptr(), n, n, n, lab.data_ptr(), lab.data_ptr(), 1, 1.0, 1.0, 0.5, out.data_ptr(),
                                              ws.data_ptr(), ws.numel(), stream())
    res = {}
    for name, fn, calls in (("trials", small, 20), ("all_pairs", big, 3)):
        assert fn() == 0
        torch.cuda.synchronize()
        ts = []
        for _ in range(ROUNDS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) / calls)
        res[name] = float(np.median(ts))
    res["build"] = lib.xvec_version().decode().split()[-1]
    print(json.dumps(res))


if len(sys.argv) > 2 and sys.argv[1] == "--eval-child":
    eval_child(sys.argv[2])
    sys.exit(0)

import boot_ref as br
from xvector_amd import bootstrap, hip

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


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


fmt = lambda t: f"{t[0]:10.3f} ms ({t[1]:.3f}, {t[2]:.3f})"
say(f"Bootstrap timing: one MI355X, build {hip.version().split()[-1]} (xvec_version()), `python profiles/diag/boot_timing.py`.")
say(f"{n} x {n} fp64 score matrix (target scores N(-22, 24), non-target scores N(-50, 27)); joint resampling of the speakers of both")
say(f"sides; device time per call from hipEvents, {ROUNDS} rounds with the candidates interleaved, medians (min, max).  The library calls")
say("themselves: no label look-up, no read-back inside the timed region.  HBM figure: 8.0 TB/s.")
say()
rng = np.random.default_rng(0)
rows, cols = rng.integers(0, n, n_trials), rng.integers(0, n, n_trials)
row_d, col_d = (torch.from_numpy(a.astype(np.int32)).to(dev) for a in (rows, cols))


def torch_replicates(keys_sorted, gr, gc, bit, tabs, batch, c_miss=1.0, c_fa=1.0, p_target=0.5):
    """Baseline (a): the replicates of `tabs` [R, G] (int64 count tables, row 0 all ones) over the sorted trials, `batch` at a
    time: gather of the weights, two cumsums, both objectives at the run ends, arg-min.  Returns [R, 2] (eer, min_dcf)."""
    last = torch.ones_like(keys_sorted, dtype=torch.bool)
    last[:-1] = keys_sorted[1:] != keys_sorted[:-1]
    big = torch.iinfo(torch.int64).max
    out = []
    for b0 in range(0, tabs.shape[0], batch):
        t = tabs[b0:b0 + batch]
        w = t[:, gr] * t[:, gc]
        ta = torch.cumsum(w, 1)
        tp = torch.cumsum(w * bit, 1)
        P, A = tp[:, -1:], ta[:, -1:]
        N = A - P
        fa = N - (ta - tp)
        cand = last & (ta > 0)
        obj = torch.where(cand, (fa * P - tp * N).abs(), big)
        k = obj.argmin(1, keepdim=True)
        frr, far = tp.double() / P.double(), fa.double() / N.double()
        eer = (far.gather(1, k) + frr.gather(1, k)) / 2
        dcf = torch.where(cand, c_miss * frr * p_target + c_fa * far * (1 - p_target), float("inf")).min(1, keepdim=True).values
        out.append(torch.cat([eer, dcf], 1))
    return torch.cat(out)


def numpy_replicates(srt, n_boot, seed):
    """Baseline (b)'s replicate loop: tests/boot_ref.py, vectorised over the trials, one replicate after the other."""
    return [br.replicate(srt, srt.weights(seed, b, True)) for b in range(n_boot + 1)]


def tables(seed, n_boot, g):
    t = np.ones((n_boot + 1, g), dtype=np.int64)
    for b in range(1, n_boot + 1):
        t[b] = br.group_counts(seed, b, 0, g)
    return torch.from_numpy(t).to(dev)


for speakers in (40, 1251):
    labels = np.arange(n) % speakers
    same = labels[:, None] == labels[None, :]
    host = np.where(same, rng.normal(-22.0, 24.0, (n, n)), rng.normal(-50.0, 27.0, (n, n)))
    S = torch.from_numpy(host).to(dev)
    lab_d = torch.from_numpy(labels.astype(np.int32)).to(dev)
    tgt = (labels[rows] == labels[cols]).astype(np.uint8)
    tgt_d = torch.from_numpy(tgt).to(dev)
    for pairs, n_boot in ((False, 1000), (True, 100)):
        m = n * n if pairs else n_trials
        ws = torch.empty(int(hip.lib.xvec_boot_workspace_bytes(m, n_boot, speakers, speakers)), dtype=torch.uint8, device=dev)
        rec = torch.empty((n_boot + 1, 8), dtype=torch.float64, device=dev)
        summ = torch.empty(5, dtype=torch.int64, device=dev)
        params = hip.BootParams(lab_d.data_ptr(), lab_d.data_ptr(), speakers, speakers, 1, n_boot, 5, 1.0, 1.0, 0.5)
        one = hip.BootParams(lab_d.data_ptr(), lab_d.data_ptr(), speakers, speakers, 1, 1, 5, 1.0, 1.0, 0.5)
        if pairs:
            boot = lambda p=params: hip.lib.xvec_boot_all_pairs(S.data_ptr(), n, n, n, lab_d.data_ptr(), lab_d.data_ptr(), 1, C.byref(p),
                                                                summ.data_ptr(), rec.data_ptr(), ws.data_ptr(), ws.numel(), stream())
        else:
            boot = lambda p=params: hip.lib.xvec_boot_trials(S.data_ptr(), n, n, n, row_d.data_ptr(), col_d.data_ptr(), tgt_d.data_ptr(), n_trials,
                                                             C.byref(p), summ.data_ptr(), rec.data_ptr(), ws.data_ptr(), ws.numel(), stream())
        assert boot() == 0, hip.lib.xvec_boot_last_error().decode()
        torch.cuda.synchronize()
        got = rec.clone()
        # the sort alone: xvec_eval_sorted_order (the same gather and the same four passes, the index as the payload)
        keys = torch.empty(m, dtype=torch.int32, device=dev)
        order = torch.empty(m, dtype=torch.int32, device=dev)
        if pairs:
            sort = lambda: hip.lib.xvec_eval_sorted_order_all_pairs(S.data_ptr(), n, n, n, lab_d.data_ptr(), lab_d.data_ptr(), 1, keys.data_ptr(),
                                                                    order.data_ptr(), ws.data_ptr(), ws.numel(), stream())
        else:
            sort = lambda: hip.lib.xvec_eval_sorted_order(S.data_ptr(), n, n, n, row_d.data_ptr(), col_d.data_ptr(), tgt_d.data_ptr(), n_trials,
                                                          keys.data_ptr(), order.data_ptr(), ws.data_ptr(), ws.numel(), stream())
        assert sort() == 0, hip.lib.xvec_eval_last_error().decode()
        # baseline (a): torch on the same device.  The count tables come from the host (not timed: the library draws its own)
        tabs = tables(5, n_boot, speakers)
        if pairs:
            ii = torch.arange(n, device=dev).repeat_interleave(n)
            jj = torch.arange(n, device=dev).repeat(n)
            off = ii != jj
            ii, jj = ii[off], jj[off]
        else:
            ii, jj = row_d.long(), col_d.long()
        bit_all = (lab_d[ii] == lab_d[jj]).to(torch.int64)
        batch = 2 if pairs else 125

        def torch_boot():
            s32 = S[ii, jj].to(torch.float32)
            ks, perm = torch.sort(s32, stable=True)
            return torch_replicates(ks, lab_d[ii][perm].long(), lab_d[jj][perm].long(), bit_all[perm], tabs, batch)
        ref = torch_boot()
        ok = ~torch.isnan(got[:, 0])
        assert torch.equal(ref[ok, 0], got[ok, 0]) and (ref[ok, 1] - got[ok, 4]).abs().max() < 1e-15, "torch baseline and library disagree"
        del ref
        t_boot, t_one, t_sort, t_torch = interleaved([boot, lambda: boot(one), sort, torch_boot])
        reps = t_boot[0] - t_sort[0]
        say(f"{'all ' + str(n) + '^2 cells (' + str(m - n) + ' trials off the diagonal)' if pairs else 'the ' + str(m) + '-trial list'}, "
            f"{speakers} speaker groups, n_boot = {n_boot}: {int(summ[3])} degenerate replicates, workspace {ws.numel() / 2 ** 20:.1f} MiB, "
            f"batches of {hip.lib.xvec_boot_batch(m, n_boot)} records, {hip.lib.xvec_boot_batches(m, n_boot)} of them")
        say(f"    library, n_boot = {n_boot:4d}                         {fmt(t_boot)}")
        say(f"    library, n_boot = 1 (gather, sort, one batch)     {fmt(t_one)}")
        say(f"    gather and sort alone (xvec_eval_sorted_order)    {fmt(t_sort)}   {100 * t_sort[0] / t_boot[0]:5.1f} % of the call")
        say(f"    the replicate passes (the difference)             {reps:10.3f} ms   {reps / (n_boot + 1) * 1e3:8.1f} us per record, "
            f"{(n_boot + 1) * m / (reps * 1e-3) / 1e9:7.2f} G weighted items / s")
        rate = (n_boot + 1) * m / (reps * 1e-3)
        say(f"    per weighted item the two passes read (4 + 8) / 8 = 1.5 bytes of the sorted arrays (a tile is loaded once per 8 replicates) and two")
        say(f"    16-bit counts from L2: {1.5 * rate / 1e12:.3f} TB/s = {100 * 1.5 * rate / HBM:.1f} % of HBM.  The passes are bound by their arithmetic, not by")
        say(f"    memory: a weighted item costs {256 * 64 * 2.4e9 / rate:.0f} lane-cycles of the 256 x 64 lanes at 2.4 GHz (weights, two 64-bit running")
        say(f"    sums, and at a candidate two 64-bit cross products and two fp64 quotients), at 2 waves per SIMD")
        say(f"    (a) torch ops, same device, batches of {batch:3d}        {fmt(t_torch)}   torch / library {t_torch[0] / t_boot[0]:6.2f} x")
        if not pairs:
            t0 = time.perf_counter()
            host_scores = S.cpu().numpy()
            srt = br.Sorted.trials(host_scores, rows, cols, tgt, labels, labels, speakers, speakers)
            t_copy = time.perf_counter() - t0
            t0 = time.perf_counter()
            refs = numpy_replicates(srt, 100, 5)
            t_np = (time.perf_counter() - t0) / 101 * (n_boot + 1)
            for b in (0, 1, 50, 100):
                assert refs[b]["n_target"] == int(got[b, 6:8].view(torch.int64)[0]) and (np.isnan(refs[b]["eer"]) or refs[b]["eer"] == float(got[b, 0]))
            say(f"    (b) host: copy of the matrix, gather, sort {t_copy * 1e3:8.1f} ms + numpy replicates {t_np * 1e3:9.1f} ms (101 measured, scaled to "
                f"{n_boot + 1}; wall clock)   host / library {(t_copy + t_np) * 1e3 / t_boot[0]:7.1f} x")
        say()
        del ws, tabs, bit_all, ii, jj, keys, order
    del S

parent = sys.argv[2] if len(sys.argv) > 2 else None
if parent and os.path.exists(parent):
    say(f"xvec_eval_trials ({n_trials} trials) and xvec_eval_all_pairs ({n}^2 cells) on this build and on the parent commit's library: a fresh")
    say(f"process per library and round, {ROUNDS} rounds alternating, each the median of {ROUNDS} timings; median over the rounds (min, max)")
    res = {"this": [], "parent": []}
    for _ in range(ROUNDS):
        for name in ("this", "parent"):
            path = os.path.abspath(parent) if name == "parent" else hip.LIB_PATH
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--eval-child", path], capture_output=True, text=True, timeout=300)
            line = [x for x in out.stdout.splitlines() if x.startswith("{")]
            assert out.returncode == 0 and line, out.stderr[-800:]
            res[name].append(json.loads(line[-1]))
    for key in ("trials", "all_pairs"):
        a, b = ([r[key] for r in res[name]] for name in ("this", "parent"))
        say(f"    {key:10s} this build ({res['this'][0]['build']}) {np.median(a):9.4f} ms ({min(a):.4f}, {max(a):.4f})   parent ({res['parent'][0]['build']}) "
            f"{np.median(b):9.4f} ms ({min(b):.4f}, {max(b):.4f})   this / parent {np.median(a) / np.median(b):6.3f}")
else:
    say("(no parent library given: the comparison of xvec_eval_trials / xvec_eval_all_pairs with the parent commit was not run)")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
