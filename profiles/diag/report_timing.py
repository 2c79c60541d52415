"""Timing of the trial report (xvector_amd.report) at the reference's test-set size: the 4874 x 4874 score matrix with the
37 720-trial list.  The trial map, the range and all six uint8 images against the same arithmetic in torch ops on the same
device and against a copy to the host followed by the numpy restatement (tests/report_ref.py); the DET curve at grid 0 and 1000
for the list and for all pairs against torch.sort + cumsum + unique_consecutive.  Device time from hipEvents around 3 calls, 7
rounds with the library and the torch baseline interleaved, medians over the rounds, one box; the host path in wall-clock time,
once.  Writes profiles-style text to the path given as the first argument (default: standard output only)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from xvector_amd import evaluate as ev, hip, report

dev = "cuda:0"
n, n_trials, ROUNDS, CALLS, HBM = 4874, 37720, 7, 3, 8.0e12
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


def must(rc):
    """Every timed library call goes through it: a refused call would otherwise be timed as a fast success."""
    assert rc == 0, hip.lib.xvec_report_last_error().decode()


fmt = lambda t: f"{t[0]:9.3f} ms ({t[1]:.3f}, {t[2]:.3f})"
stream = lambda: torch.cuda.current_stream(dev).cuda_stream
say(f"Trial report timing: one MI355X, build {hip.version().split()[-1]} (xvec_version()), `python profiles/diag/report_timing.py`.")
say(f"{n} x {n} fp64 score matrix (the reference's test set), target scores N(-22, 24), non-target scores N(-50, 27), 40 speakers,")
say(f"the {n_trials}-trial list; device time per call from hipEvents around {CALLS} calls, {ROUNDS} rounds with the library and the torch")
say("baseline interleaved, medians (min, max).  Host path: wall-clock time, once.  Rates against the 8.0 TB/s HBM figure.")
say()
rng = np.random.default_rng(0)
labels = np.arange(n) % 40
same = labels[:, None] == labels[None, :]
host = np.where(same, rng.normal(-22.0, 24.0, (n, n)), rng.normal(-50.0, 27.0, (n, n)))
host = np.triu(host) + np.triu(host, 1).T
S = torch.from_numpy(host).to(dev)
rows, cols = rng.integers(0, n, n_trials), rng.integers(0, n, n_trials)
trials = ev.TrialList(rows, cols, labels[rows] == labels[cols])
row_d, col_d, tgt_d = trials.on(dev)
res = ev.evaluate_trials(S, trials)
e_th, m_th = res.eer_th, res.min_dcf_th

# ---------------------------------------------------------------- images
ld_map = (n + 3) // 4 * 4
map_buf = torch.empty((n, ld_map), dtype=torch.uint8, device=dev)
bad = torch.empty(1, dtype=torch.int64, device=dev)
rec = torch.empty(3, dtype=torch.float64, device=dev)
rws = torch.empty(int(hip.lib.xvec_report_range_workspace_bytes()), dtype=torch.uint8, device=dev)
outs = [torch.empty(report._image_shape(i, n, n), dtype=torch.uint8, device=dev) for i in range(6)]
lib_map = lambda: must(hip.lib.xvec_report_trial_map(row_d.data_ptr(), col_d.data_ptr(), tgt_d.data_ptr(), n_trials, n, n, map_buf.data_ptr(),
                                                ld_map, bad.data_ptr(), stream()))
lib_range = lambda: must(hip.lib.xvec_report_range(S.data_ptr(), n, n, n, rec.data_ptr(), rws.data_ptr(), rws.numel(), stream()))
lib_images = lambda which=63: must(hip.lib.xvec_report_images(S.data_ptr(), n, n, n, map_buf.data_ptr(), ld_map, rec.data_ptr(), e_th, m_th, which, 0,
                                                         *[o.data_ptr() for o in outs], stream()))


def lib_all():
    lib_map()
    lib_range()
    lib_images()


def u8(x):
    return (x.to(torch.float32) * 255.0).nan_to_num(0.0).clamp(0.0, 255.0).to(torch.uint8)


def torch_all():
    """The same arithmetic in torch ops: masks, finite range, normalisation, the six uint8 images."""
    t = tgt_d.bool()
    pos = torch.zeros((n, n), dtype=torch.float64, device=dev)
    neg = torch.zeros((n, n), dtype=torch.float64, device=dev)
    pos[row_d[t].long(), col_d[t].long()] = 1
    neg[row_d[~t].long(), col_d[~t].long()] = 1
    fin = torch.isfinite(S)
    mn = torch.where(fin, S, torch.inf).min()
    mx = torch.where(fin, S, -torch.inf).max()
    v = (S - mn) / (mx - mn)
    zero = torch.zeros((n, n), dtype=torch.uint8, device=dev)
    imgs = [u8(v), torch.stack([u8(neg), u8(pos), zero]), torch.stack([u8(v * neg), u8(v * pos), zero])]
    k = pos + neg
    cv = k * S
    pp_e, pn_e, pp_m, pn_m = (cv >= e_th) * k, (cv < e_th) * k, (cv >= m_th) * k, (cv < m_th) * k
    for w1, w0 in ((1.0, 1.0), (pos, neg), (neg, pos)):
        img = torch.full((3, n, 2 * n + 5), 255, dtype=torch.uint8, device=dev)
        img[1, :, :n], img[0, :, :n] = u8(pp_e * w1), u8(pn_e * w0)
        img[1, :, -n:], img[0, :, -n:] = u8(pp_m * w1), u8(pn_m * w0)
        img[2, :, :n] = 0
        img[2, :, -n:] = 0
        imgs.append(img)
    return imgs


t_map, t_range, t_img, t_wide, t_all, t_torch = interleaved([lib_map, lib_range, lib_images, lambda: lib_images(8), lib_all, torch_all])
for got, want in zip(outs, torch_all()):
    assert torch.equal(got, want), "the torch baseline and the library disagree"
read_b = n * n * 9
write_b = sum(o.numel() for o in outs)
rate = (read_b + write_b) / (t_img[0] * 1e-3)
say("map + range + the six uint8 images")
say(f"  xvec_report_trial_map (memset + {n_trials} OR atomics)        {fmt(t_map)}")
say(f"  xvec_report_range (one read of the matrix)                {fmt(t_range)}   {n * n * 8 / (t_range[0] * 1e-3) / 1e12:.2f} TB/s = "
    f"{100 * n * n * 8 / (t_range[0] * 1e-3) / HBM:.0f} % of HBM")
say(f"  xvec_report_images, all six                               {fmt(t_img)}   reads {read_b / 1e6:.0f} MB (matrix + map, once), writes "
    f"{write_b / 1e6:.0f} MB: {rate / 1e12:.2f} TB/s = {100 * rate / HBM:.0f} % of HBM")
wide_b = outs[3].numel()
say(f"  xvec_report_images, prediction_eer_min_dcf alone          {fmt(t_wide)}   reads {read_b / 1e6:.0f} MB, writes {wide_b / 1e6:.0f} MB: "
    f"{(read_b + wide_b) / (t_wide[0] * 1e-3) / 1e12:.2f} TB/s = {100 * (read_b + wide_b) / (t_wide[0] * 1e-3) / HBM:.0f} % of HBM")
say(f"  the three calls                                           {fmt(t_all)}")
say(f"  torch ops, the same arithmetic (bit-equal images)         {fmt(t_torch)}   torch / library {t_torch[0] / t_all[0]:6.2f} x")
import report_ref
t0 = time.perf_counter()
s_h = S.cpu().numpy()
t1 = time.perf_counter()
pos, neg, _ = report_ref.masks(trials.row_idx, trials.col_idx, trials.is_target, s_h.shape)
ref = report_ref.images(s_h, pos, neg, e_th, m_th)
t2 = time.perf_counter()
ref = {k: report_ref.to_u8(v) for k, v in ref.items()}
t3 = time.perf_counter()
assert all(np.array_equal(ref[name] if i else ref[name][0], outs[i].cpu().numpy()) for i, name in enumerate(report.IMAGE_NAMES))
say(f"  host path: copy of the matrix {1e3 * (t1 - t0):9.1f} ms, the numpy restatement (float64 images) {1e3 * (t2 - t1):9.1f} ms, to uint8 "
    f"{1e3 * (t3 - t2):9.1f} ms   host / library {1e3 * (t3 - t0) / t_all[0]:8.1f} x")
say()
del ref, pos, neg, s_h, outs, map_buf

# ---------------------------------------------------------------- the curve
lab_d = torch.from_numpy(labels.astype(np.int32)).to(dev)
head = torch.empty(5, dtype=torch.int64, device=dev)


def torch_curve(s, t):
    srt, idx = torch.sort(s.to(torch.float32))
    ctp = torch.cumsum(t[idx].to(torch.int64), 0)
    uniq, counts = torch.unique_consecutive(srt, return_counts=True)
    ends = torch.cumsum(counts, 0) - 1
    tp = ctp[ends]
    return uniq, tp, ends + 1 - tp


off = ~torch.eye(n, dtype=torch.bool, device=dev)
same_d = torch.from_numpy(same).to(dev)
for name, m, pairs in ((f"the {n_trials}-trial list", n_trials, False), (f"all {n}^2 cells ({n * n - n} trials off the diagonal)", n * n, True)):
    ws = torch.empty(int(hip.lib.xvec_report_det_workspace_bytes(m)), dtype=torch.uint8, device=dev)
    thr = torch.empty(m, dtype=torch.float32, device=dev)
    tp = torch.empty(m, dtype=torch.int64, device=dev)
    nn = torch.empty(m, dtype=torch.int64, device=dev)
    if pairs:
        lib = lambda grid: must(hip.lib.xvec_report_det_all_pairs(S.data_ptr(), n, n, n, lab_d.data_ptr(), lab_d.data_ptr(), 1, grid, head.data_ptr(),
                                                             thr.data_ptr(), tp.data_ptr(), nn.data_ptr(), m, ws.data_ptr(), ws.numel(), stream()))
        base = lambda: torch_curve(S[off], same_d[off])
    else:
        lib = lambda grid: must(hip.lib.xvec_report_det(S.data_ptr(), n, n, n, row_d.data_ptr(), col_d.data_ptr(), tgt_d.data_ptr(), m, grid,
                                                   head.data_ptr(), thr.data_ptr(), tp.data_ptr(), nn.data_ptr(), m, ws.data_ptr(), ws.numel(), stream()))
        base = lambda: torch_curve(S[row_d.long(), col_d.long()], tgt_d)
    lib(0)
    pts = int(head[0])
    want = base()
    assert pts == want[0].numel() and torch.equal(tp[:pts], want[1]) and torch.equal(nn[:pts], want[2]) and torch.equal(thr[:pts], want[0])
    t_0, t_g, t_t = interleaved([lambda: lib(0), lambda: lib(1000), base])
    lib(1000)
    say(f"DET curve, {name}: {pts} distinct scores, {int(head[0])} points at grid 1000; workspace {ws.numel() / 1e6:.1f} MB")
    say(f"  grid 0                                                    {fmt(t_0)}")
    say(f"  grid 1000                                                 {fmt(t_g)}")
    say(f"  torch: gather, sort, cumsum, unique_consecutive (bit-equal points)   {fmt(t_t)}   torch / library(grid 0) {t_t[0] / t_0[0]:6.2f} x")
    say()
    del ws, thr, tp, nn
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
