"""Timing of DER scoring (xvector_amd.der, csrc/der.hip): xvec_der_score on (A) the diarization workload, 64 recordings x 3000
ticks with about 40 turns a side, and (B) 16 recordings x 360000 ticks (an hour at 10 ms), 8 speakers, 5 % overlap, collar 25.
One box; device time from hipEvents, 7 rounds with the variants interleaved, medians.  Two baselines: (a) what a user does
without the kernels -- the device turns copied to the host and tests/der_ref.py (numpy masks, scipy's assignment) per recording
on one thread, wall time with the copy included; (b) the same arithmetic in torch ops on the device (difference arrays and a
cumulative sum for the per-tick speaker sets, a matrix product per recording for C) with scipy behind a copy of C.  The parts by
difference: the front (memset, raster, pass, copy out) through xvec_der_cooccurrence, the same with no turns (what the ticks
alone cost), and the solver alone through xvec_der_assign on the matrices of the workload and on full 64 x 64 ones.
Writes profiles-style text to the path given as the first argument (default: standard output only)."""
import ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from scipy.optimize import linear_sum_assignment
import der_ref
from xvector_amd import der as der_mod, hip

dev = "cuda:0"
ROUNDS, BASE_ROUNDS, HBM = 7, 3, 8.0e12
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def interleaved(fns, timers, rounds):
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for q in range(max(rounds)):
        for t, fn, timer, n in zip(ts, fns, timers, rounds):
            if q < n:
                t.append(timer(fn))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


def conversation(rng, rec, n, n_spk, mean_len, overlap):
    """Reference turns of one recording: speakers alternate in turns of about mean_len ticks, short pauses, and with
    probability `overlap`-ish the next speaker starts before the last one ends."""
    out, t, last = [], 0, -1
    while t < n:
        spk = int(rng.integers(0, n_spk))
        if spk == last:
            continue
        length = int(rng.geometric(1.0 / mean_len))
        start = t - int(rng.integers(0, mean_len // 2)) if out and rng.random() < 4.0 * overlap else t + int(rng.integers(0, mean_len // 8 + 1))
        start = max(start, 0)
        if start >= n:
            break
        out.append([rec, start, min(start + length, n), spk])
        t, last = start + length, spk
    return out


def system_output(rng, ref, n_spk, jitter):
    """A hypothesis: the reference with its boundaries moved by up to `jitter` ticks, a tenth of the turns given to another
    speaker, the speaker numbers permuted."""
    hyp = ref.copy()
    hyp[:, 1] += rng.integers(-jitter, jitter + 1, len(hyp))
    hyp[:, 2] += rng.integers(-jitter, jitter + 1, len(hyp))
    hyp = hyp[hyp[:, 2] > hyp[:, 1]]
    wrong = rng.random(len(hyp)) < 0.1
    hyp[wrong, 3] = rng.integers(0, n_spk, int(wrong.sum()))
    hyp[:, 3] = rng.permutation(n_spk)[hyp[:, 3]]
    return hyp


def torch_der(ref, hyp, rs, n_spk, collar):
    """The same arithmetic in torch ops on the device; the mapping by scipy behind a copy of C.  ref / hyp: device int64 turns."""
    N, n_rec = int(rs[-1]), len(rs) - 1
    base = torch.as_tensor(rs[:-1], device=dev)
    length = torch.as_tensor(np.diff(rs), device=dev)

    def active(t):
        b, n = base[t[:, 0]], length[t[:, 0]]
        lo, hi = b + t[:, 1].clamp(min=0), b + torch.minimum(t[:, 2], n)
        d = torch.zeros((N + 1, n_spk), dtype=torch.int32, device=dev)
        one = torch.ones(len(t), dtype=torch.int32, device=dev)
        d.index_put_((lo, t[:, 3]), one, accumulate=True)
        d.index_put_((hi, t[:, 3]), -one, accumulate=True)
        return (d.cumsum(0)[:N] > 0)

    R, H = active(ref), active(hyp)
    scored = torch.ones(N, dtype=torch.bool, device=dev)
    if collar:
        d = torch.zeros(N + 1, dtype=torch.int32, device=dev)
        for col in (1, 2):
            b, n = base[ref[:, 0]], length[ref[:, 0]]
            lo, hi = b + (ref[:, col] - collar).clamp(min=0), b + torch.minimum(ref[:, col] + collar, n)
            one = torch.ones(len(ref), dtype=torch.int32, device=dev)
            d.index_put_((lo,), one, accumulate=True)
            d.index_put_((hi,), -one, accumulate=True)
        scored = d.cumsum(0)[:N] == 0
    nref, nhyp = R.sum(1), H.sum(1)
    Rf, Hf = (R & scored[:, None]).to(torch.float64), H.to(torch.float64)
    C = torch.stack([Rf[a:b].T @ Hf[a:b] for a, b in zip(rs[:-1], rs[1:])])
    seg = torch.repeat_interleave(torch.arange(n_rec, device=dev), length)
    sums = torch.zeros((n_rec, 4), dtype=torch.int64, device=dev)
    vals = torch.stack([nref, (nref - nhyp).clamp(min=0), (nhyp - nref).clamp(min=0), torch.minimum(nref, nhyp)], 1) * scored[:, None]
    sums.index_add_(0, seg, vals)
    Ch = C.cpu().numpy()
    correct = np.array([Ch[r][linear_sum_assignment(Ch[r], maximize=True)].sum() for r in range(n_rec)])
    s = sums.cpu().numpy()
    return (s[:, 1] + s[:, 2] + s[:, 3] - correct).sum() / s[:, 0].sum()


fmt = lambda t: f"{t[0]:10.3f} ms ({t[1]:.3f}, {t[2]:.3f})"
say(f"DER timing: one MI355X, build {hip.version().split()[-1]} (xvec_version()), `python profiles/diag/der_timing.py`.")
say(f"Device time per call from hipEvents, {ROUNDS} rounds with the variants interleaved, medians (min, max); the baselines are wall time,")
say(f"{BASE_ROUNDS} rounds (1 for workload B).  host: the device turns copied to the host, tests/der_ref.py per recording on one thread (numpy masks,")
say("scipy's linear_sum_assignment), copy included; torch: difference arrays, cumulative sums and a matrix product per recording on the")
say("device, scipy behind a copy of C.  xvec_der_score is one memset and four launches whatever the batch.")
rng = np.random.default_rng(7)
WORK = (("A: 64 recordings x 3000 ticks, 4 speakers, about 40 turns a side, collar 0", 64, 3000, 4, 75, 0.0, 0, 10),
        ("B: 16 recordings x 360000 ticks, 8 speakers, 5 % overlap, collar 25", 16, 360000, 8, 300, 0.05, 25, 30))
for title, n_rec, n, n_spk, mean_len, overlap, collar, jitter in WORK:
    ref = np.asarray([row for r in range(n_rec) for row in conversation(rng, r, n, n_spk, mean_len, overlap)], dtype=np.int64)
    hyp = system_output(rng, ref, n_spk, jitter)
    rec_len = [n] * n_rec
    rs = np.concatenate([[0], np.cumsum(rec_len)]).astype(np.int64)
    N = int(rs[-1])
    rd, hd = torch.from_numpy(ref.astype(np.int32)).to(dev), torch.from_numpy(hyp.astype(np.int32)).to(dev)
    r64, h64 = rd.to(torch.int64), hd.to(torch.int64)
    rs_c = (ctypes.c_int64 * len(rs))(*rs.tolist())
    need = int(hip.lib.xvec_der_workspace_bytes(rs_c, n_rec, len(ref), len(hyp)))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.empty((n_rec, 5), dtype=torch.int64, device=dev)
    mapping = torch.empty((n_rec, 64), dtype=torch.int32, device=dev)
    rate = torch.empty(n_rec + 1, dtype=torch.float64, device=dev)
    ign = torch.empty(2, dtype=torch.int64, device=dev)
    cooc = torch.empty((n_rec, 64, 64), dtype=torch.int64, device=dev)
    correct = torch.empty(n_rec, dtype=torch.int64, device=dev)
    st = lambda: torch.cuda.current_stream().cuda_stream

    def score():
        assert hip.lib.xvec_der_score(rd.data_ptr(), len(ref), hd.data_ptr(), len(hyp), rs_c, n_rec, collar, 0, counts.data_ptr(),
                                      mapping.data_ptr(), rate.data_ptr(), ign.data_ptr(), None, ws.data_ptr(), need, st()) == 0

    def front(m_ref=len(ref), m_hyp=len(hyp)):
        assert hip.lib.xvec_der_cooccurrence(rd.data_ptr(), m_ref, hd.data_ptr(), m_hyp, rs_c, n_rec, collar, 0, counts.data_ptr(),
                                             cooc.data_ptr(), ign.data_ptr(), ws.data_ptr(), need, st()) == 0

    def solver():
        assert hip.lib.xvec_der_assign(cooc.data_ptr(), n_rec, mapping.data_ptr(), correct.data_ptr(), st()) == 0

    def host():
        hr, hh = rd.cpu().numpy(), hd.cpu().numpy()
        return der_ref.der(hr, hh, rec_len, collar)["der"][n_rec]

    front()
    torch.cuda.synchronize()
    big = N > 10 ** 6
    module = lambda: der_mod.der(rd, hd, rec_len, collar=collar, workspace=ws)
    t_s, t_f, t_0, t_a, t_m, t_h, t_t = interleaved(
        [score, front, lambda: front(0, 0), solver, module, host, lambda: torch_der(r64, h64, rs, n_spk, collar)],
        [once, once, once, once, wall, wall, wall], [ROUNDS] * 5 + [1 if big else BASE_ROUNDS] * 2)
    score()
    got, want, via_torch = float(rate[n_rec]), float(host()), float(torch_der(r64, h64, rs, n_spk, collar))
    say()
    say(f"{title}: {len(ref)} reference and {len(hyp)} hypothesis turns, {N} ticks, workspace {need / 2 ** 20:.1f} MiB;")
    say(f"  pooled DER {got:.6f}, equal to the host form's: {got == want}, to the torch form's: {got == via_torch}")
    say(f"  xvec_der_score                 {fmt(t_s)}")
    say(f"  der.der (module, wall, with the copy of `ignored`) {fmt(t_m)}")
    say(f"  front: memset + raster + pass + copy out of C  {fmt(t_f)}   with no turns (the ticks alone) {fmt(t_0)}")
    mask_bytes = 16.0 * N
    say(f"    the pass reads 16 bytes a tick = {mask_bytes / 1e6:.1f} MB, the memset writes as much: over the no-turn front {2 * mask_bytes / (t_0[0] * 1e-3) / 1e12:.3f} TB/s "
        f"= {100 * 2 * mask_bytes / (t_0[0] * 1e-3) / HBM:.1f} % of {HBM / 1e12:.1f} TB/s; over the whole front {2 * mask_bytes / (t_f[0] * 1e-3) / 1e12:.3f} TB/s")
    say(f"  solver alone (xvec_der_assign on these matrices) {fmt(t_a)}   = {1e3 * t_a[0] / n_rec:.2f} us a recording in one launch of {n_rec} waves")
    say(f"  host                           {fmt(t_h)}   host / xvec_der_score {t_h[0] / t_s[0]:9.1f} x")
    say(f"  torch + scipy                  {fmt(t_t)}   torch / xvec_der_score {t_t[0] / t_s[0]:8.1f} x")
    del ws, cooc

# the solver on matrices no tick count of these workloads produces: full 64 x 64, entries up to 2^31 - 1
say()
for n_mat in (1, 64, 1024):
    mats = torch.from_numpy(np.random.default_rng(n_mat).integers(0, 2 ** 31, (n_mat, 64, 64))).to(dev)
    mp = torch.empty((n_mat, 64), dtype=torch.int32, device=dev)
    cr = torch.empty(n_mat, dtype=torch.int64, device=dev)
    run = lambda: hip.lib.xvec_der_assign(mats.data_ptr(), n_mat, mp.data_ptr(), cr.data_ptr(), torch.cuda.current_stream().cuda_stream)
    hm = mats.cpu().numpy()
    sci = lambda: [linear_sum_assignment(m, maximize=True) for m in hm]
    t_d, t_c = interleaved([run, sci], [once, wall], [ROUNDS, BASE_ROUNDS])
    ok = all(int(c) == int(m[linear_sum_assignment(m, maximize=True)].sum()) for c, m in zip(cr.cpu().numpy()[:8], hm[:8]))
    say(f"xvec_der_assign, {n_mat:5d} full random 64 x 64 matrices {fmt(t_d)} = {1e3 * t_d[0] / n_mat:8.2f} us a matrix; scipy on one thread "
        f"{fmt(t_c)} = {1e3 * t_c[0] / n_mat:8.2f} us a matrix; optimum equal: {ok}")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
