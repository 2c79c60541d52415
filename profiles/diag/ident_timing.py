"""Timing of speaker identification (xvector_amd.identify): per-model means of 3 enrolment vectors per model, open-set scores
and the k best models per test column, at 1251 models (VoxCeleb1's speakers) and at 10 000, against the reference's 4874 test
segments.  Device time from hipEvents around 5 calls, 7 rounds with the library and the torch baseline interleaved, medians
over the rounds, one box.  The baseline is the same work in torch ops on the same device: the mean by index_add_ and a
division; the open-set scores by the library's own cancellation-free form (column max and argmax, exp(S - max) with the
maximum's own term masked out by scatter_, its column sum, 1 + (R - e) per cell, the two-sided logarithm by torch.where); the
k best by torch.topk(dim=0).  Writes profiles-style text to the path given as the first argument (default: standard output
only)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from xvector_amd import hip, identify

dev = "cuda:0"
T, dim, SESSIONS, ROUNDS, CALLS, HBM = 4874, 512, 3, 7, 5, 8.0e12
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


def torch_open_set(S, p):
    N = S.shape[0]
    m1, i1 = S.max(dim=0)
    E = torch.exp(S - m1[None, :])
    E.scatter_(0, i1[None, :], 0.0)
    R = E.sum(dim=0)
    A = 1.0 + (R[None, :] - E)
    A.scatter_(0, i1[None, :], R[None, :])
    q = (p * A) / (N - 1)
    shifted = (m1 > 0) | (p == 1.0)
    up = m1[None, :] + torch.log(q + ((1.0 - p) * torch.exp(-m1))[None, :])
    down = torch.log(torch.exp(m1)[None, :] * q + (1.0 - p))
    return S - torch.where(shifted[None, :], up, down)


fmt = lambda t: f"{t[0]:8.3f} ms ({t[1]:.3f}, {t[2]:.3f})"
say(f"Speaker identification timing: one MI355X, build {hip.version().split()[-1]} (xvec_version()), `python profiles/diag/ident_timing.py`.")
say(f"{T} test columns (the reference's test set), fp64 N(-20, 15) scores; device time per call from hipEvents around {CALLS} calls,")
say(f"{ROUNDS} rounds with the library and the torch baseline interleaved, medians (min, max).  Rates: the algorithm's own bytes (the")
say("enrolment vectors once; S once in and once out for the open-set scores; S once for the k best) over the time, against the")
say("8.0 TB/s HBM figure.  The open-set kernels read S twice (column statistics, then the scores).")
gen = torch.Generator(device=dev).manual_seed(0)
for N in (1251, 10000):
    say()
    say(f"N = {N} models")
    n = N * SESSIONS
    x = torch.randn((n, dim), dtype=torch.float64, device=dev, generator=gen)
    names = np.random.default_rng(N).permutation(np.repeat(np.arange(N), SESSIONS))
    _, order, start = identify.group_models(names)
    cls = torch.from_numpy(names.astype(np.int64)).to(dev)
    counts = torch.full((N, 1), float(SESSIONS), dtype=torch.float64, device=dev)
    ours = lambda: identify.enroll(x, names, device=dev)

    def ours_call(out=torch.empty((N, dim), dtype=torch.float64, device=dev), order_d=torch.from_numpy(order).to(dev),
                  ws=torch.empty(int(hip.lib.xvec_model_mean_workspace_bytes(N)), dtype=torch.uint8, device=dev)):
        hip.lib.xvec_model_mean(x.data_ptr(), hip.IDENT_X_F64, n, dim, dim, order_d.data_ptr(),
                                start.ctypes.data_as(hip.C.POINTER(hip.C.c_int64)), N, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                torch.cuda.current_stream(dev).cuda_stream)
        return out

    base = lambda: torch.zeros((N, dim), dtype=torch.float64, device=dev).index_add_(0, cls, x) / counts
    t_o, t_c, t_b = interleaved([ours, ours_call, base])
    err = float((ours().vectors - base()).abs().max())
    rate = n * dim * 8 / (t_c[0] * 1e-3)
    say(f"  model means of {n} x {dim} (xvec_model_mean; torch: index_add_ and a division)")
    say(f"    library call {fmt(t_c)}   enroll() with its host grouping and upload {fmt(t_o)}   torch {fmt(t_b)}   "
        f"torch / library call {t_b[0] / t_c[0]:6.2f} x   {rate / 1e12:.2f} TB/s = {100 * rate / HBM:.0f} % of HBM   (largest difference to torch {err:.1e})")
    del x

    S = torch.randn((N, T), dtype=torch.float64, device=dev, generator=gen) * 15.0 - 20.0
    S[torch.randint(0, N, (T,), device=dev, generator=gen), torch.arange(T, device=dev)] += 80.0          # a target per column
    out = torch.empty_like(S)
    ws = torch.empty(int(hip.lib.xvec_ident_workspace_bytes(N, T, identify.MAX_K)), dtype=torch.uint8, device=dev)
    for p in (0.1,):
        ours = lambda: identify.open_set_scores(S, p, out=out, workspace=ws)
        base = lambda: torch_open_set(S, p)
        t_o, t_b = interleaved([ours, base])
        err = float((ours() - base()).abs().max())
        rate = 2 * N * T * 8 / (t_o[0] * 1e-3)
        say(f"  open-set scores, p_known = {p} (xvec_open_set_scores, out of place; torch: max, exp, scatter_, sum, log, where)")
        say(f"    library {fmt(t_o)}   torch {fmt(t_b)}   torch / library {t_b[0] / t_o[0]:6.2f} x   "
            f"{rate / 1e12:.2f} TB/s = {100 * rate / HBM:.0f} % of HBM   (largest difference to torch {err:.1e})")
    del out
    say("  the k best models per column (xvec_identify_topk with a threshold; torch: topk(dim=0))")
    for k in (1, 4, identify.MAX_K):
        ours = lambda: identify.identify(S, k, threshold=0.0, workspace=ws)
        base = lambda: torch.topk(S, k, dim=0)
        t_o, t_b = interleaved([ours, base])
        same = bool(torch.equal(ours().scores, base().values))
        rate = N * T * 8 / (t_o[0] * 1e-3)
        say(f"    k = {k:2d}: library {fmt(t_o)}   torch {fmt(t_b)}   torch / library {t_b[0] / t_o[0]:6.2f} x   "
            f"{rate / 1e12:.2f} TB/s = {100 * rate / HBM:.0f} % of HBM   (scores equal to torch's: {same})")
    del S, ws
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
