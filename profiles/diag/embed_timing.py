"""Timing of embedding conditioning (xvector_amd.lda) at the reference's sizes: the transform (centre -> LDA -> length norm,
xvec_embed_transform) and the pure centre / length-norm pass at N = 150 000 (its training set) and N = 4874 (its test set),
D = 512, R = 150, and the LDA statistics (xvec_lda_stats) at N = 150 000, C = 1211.  Device time from hipEvents around 5 calls,
7 rounds with the library and the torch baseline interleaved, medians over the rounds, one box.  The baseline is the same
work in torch ops on the same device: `(x.double() - mu) @ W` then `/ norm.clamp_min(1e-8)`; class sums by index_add_, then the
weighted centred rows times their transpose as one dgemm.  Writes profiles-style text to the path given as the first argument
(default: standard output only)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from xvector_amd import hip, lda, plda

dev = "cuda:0"
D, R, C, ROUNDS, CALLS = 512, 150, 1211, 7, 5
PEAK64, HBM = 78.6e12, 8.0e12            # the vendor's fp64 matrix figure and HBM figure
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
say(f"Embedding conditioning timing: one MI355X, build {hip.version().split()[-1]} (xvec_version()), `python profiles/diag/embed_timing.py`.")
say(f"D = {D}, R = {R}, C = {C}, fp32 x-vectors; device time per call from hipEvents around {CALLS} calls, {ROUNDS} rounds with the")
say("library and the torch baseline interleaved, medians (min, max).  Peak figures: the vendor's 78.6 TF fp64 matrix rate")
say("(VERDICT.md) and 8.0 TB/s HBM; FLOP and bytes are the algorithm's, from the shapes.")
gen = torch.Generator(device=dev).manual_seed(0)
mu = torch.randn(D, dtype=torch.float64, device=dev, generator=gen)
W = torch.randn((D, R), dtype=torch.float64, device=dev, generator=gen) / D ** 0.5
stream = lambda: torch.cuda.current_stream(dev).cuda_stream

for n in (150000, 4874):
    say()
    say(f"N = {n}")
    x = torch.randn((n, D), dtype=torch.float32, device=dev, generator=gen) + 0.5
    y = torch.empty((n, R), dtype=torch.float64, device=dev)
    yd = torch.empty((n, D), dtype=torch.float64, device=dev)
    ws = torch.empty(int(hip.lib.xvec_embed_transform_workspace_bytes(n, D, D)), dtype=torch.uint8, device=dev)

    def base_tf():
        t = (x.double() - mu) @ W
        return t / t.norm(dim=1, keepdim=True).clamp_min(1e-8)

    def base_norm():
        t = x.double() - mu
        return t / t.norm(dim=1, keepdim=True).clamp_min(1e-8)

    ours_tf = lambda: lda.embed_transform(x, mu, W, True, out=y, workspace=ws)
    ours_norm = lambda: lda.embed_transform(x, mu, None, True, out=yd, workspace=ws)
    t_o, t_b, t_on, t_bn = interleaved([ours_tf, base_tf, ours_norm, base_norm])
    err = float((ours_tf() - base_tf()).abs().max())
    flops = 2.0 * n * D * R
    say(f"  centre -> LDA -> length norm (one launch; torch: (x.double() - mu) @ W, / norm.clamp_min(1e-8))")
    say(f"    library {fmt(t_o)}   torch {fmt(t_b)}   torch / library {t_b[0] / t_o[0]:6.2f} x   "
        f"{flops / (t_o[0] * 1e-3) / 1e12:.1f} TF = {100 * flops / (t_o[0] * 1e-3) / PEAK64:.0f} % of the fp64 matrix peak   "
        f"(largest difference to torch {err:.1e})")
    byts = n * D * (4 + 8)
    say(f"  centre -> length norm, w == NULL (torch: x.double() - mu, / norm.clamp_min(1e-8))")
    say(f"    library {fmt(t_on)}   torch {fmt(t_bn)}   torch / library {t_bn[0] / t_on[0]:6.2f} x   "
        f"read fp32 + write fp64 {byts / (t_on[0] * 1e-3) / 1e12:.2f} TB/s = {100 * byts / (t_on[0] * 1e-3) / HBM:.0f} % of HBM")
    if n != 150000:
        continue
    labels = np.arange(n) % C
    classes, order, start = plda._labels(labels, n)
    order_d = torch.from_numpy(order).to(dev)
    lab_d = torch.from_numpy(labels).to(dev)
    cnt = torch.bincount(lab_d, minlength=C).double()
    f64 = dict(dtype=torch.float64, device=dev)
    outs = [torch.empty(D, **f64), torch.empty((C, D), **f64), torch.empty((D, D), **f64), torch.empty((D, D), **f64)]
    ws_s = torch.empty(int(hip.lib.xvec_lda_stats_workspace_bytes(n, D, C)), dtype=torch.uint8, device=dev)
    cs = start.ctypes.data_as(hip.C.POINTER(hip.C.c_int64))

    def ours_stats():
        rc = hip.lib.xvec_lda_stats(x.data_ptr(), hip.LDA_X_F32, n, D, order_d.data_ptr(), cs, C, *(t.data_ptr() for t in outs),
                                    ws_s.data_ptr(), ws_s.numel(), stream())
        assert rc == 0, hip.lib.xvec_lda_last_error()

    def base_stats():
        xd = x.double()
        sums = torch.zeros((C, D), **f64).index_add_(0, lab_d, xd)
        cm = sums / cnt[:, None]
        mean = sums.sum(0) / n
        t = xd - cm[lab_d]
        sw = (t / cnt[lab_d][:, None]).T @ t
        a = cm - mean
        return mean, cm, sw, a.T @ a

    t_o, t_b = interleaved([ours_stats, base_stats])
    ours_stats()
    ref = base_stats()
    err = max(float(((o - r).abs().max() / r.abs().max())) for o, r in zip(outs, ref))
    flops = 2.0 * n * D * D / 2 + 2.0 * C * D * D / 2           # the upper triangles
    say(f"  LDA statistics, C = {C} (xvec_lda_stats: 7 launches; torch: index_add_, one dgemm of the weighted centred rows, one of the class means)")
    say(f"    library {fmt(t_o)}   torch {fmt(t_b)}   torch / library {t_b[0] / t_o[0]:6.2f} x   "
        f"{flops / (t_o[0] * 1e-3) / 1e12:.1f} TF (triangle FLOP) = {100 * flops / (t_o[0] * 1e-3) / PEAK64:.0f} % of the fp64 matrix peak   "
        f"(largest difference to torch, relative to the largest element, {err:.1e})")
    del x, y, yd
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
