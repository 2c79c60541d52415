"""Timing of the embedding maps (xvector_amd.visualize) at N = 1200 (about one of the reference's four plotted groups) and
N = 4874 (its whole test set), D = 512: tsne_affinities, one iteration (with and without the KL pass) and its split by kernel
from torch.profiler, and Tsne.run() of 1000 iterations.  Device time from hipEvents, 7 rounds with the library and the
baseline interleaved (the baseline of an iteration: the same arithmetic in torch ops on the device, fp64), medians over the
rounds, one box.  Where scikit-learn is installed, TSNE(method='exact') (N = 1200 only: it takes minutes beyond) and the
default Barnes-Hut on the box's cores are timed once each by the wall clock.  Writes profiles-style text to the path given as
the first argument (default: standard output only)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))      # tsne_ref: the quality measures
import numpy as np, torch
import tsne_ref
from xvector_amd import hip, visualize

dev = "cuda:0"
DIM, ROUNDS, HBM, F64_VECTOR, PAIR_OPS = 512, 7, 8.0e12, 78.6e12, 19      # the public HBM and fp64 vector figures of the MI355X
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


def interleaved(fns, calls):
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(ROUNDS):
        for t, fn in zip(ts, fns):
            t.append(once(fn, calls))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


def planted(n, seed=0):
    rng = np.random.default_rng(seed)
    labels = np.arange(n) % 40
    return (4.0 * rng.standard_normal((40, DIM))[labels] + rng.standard_normal((n, DIM))).astype(np.float32), labels


def torch_iteration(P, Y, update, gains, exaggeration, momentum, lr):
    diff = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + (diff * diff).sum(-1))
    w.fill_diagonal_(0.0)
    Z = w.sum()
    grad = 4.0 * ((((exaggeration * P) * w)[:, :, None] * diff).sum(1) - ((w * w)[:, :, None] * diff).sum(1) / Z)
    inc = update * grad < 0.0
    gains.copy_(torch.where(inc, gains + 0.2, gains * 0.8).clamp_min(0.01))
    update.mul_(momentum).sub_(lr * gains * grad)
    Y.add_(update)


fmt = lambda t: f"{t[0]:9.3f} ms ({t[1]:.3f}, {t[2]:.3f})"
say(f"Embedding maps timing: one MI355X, build {hip.version().split()[-1]} (xvec_version()), `python profiles/diag/tsne_timing.py`.")
say(f"Planted speakers (40 x N / 40 points, D = {DIM}, fp32); device time per call from hipEvents, {ROUNDS} rounds with the library")
say("and the torch baseline interleaved, medians (min, max).  Rates of the pair pass: its P bytes (N^2 x 8) against the 8.0 TB/s")
say(f"HBM figure, and {PAIR_OPS} fp64 operations a pair against the 78.6 TFLOP/s fp64 vector figure.")
for n in (1200, 4874):
    x, labels = planted(n)
    xd = torch.from_numpy(x).to(dev)
    say()
    say(f"N = {n}: plan (rows of a block, slices, columns of a slice) = {visualize.tsne_plan(n)}")
    d2 = visualize.squared_distances(xd)
    t_d, t_a, t_p = interleaved([lambda: visualize.squared_distances(xd, out=d2), lambda: visualize.tsne_affinities(sqdist=d2),
                                 lambda: visualize.pca_map(xd)], 3)
    say(f"  squared distances {fmt(t_d)}   affinities from them {fmt(t_a)}   pca_map {fmt(t_p)}")
    t = visualize.Tsne(xd, init="random", seed=0)
    t.step(100)
    lr = t.learning_rate_
    Yb, ub, gb = t.Y.clone(), t.update.clone(), t.gains.clone()
    fns = [lambda: t.step(1, 12.0, 0.5), lambda: t.step(1, 12.0, 0.5, report=True)]
    if n <= 1200:                                                      # the [N, N, 2] temporaries of the torch form
        fns.append(lambda: torch_iteration(t.P, Yb, ub, gb, 12.0, 0.5, lr))
    res = interleaved(fns, 20)
    say(f"  one iteration (pair pass + update) {fmt(res[0])}   with the KL value read back {fmt(res[1])}"
        + (f"   torch ops {fmt(res[2])} = {res[2][0] / res[0][0]:.1f} x" if len(res) > 2 else "   torch ops: not run (temporaries of N^2 x 2 doubles, several of them)"))
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(20):
                t.step(1, 12.0, 0.5, report=True)
            torch.cuda.synchronize()
        for e in sorted(prof.key_averages(), key=lambda e: e.key):
            if "tsne_" in e.key:
                us = getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / max(e.count, 1)
                name = e.key.split("tsne_")[1].split("(")[0].split("<")[0]
                extra = ""
                if name.startswith("pair_kernel") and us > 0:
                    extra = (f"   P at {n * n * 8 / (us * 1e-6) / 1e12:.2f} TB/s = {100 * n * n * 8 / (us * 1e-6) / HBM:.0f} % of HBM, "
                             f"{100 * PAIR_OPS * n * n / (us * 1e-6) / F64_VECTOR:.0f} % of the fp64 vector figure")
                say(f"    tsne_{name:<20s} {us:9.1f} us a launch ({e.count} launches){extra}")
    except Exception as e:      # noqa: BLE001
        say(f"    split by kernel: torch.profiler not usable here ({type(e).__name__}: {e})")
    runs = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tt = visualize.Tsne(xd, init="random", seed=0)
        tt.run()
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    y = tt.embedding_.cpu().numpy()
    sub = np.arange(0, n, max(1, n // 1200))
    say(f"  Tsne(x).run(), distances and affinities included, wall clock: {np.median(runs):.3f} s (of 3: {min(runs):.3f} .. {max(runs):.3f}); "
        f"n_iter_ {tt.n_iter_}, KL {tt.kl_divergence_:.4f}, 1-NN label accuracy {tsne_ref.nn_accuracy(y, labels):.4f}, "
        f"trustworthiness(5) on {sub.size} points {tsne_ref.trustworthiness(x[sub], y[sub], 5):.4f}")
    try:
        from sklearn.manifold import TSNE
        for method in (("exact", "barnes_hut") if n <= 1200 else ("barnes_hut",)):
            t0 = time.perf_counter()
            sk = TSNE(2, method=method, init="random", random_state=0, n_jobs=16)
            ysk = sk.fit_transform(x)
            say(f"  scikit-learn TSNE(method={method!r}) on the host: {time.perf_counter() - t0:.1f} s; KL {sk.kl_divergence_:.4f}, "
                f"1-NN label accuracy {tsne_ref.nn_accuracy(ysk, labels):.4f}")
        if n > 1200:
            say("  scikit-learn TSNE(method='exact'): not run at this size (minutes)")
    except ImportError:
        say("  scikit-learn is not installed on this box: no host baseline")
    del t, tt, d2
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
