"""Timing of VBx (xvector_amd.vbx): the Bayesian HMM over a batch of recordings' projected x-vectors, from an AHC-like noisy
initial assignment, D = 128, S = 10, 20 iterations, epsilon = -inf.  Shapes: 64 recordings x 37 windows (the workload of
profiles/segments_timing.txt), 8 x 512, 1 x 2048, 1 x 16384.  One box; device time from hipEvents, 7 rounds with the variants
interleaved, medians.  Two baselines: (a) what a user does without the kernel -- the same device tensors copied to pinned host
memory and the scaled fp64 form of tests/vbx_ref.py per recording on one thread, wall time with the copy included; (b) the scaled
recurrences written in torch ops on the same device.  Both baselines run BASE_ITERS iterations and are compared per iteration
(their cost per iteration does not depend on the count).  The recurrence's time per frame-step is taken by difference between
the two single recordings, the share of the two matrix products by difference between D = 128 and D = 8.  Last the whole chain,
Diarizer.diarize on 64 x 3000 frames with and without `resegment`.
Writes profiles-style text to the path given as the first argument (default: standard output only)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import vbx_ref
import xvector_amd as xa
from xvector_amd import diarize, hip, vbx as vbx_mod
from xvector_amd.scoring import PldaScorer

dev = "cuda:0"
D, S, K, ITERS, BASE_ITERS, ROUNDS, BASE_ROUNDS = 128, 10, 4, 20, 2, 7, 3
SHAPES = [(64, 37), (8, 512), (1, 2048), (1, 16384)]
OPTS = dict(loop_prob=0.99, Fa=0.3, Fb=17.0)
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


def data(n_rec, n, dim, seed):
    rs = np.arange(n_rec + 1, dtype=np.int64) * n
    phi = vbx_ref.planted(4, dim, 1, seed)[1]
    parts = [vbx_ref.planted(n, dim, K, seed + r, sep=1.5) for r in range(n_rec)]
    X = np.concatenate([p[0] for p in parts])
    lab = np.concatenate([vbx_ref.noisy_labels(p[2], S, seed + r) for r, p in enumerate(parts)])
    return rs, X, phi, lab


def torch_scaled(x, phi, gamma, pi, rs, iters):
    """The scaled form in torch ops, recording by recording (float64, on the device)."""
    lp, Fa, Fb = OPTS["loop_prob"], OPTS["Fa"], OPTS["Fb"]
    for a, b in zip(rs[:-1], rs[1:]):
        X, g, p = x[a:b], gamma[a:b].clone(), pi.clone()
        T = X.shape[0]
        G = -0.5 * ((X * X).sum(1, keepdim=True) + X.shape[1] * np.log(2 * np.pi))
        rho = X * phi.sqrt()
        for _ in range(iters):
            invL = 1.0 / (1 + Fa / Fb * g.sum(0, keepdim=True).T * phi)
            alpha = Fa / Fb * invL * (g.T @ rho)
            logp = Fa * (rho @ alpha.T - 0.5 * ((invL + alpha * alpha) @ phi) + G)
            bm = torch.exp(logp - logp.max(1, keepdim=True).values)
            q = (1 - lp) * p
            av = torch.empty_like(bm)
            c = torch.empty(T, dtype=torch.float64, device=x.device)
            v = p * bm[0]
            for t in range(T):
                if t:
                    v = (lp * av[t - 1] + q) * bm[t]
                c[t] = v.sum()
                av[t] = v / c[t]
            beta = torch.ones_like(p)
            arrive = torch.zeros_like(p)
            for t in range(T - 1, -1, -1):
                g[t] = av[t] * beta
                if t:
                    w = bm[t] * beta
                    arrive += q * w / c[t]
                    beta = (lp * w + (q * w).sum()) / c[t]
            p = g[0] + arrive
            p = p / p.sum()
    return g


fmt = lambda t: f"{t[0]:10.3f} ms ({t[1]:.3f}, {t[2]:.3f})"
say(f"VBx timing: one MI355X, build {hip.version().split()[-1]} (xvec_version()), `python profiles/diag/vbx_timing.py`.")
say(f"Planted speakers ({K} per recording, turns of 3 .. 11 windows), D = {D}, S = {S} states, a fifth of the initial labels redrawn,")
say(f"smoothing 5; loop_prob 0.99, Fa 0.3, Fb 17, {ITERS} iterations, epsilon = -inf.  Device time per call from hipEvents, {ROUNDS} rounds")
say(f"with the variants interleaved, medians (min, max).  host: X, gamma and pi copied to pinned host memory, then the scaled fp64 form")
say(f"of tests/vbx_ref.py per recording on one thread, wall time, copy included; torch: the same form in torch ops on the device.  Both")
say(f"baselines run {BASE_ITERS} iterations, {BASE_ROUNDS} rounds, and are compared PER ITERATION.  Every recording is one block of 256 threads, all of them")
say("resident at once; a frame-step is one dependent step of one of the two recurrences (2 T of them an iteration).")
single = {}
for n_rec, n in SHAPES:
    rs, X, phi, lab = data(n_rec, n, D, seed=n)
    N = n_rec * n
    xd, labd = torch.from_numpy(X).to(dev), torch.from_numpy(lab).to(dev)
    phid = torch.from_numpy(phi).to(dev)
    ws = torch.empty(vbx_mod.workspace_bytes(rs, D, S), dtype=torch.uint8, device=dev)
    g0, p0 = vbx_mod.vbx_init(labd, rs, S)
    ours = lambda: vbx_mod.vbx(xd, rs, phid, gamma=g0, pi=p0, max_iter=ITERS, epsilon=-np.inf, workspace=ws, **OPTS)
    one = lambda: vbx_mod.vbx(xd, rs, phid, gamma=g0, pi=p0, max_iter=1, epsilon=-np.inf, workspace=ws, **OPTS)
    px, pg, pp = (torch.empty(s, dtype=torch.float64).pin_memory() for s in ((N, D), (N, S), (n_rec, S)))

    def host():
        px.copy_(xd, non_blocking=True)
        pg.copy_(g0, non_blocking=True)
        pp.copy_(p0, non_blocking=True)
        torch.cuda.synchronize()
        hx, hg, hp = px.numpy(), pg.numpy(), pp.numpy()
        return [vbx_ref.vbx_scaled(hx[a:b], phi, hg[a:b], hp[r], max_iter=BASE_ITERS, epsilon=-np.inf, **OPTS)
                for r, (a, b) in enumerate(zip(rs[:-1], rs[1:]))]

    tch = lambda: torch_scaled(xd, phid, g0, p0[0], rs, BASE_ITERS)
    big = N > 4096
    t_o, t_1, t_h, t_t = interleaved([ours, one, host, tch], [once, once, wall, wall], [ROUNDS, ROUNDS, 1 if big else BASE_ROUNDS, 1 if big else BASE_ROUNDS])
    res = ours()
    same = all(np.array_equal(vbx_ref.labels_of(vbx_ref.vbx_scaled(X[a:b], phi, g0[a:b].cpu().numpy(), p0[r].cpu().numpy(), max_iter=ITERS,
                                                                   epsilon=-np.inf, **OPTS)[0])[0], res.labels[a:b].cpu().numpy())
               for r, (a, b) in enumerate(zip(rs[:2], rs[1:3])))
    per_it = (t_o[0] - t_1[0]) / (ITERS - 1)
    if n_rec == 1:
        single[n] = per_it
    say()
    say(f"{n_rec} recordings x {n} windows (workspace {ws.numel() / 2 ** 20:.1f} MiB; speakers found {int(res.n_speakers.min())} .. "
        f"{int(res.n_speakers.max())}; labels of the first recordings equal the reference's: {same})")
    say(f"  vbx, {ITERS} iterations {fmt(t_o)}   1 iteration {fmt(t_1)}   per further iteration {per_it:8.3f} ms = "
        f"{1e3 * per_it / (2 * n):6.3f} us per frame-step with everything else in it")
    say(f"  host, {BASE_ITERS} iterations  {fmt(t_h)}   per iteration {t_h[0] / BASE_ITERS:10.3f} ms   host / vbx per iteration {t_h[0] / BASE_ITERS / per_it:8.2f} x")
    say(f"  torch, {BASE_ITERS} iterations {fmt(t_t)}   per iteration {t_t[0] / BASE_ITERS:10.3f} ms   torch / vbx per iteration {t_t[0] / BASE_ITERS / per_it:8.2f} x")
    if n_rec == 1:                                   # the share of the two products: the same frames at D = 8
        rs8, X8, phi8, lab8 = data(n_rec, n, 8, seed=n)
        x8, ph8 = torch.from_numpy(X8).to(dev), torch.from_numpy(phi8).to(dev)
        g8, p8 = vbx_mod.vbx_init(torch.from_numpy(lab8).to(dev), rs8, S)
        f20 = lambda: vbx_mod.vbx(x8, rs8, ph8, gamma=g8, pi=p8, max_iter=ITERS, epsilon=-np.inf, **OPTS)
        f1 = lambda: vbx_mod.vbx(x8, rs8, ph8, gamma=g8, pi=p8, max_iter=1, epsilon=-np.inf, **OPTS)
        t20, t1 = interleaved([f20, f1], [once, once], [ROUNDS, ROUNDS])
        it8 = (t20[0] - t1[0]) / (ITERS - 1)
        say(f"  at D = 8: per iteration {it8:8.3f} ms, so the products' part that grows with D is {per_it - it8:8.3f} ms an iteration "
            f"({100 * (per_it - it8) / per_it:.0f} % of it at D = {D})")
    del xd, ws
if len(single) == 2:
    (na, ta), (nb, tb) = sorted(single.items())
    say()
    say(f"By difference between the single recordings of {na} and {nb} windows: {1e3 * (tb - ta) / (2 * (nb - na)):.3f} us per frame-step "
        "(both recurrences' steps, with the per-frame share of the products and the emissions).")

# the whole chain with and without the refinement
B, T, WIN, HOP, DIM, RANK = 64, 3000, 300, 75, 512, 200
model = xa.XVectorModel()
model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in xa.synth.make_state_dict(seed=42).items()})
model = model.to(dev).eval()
feats = torch.from_numpy(xa.synth.make_mfcc(B, T, seed=1)).to(dev)
mean, F, Sigma = xa.synth.make_plda(DIM, RANK, seed=21)
scorer = PldaScorer(mean, F, Sigma, device=dev)
vm = vbx_mod.VbxModel.from_plda(mean, F, Sigma)
plain = diarize.Diarizer(model, scorer, win=WIN, hop=HOP, threshold=0.0, device=dev)
refined = diarize.Diarizer(model, scorer, win=WIN, hop=HOP, threshold=0.0, device=dev, resegment=vbx_mod.Vbx(vm, n_speakers=S, max_iter=ITERS, epsilon=-np.inf))
t_p, t_r = interleaved([lambda: plain.diarize(feats), lambda: refined.diarize(feats)], [wall, wall], [ROUNDS, ROUNDS])
say()
say(f"The chain on {B} recordings x {T} frames, win {WIN}, hop {HOP} (fp32 model, PLDA rank {RANK}: VBx in {len(vm.phi)} dimensions, {S} states,")
say(f"{ITERS} iterations; wall time with the final copy of the labels and the turns on the host):")
say(f"  Diarizer.diarize                  {fmt(t_p)}")
say(f"  Diarizer.diarize, resegment=Vbx   {fmt(t_r)}   (+ {t_r[0] - t_p[0]:.3f} ms)")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
