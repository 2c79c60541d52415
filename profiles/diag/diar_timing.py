"""Timing of diarization's clustering (xvector_amd.diarize): average-linkage clustering of the window scores of a batch of
recordings, alone and behind the PLDA scorer, on planted-speaker x-vectors drawn from the PLDA model itself (4 speakers per
recording in turns of 1 .. 8 windows), stopped by the threshold 0.  Shapes: 64 recordings x 37 windows (the workload of
profiles/segments_timing.txt: 3000 frames, win 300, hop 75), 8 x 512, 1 x 2048.  One box; device time from hipEvents around 5
calls, 7 rounds with the variants interleaved, medians.  The baseline is what a user does without the kernel: the same device
matrix copied to pinned host memory, then scipy's linkage(method='average') and fcluster per recording on one thread, wall
time with the copy included.  Last the whole chain, Diarizer.diarize on 64 x 3000 frames beside extract_windows alone.
Writes profiles-style text to the path given as the first argument (default: standard output only)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from scipy.cluster import hierarchy
import xvector_amd as xa
from xvector_amd import diarize, hip
from xvector_amd.scoring import PldaScorer

dev = "cuda:0"
DIM, RANK, SPEAKERS, ROUNDS, CALLS, THR = 512, 200, 4, 7, 5, 0.0
SHAPES = [(64, 37), (8, 512), (1, 2048)]
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


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def interleaved(fns, timers):
    """Median, min and max over ROUNDS of every function's time (ms), one after the other in each round."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(ROUNDS):
        for t, fn, timer in zip(ts, fns, timers):
            t.append(timer(fn))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


def planted(n_rec, n, mean, F, chol, seed):
    """[n_rec n, DIM] x-vectors: per recording SPEAKERS speakers y ~ N(0, I), mean + F y + noise of covariance Sigma."""
    rng = np.random.default_rng(seed)
    out = np.empty((n_rec * n, DIM))
    for r in range(n_rec):
        centres = mean + rng.standard_normal((SPEAKERS, RANK)) @ F.T
        who, k, s = np.zeros(n, dtype=np.int64), 0, 0
        while k < n:
            run = int(rng.integers(1, 9))
            who[k:k + run] = s
            k += run
            s = int(rng.integers(0, SPEAKERS))
        out[r * n:(r + 1) * n] = centres[who] + rng.standard_normal((n, DIM)) @ chol.T
    return out


def scipy_labels(block):
    n = block.shape[0]
    if n == 1:
        return np.ones(1, dtype=np.int32)
    Z = hierarchy.linkage(-block[np.triu_indices(n, 1)], "average")
    shift = Z[:, 2].min()
    Z[:, 2] -= shift
    return hierarchy.fcluster(Z, t=-THR - shift, criterion="distance")


fmt = lambda t: f"{t[0]:9.3f} ms ({t[1]:.3f}, {t[2]:.3f})"
say(f"Diarization clustering timing: one MI355X, build {hip.version().split()[-1]} (xvec_version()), `python profiles/diag/diar_timing.py`.")
say(f"Planted-speaker x-vectors ({SPEAKERS} speakers per recording, dim {DIM}) drawn from a rank-{RANK} PLDA model and scored by it; stop at")
say(f"threshold {THR}.  Device time per call from hipEvents around {CALLS} calls, {ROUNDS} rounds with the variants interleaved, medians (min,")
say("max).  scipy: the device matrix copied to pinned host memory, then linkage('average') + fcluster per recording on one thread,")
say("wall time, copy included.  A recording's merges are dependent steps: `per step` is the cluster time over the most merges any")
say("recording of the batch performed; every recording is one block, all of them resident at once (256 CUs).")
mean, F, Sigma = xa.synth.make_plda(DIM, RANK, seed=21)
chol = np.linalg.cholesky(Sigma)
scorer = PldaScorer(mean, F, Sigma, device=dev)
for n_rec, n in SHAPES:
    N = n_rec * n
    x = torch.from_numpy(planted(n_rec, n, mean, F, chol, seed=n)).to(dev)
    rs = np.arange(n_rec + 1, dtype=np.int64) * n
    S = scorer.score(x)
    ws = torch.empty(int(hip.lib.xvec_ahc_workspace_bytes(rs.ctypes.data_as(hip.C.POINTER(hip.C.c_int64)), n_rec)), dtype=torch.uint8,
                     device=dev)
    pinned = torch.empty((N, N), dtype=torch.float64).pin_memory()
    ours = lambda: diarize.cluster(S, rs, threshold=THR, workspace=ws)
    both = lambda: diarize.cluster(scorer.score(x), rs, threshold=THR, workspace=ws)

    def base():
        pinned.copy_(S, non_blocking=True)
        torch.cuda.synchronize()
        h = pinned.numpy()
        return [scipy_labels(h[a:b, a:b]) for a, b in zip(rs[:-1], rs[1:])]

    def copy_only():
        pinned.copy_(S, non_blocking=True)
        torch.cuda.synchronize()

    t_c, t_b, t_s, t_copy = interleaved([ours, both, base, copy_only], [once, once, wall, wall])
    cl = diarize.cluster(S, rs, threshold=THR, return_merges=True)
    merges = (cl.merges[0].view(n_rec, n) >= 0).sum(dim=1)
    counts = cl.n_clusters.cpu().numpy()
    same = all(len(set(l.tolist())) == c for l, c in zip(base(), counts))
    steps = max(1, int(merges.max()))
    say()
    say(f"{n_rec} recordings x {n} windows ({N} x {N} scores; workspace {ws.numel() / 2 ** 20:.1f} MiB; clusters per recording "
        f"{int(counts.min())} .. {int(counts.max())}, as many as scipy finds: {same})")
    say(f"  cluster          {fmt(t_c)}   {1e3 * t_c[0] / steps:7.2f} us per step ({steps} dependent steps, {n_rec} recordings in flight)")
    say(f"  score + cluster  {fmt(t_b)}")
    say(f"  scipy            {fmt(t_s)}   of which the copy {fmt(t_copy)}   scipy / cluster {t_s[0] / t_c[0]:7.2f} x")
    del x, S, ws, pinned

# the whole chain beside extract_windows alone
B, T, WIN, HOP = 64, 3000, 300, 75
model = xa.XVectorModel()
model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in xa.synth.make_state_dict(seed=42).items()})
model = model.to(dev).eval()
feats = torch.from_numpy(xa.synth.make_mfcc(B, T, seed=1)).to(dev)
scorer = PldaScorer(*xa.synth.make_plda(DIM, RANK, seed=21), device=dev)
d = diarize.Diarizer(model, scorer, win=WIN, hop=HOP, threshold=THR, device=dev)
t_w, t_d = interleaved([lambda: model.extract_windows(feats, WIN, HOP), lambda: d.diarize(feats)], [wall, wall])
res = d.diarize(feats)
say()
say(f"The chain on {B} recordings x {T} frames, win {WIN}, hop {HOP} ({len(res.windows)} windows, fp32 model, wall time with the final copy")
say("of the labels and the turns on the host):")
say(f"  extract_windows  {fmt(t_w)}")
say(f"  Diarizer.diarize {fmt(t_d)}   (+ {t_d[0] - t_w[0]:.3f} ms for scoring, clustering, the labels' copy and turns())")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
