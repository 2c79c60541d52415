"""Timing of resampling (xvector_amd.resample) at the bench's batch: 256 rows x 3 s of OUTPUT at 16 kHz, from 48 kHz, 44.1 kHz,
8 kHz and 16 kHz, both accumulate modes, and speed perturbation at 0.9 / 1.0 / 1.1.  Device time from hipEvents, 7 rounds with
the library and the torch baseline interleaved, medians over the rounds, one box.  The torch baseline is the same arithmetic in
torch ops on the same device (index tensors, a gather of the table and of the samples, a sum over the tap axis in chunks of
rows); the CPU figure is the vectorised numpy restatement (tests/resample_ref.py) of ONE row on one thread, times 256.  A second
table with eight entries per zero crossing (precision 3: 513 entries, 4 KiB, every read a cache hit next to its neighbours')
separates the cost of the table gathers from the rest, per tap (its wings have a different number of taps).  Writes
profiles-style text to the path given as the first argument (default: standard output only)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import resample_ref as ref
from xvector_amd import hip, resample as rs

dev = "cuda:0"
B, N_OUT, ROUNDS, CALLS = 256, 48000, 7, 3
FP64_FMA_PEAK = 78.6e12           # vendor figure, fp64 vector, counting a fused multiply-add as two
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
        for t, fn, c in zip(ts, fns, calls):
            t.append(once(fn, c))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


def torch_resample(x, ratio, win_d, precision, rows_per_chunk=8):
    """The restatement in torch ops, fp64 running sum (a sum over the tap axis, not the package's order)."""
    n, nwin, P = x.shape[1], win_d.shape[0], 2 ** precision
    inc, scale, step = ref.ratio_plan(ratio, precision)
    win_s = win_d * ratio if ratio < 1 else win_d
    delta = torch.cat([win_s[1:] - win_s[:-1], win_s.new_zeros(1)])
    n_out = int(n * ratio)
    time_ = torch.arange(n_out, dtype=torch.float64, device=x.device) * inc
    n0 = time_.long()
    frac = scale * (time_ - n0)
    out = torch.zeros((x.shape[0], n_out), dtype=torch.float64, device=x.device)
    xd = x.double()
    taps = torch.arange(nwin // step + 1, device=x.device)
    for wing in (0, 1):
        if wing:
            frac = scale - frac
        idx = frac * P
        off = idx.long()
        eta = idx - off
        count = torch.minimum(n - n0 - 1 if wing else n0 + 1, (nwin - off) // step)
        j = (off[:, None] + taps[None, :] * step).clamp_(max=nwin - 1)
        live = taps[None, :] < count[:, None]
        w = torch.where(live, win_s[j] + eta[:, None] * delta[j], 0.0)
        src = ((n0[:, None] + taps[None, :] + 1) if wing else (n0[:, None] - taps[None, :])).clamp_(0, n - 1)
        for r0 in range(0, x.shape[0], rows_per_chunk):
            out[r0:r0 + rows_per_chunk] += (xd[r0:r0 + rows_per_chunk][:, src] * w[None]).sum(-1)
    return out


fmt = lambda t: f"{t[0]:9.3f} ms ({t[1]:.3f}, {t[2]:.3f})"
say(f"Resampling timing: one MI355X, build {hip.version().split()[-1]} (xvec_version()), `python profiles/diag/resample_timing.py`.")
say(f"{B} rows x {N_OUT} outputs (3 s at 16 kHz), int16 PCM in, float32 out, filter kaiser_best; device time per call from hipEvents")
say(f"around {CALLS} calls (1 for torch), {ROUNDS} rounds with the library and the torch baseline interleaved, medians (min, max).")
say("fp64 operations: 7 per tap when downsampling (two table entries scaled, their difference, the weight, the update), 5 otherwise,")
say(f"none of them fused; rate against the vendor's {FP64_FMA_PEAK / 1e12:.1f} TFLOP/s fp64 vector figure (which counts a fused multiply-add as")
say("two: separate multiplies and adds can reach half of it).")
say()
best, precision = rs._table("kaiser_best")
win_d = torch.from_numpy(best).to(dev)
coarse = (ref.sinc_window(num_zeros=64, precision=3), 3)              # 513 entries: the table reads of a wave hit a few lines
coarse_d = torch.from_numpy(coarse[0]).to(dev)
rng = np.random.default_rng(0)
for sr in (48000, 44100, 8000, 16000):
    ratio = 16000 / sr
    n = next(n for n in range(int(N_OUT / ratio) - 2, int(N_OUT / ratio) + 4) if ref.num_out(n, ratio) == N_OUT)
    pcm = rng.integers(-32768, 32768, size=(B, n), dtype=np.int64).astype(np.int16)
    x = torch.from_numpy(pcm).to(dev)
    inc, scale, step = ref.ratio_plan(ratio, precision)
    taps = 2 * (best.shape[0] // step)
    flop = B * N_OUT * taps * (7 if ratio < 1 else 5)
    out = torch.empty((B, N_OUT), dtype=torch.float32, device=dev)
    ws = torch.empty(int(hip.lib.xvec_resample_workspace_bytes(B, 1)), dtype=torch.uint8, device=dev)
    f32 = lambda: rs.resample_rows(x, [ratio], None, "kaiser_best", "float32", torch.float32, out, ws, win_d)
    f64 = lambda: rs.resample_rows(x, [ratio], None, "kaiser_best", "float64", torch.float32, out, ws, win_d)
    c64 = lambda: rs.resample_rows(x, [ratio], None, coarse, "float64", torch.float32, out, ws, coarse_d)
    base = lambda: torch_resample(x, ratio, win_d, precision)
    t32, t64, tc, tb = interleaved([f32, f64, c64, base], [CALLS, CALLS, CALLS, 1])
    got = rs.resample_rows(x, [ratio], None, "kaiser_best", "float64", torch.float64)[0]
    diff = float((got - base()).abs().max() / got.abs().max())
    t0 = time.perf_counter()
    ref.resample_row(pcm[0], ratio, best, precision, "float32")
    cpu = (time.perf_counter() - t0) * B
    say(f"{sr:6d} Hz -> 16 kHz ({n} samples a row, {taps} taps an output, table step {step}, tile span {rs.tile_span(ratio)}):")
    say(f"  library, float32 sum {fmt(t32)}   float64 sum {fmt(t64)}   {flop / (t64[0] * 1e-3) / 1e12:5.2f} Tflop/s = "
        f"{100 * flop / (t64[0] * 1e-3) / FP64_FMA_PEAK:4.1f} % of the fp64 vector figure")
    ctaps = 2 * (coarse[0].shape[0] // ref.ratio_plan(ratio, 3)[2])
    say(f"  the same launch on a 513-entry table (precision 3, {ctaps} taps), float64 sum {fmt(tc)}: per tap {t64[0] / taps / (tc[0] / ctaps):.2f} x "
        f"faster without the gathers' spread")
    say(f"  torch ops, float64 {fmt(tb)} = {tb[0] / t64[0]:7.1f} x the library (largest difference to it {diff:.1e} of the peak)")
    say(f"  numpy restatement, one thread: {cpu:8.1f} s for the batch = {cpu * 1e3 / t32[0]:9.0f} x the library")
    del x, out
say()
factors = np.tile([0.9, 1.0, 1.1], B // 3 + 1)[:B]
pcm = rng.integers(-32768, 32768, size=(B, N_OUT), dtype=np.int64).astype(np.int16)
x = torch.from_numpy(pcm).to(dev)
sp32 = lambda: rs.speed_perturb(x, factors)
sp64 = lambda: rs.speed_perturb(x, factors, accumulate="float64")
t32, t64 = interleaved([sp32, sp64], [CALLS, CALLS])
say(f"speed_perturb, {B} rows x {N_OUT} samples, factors 0.9 / 1.0 / 1.1 in turn (one launch, output allocated inside the call):")
say(f"  float32 sum {fmt(t32)}   float64 sum {fmt(t64)}")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
