"""Timing of the waveform augmentation (xvector_amd.augment) at the bench batch: 256 utterances of 48 000 samples, a pool of
64 int16 clips, impulse responses of 4000 and of 16 000 taps.  Device time per library call (hipEvents around the call alone;
a preroll of the reverb kernel to bring the clocks up, three warm calls, the median of the timed ones), the reverb
kernel's rate against the 157.3 TFLOP/s fp32 MFMA peak (2 (n + L - 1) L flop per utterance: the outputs that exist, not the
padded tiles), and the same work in tests/augment_ref.py on a pool of 16 host threads (FFT convolution there, as the
reference).  Mix uses the reference's kind proportions (one fifth each of none, music, speech, noise, rir); reverb is timed
with every row reverberated.  Run it as one time-limited step:  timeout -k 10 600 python profiles/diag/augment_timing.py"""
import os, random, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import xvector_amd as xa
from xvector_amd import hip
import augment_ref as ar

dev = "cuda:0"
B, n, R, m_max, THREADS, PEAK = 256, 48000, 64, 160000, 16, 157.3
rng = np.random.default_rng(0)
pool = (rng.standard_normal((R, m_max)) * 3000).astype(np.int16)
pool_len = rng.integers(16000, m_max + 1, R)
x = (rng.standard_normal((B, n)) * 5000).astype(np.int16).astype(np.float32)
xd = torch.from_numpy(x).to(dev)
kinds = [xa.augment.KINDS[i % 5] for i in range(B)]
print(f"build {hip.version()}; B = {B}, n = {n}, pool {R} x {m_max} int16, host threads {THREADS}")


def ev_time(fn, reps=10):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def host(fn, rows):
    t0 = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as ex:
        list(ex.map(fn, rows))
    return (time.perf_counter() - t0) * 1e3


fmt = lambda t: f"{t[0]:.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"
for L in (4000, 16000):
    rirs = (rng.standard_normal((8, L)) * np.exp(-np.arange(L) / (L / 6.0))).astype(np.float32)
    aug = xa.WaveAugmenter(pool, pool_len, rirs, [L] * 8, device=dev)
    plan = xa.AugmentPlan.draw(kinds, n, range(0, 24), range(24, 48), range(48, 64), 8, rng=random.Random(0), pool_len=pool_len)
    all_rir = torch.from_numpy(np.arange(B, dtype=np.int32) % 8).to(dev)
    work = xd.clone()
    for _ in range(5): aug.reverb(work, all_rir, inplace=True)                 # preroll; the values do not matter for the time
    work.copy_(xd)
    t_mix = ev_time(lambda: aug.mix(work, plan, inplace=True))
    work.copy_(xd)
    t_rev = ev_time(lambda: aug.reverb(work, all_rir, inplace=True))           # repeated reverb keeps max|x|: values stay finite
    work.copy_(xd)
    t_norm = ev_time(lambda: aug.normalize(work, inplace=True))
    flop = 2.0 * (n + L - 1) * L * B
    tf = flop / (t_rev[0] * 1e-3) / 1e12
    print(f"L = {L}: mix ({len(plan.ops)} ops) {fmt(t_mix)}; reverb, all rows {fmt(t_rev)} = {tf:.1f} TFLOP/s = "
          f"{100 * tf / PEAK:.1f} % of {PEAK}; normalize {fmt(t_norm)}")
    h_rev = host(lambda b: ar.reverb_row(x[b], rirs[b % 8], fft=True), range(B))
    print(f"L = {L}: host reverb (augment_ref, FFT, {THREADS} threads) {h_rev:.1f} ms")
h_mix = host(lambda u: ar.mix(x[u:u + 1], pool, pool_len, [dict(zip(o.dtype.names, o), utt=0) for o in plan.ops[plan.ops["utt"] == u]],
                              plan.srcs), range(B))
h_norm = host(lambda b: ar.normalize(x[b]), range(B))
print(f"host mix (augment_ref, {THREADS} threads) {h_mix:.1f} ms; host normalize {h_norm:.1f} ms")
