"""Timing of energy VAD, sliding CMVN and the selection of voiced frames (xvector_amd.vad) at the bench batch (256 x 299 x 24)
and at the diarization workload (64 x 3000 x 24): the three calls and the fused one against the same work in torch ops on the
same device -- a mean and a conv1d vote for the decisions, cumulative sums for the window means, a stable-argsort gather for
the selection and the host length count -- and the chain waveform -> MFCC -> VadCmvn -> extract_x_vec in bf16 with and without
the new stage.  Device time from hipEvents around 5 calls, 7 rounds with the library and the torch baseline interleaved, medians
over the rounds, one box.  Writes profiles-style text to the path given as the first argument (default: standard output only)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import xvector_amd as xa
from xvector_amd import hip, vad
import vad_ref

dev = "cuda:0"
ROUNDS, CALLS, HBM = 7, 5, 8.0e12
VAD = dict(energy_threshold=5.5, energy_mean_scale=0.5, frames_context=2, proportion_threshold=0.12)
CMVN = dict(cmn_window=300, min_window=100, center=True, norm_vars=False)
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


fmt = lambda t: f"{1e3 * t[0]:8.1f} us ({1e3 * t[1]:.1f}, {1e3 * t[2]:.1f})"


def row(name, t_o, t_b, nbytes):
    rate = nbytes / (t_o[0] * 1e-3)
    say(f"  {name:<22} library {fmt(t_o)}   torch {fmt(t_b)}   torch / library {t_b[0] / t_o[0]:6.2f} x   "
        f"{nbytes / 1e6:6.2f} MB at {rate / 1e12:.3f} TB/s = {100 * rate / HBM:.1f} % of HBM")


class TorchBaseline:
    """The same work in torch ops for full-length utterances of T frames: what a user composes today."""

    def __init__(self, T):
        win = [vad_ref.window(t, T, CMVN["cmn_window"], CMVN["min_window"], CMVN["center"]) for t in range(T)]
        self.lo = torch.tensor([w[0] for w in win], device=dev)
        self.hi = torch.tensor([w[1] for w in win], device=dev)
        self.n = (self.hi - self.lo).double()[None, :, None]
        ctx = VAD["frames_context"]
        self.kernel = torch.ones(1, 1, 2 * ctx + 1, dtype=torch.float64, device=dev)
        self.den = torch.nn.functional.conv1d(torch.ones(1, 1, T, dtype=torch.float64, device=dev), self.kernel, padding=ctx)[0]
        self.ctx, self.rank = ctx, torch.arange(T, device=dev)[None, :]

    def decide(self, x):
        e = x[:, :, 0].double()
        thr = VAD["energy_threshold"] + VAD["energy_mean_scale"] * e.mean(1)
        hot = (e > thr[:, None]).double()
        num = torch.nn.functional.conv1d(hot[:, None, :], self.kernel, padding=self.ctx)[:, 0]
        mask = num >= self.den * VAD["proportion_threshold"]
        return mask, mask.sum(1)

    def normalise(self, x):
        c = torch.nn.functional.pad(torch.cumsum(x.double(), 1), (0, 0, 1, 0))
        return (x.double() - (c[:, self.hi] - c[:, self.lo]) / self.n).float()

    def select(self, y, mask, counts):
        order = torch.argsort((~mask).to(torch.uint8), dim=1, stable=True)
        out = torch.gather(y, 1, order[:, :, None].expand(-1, -1, y.shape[2]))
        return out * (self.rank < counts[:, None])[:, :, None], counts.tolist()          # the host length count

    def fused(self, x):
        mask, counts = self.decide(x)
        return self.select(self.normalise(x), mask, counts)


say(f"VAD and sliding-CMVN timing: one MI355X, build {hip.version().split()[-1]} (xvec_version()), `python profiles/diag/vad_timing.py`.")
say(f"fp32 features, energies N(10, 3), every utterance of full length; the recipe's settings (VAD {VAD}, CMVN {CMVN}).")
say(f"Device time per call from hipEvents around {CALLS} calls, {ROUNDS} rounds with the library and the torch baseline interleaved,")
say("medians (min, max).  Bytes: what the step must move (the features read and written once, the energies, the mask), against")
say("the 8.0 TB/s HBM figure.  Both sides allocate their outputs in the call; the fused call and select's baseline end in the host")
say("read of the new lengths.")
for B, T, C in ((256, 299, 24), (64, 3000, 24)):
    say()
    say(f"{B} x {T} x {C} ({B * T * C * 4 / 1e6:.2f} MB of features)")
    rng = np.random.default_rng(B)
    host = rng.standard_normal((B, T, C)).astype(np.float32)
    host[:, :, 0] = rng.normal(10.0, 3.0, (B, T)).astype(np.float32)
    x = torch.from_numpy(host).to(dev)
    base = TorchBaseline(T)
    v = vad.energy_vad(x, **VAD)
    y = vad.sliding_cmvn(x, **CMVN)
    prep = vad.VadCmvn(vad=VAD, **CMVN)
    feats = B * T * C * 4
    t = interleaved([lambda: vad.energy_vad(x, **VAD), lambda: base.decide(x),
                     lambda: vad.sliding_cmvn(x, **CMVN), lambda: base.normalise(x),
                     lambda: vad.select_voiced(y, v.mask), lambda: base.select(y, v.mask.bool(), v.counts),
                     lambda: prep(x), lambda: base.fused(x)])
    row("energy_vad", t[0], t[1], B * T * 5)
    row("sliding_cmvn", t[2], t[3], 2 * feats)
    row("select_voiced", t[4], t[5], 2 * feats + B * T)
    row("VadCmvn (fused)", t[6], t[7], 2 * feats + B * T * 6)
    # what the two sides computed: the same decisions, the same rows to fp32 rounding
    bm, bc = base.decide(x)
    p, (by, bl) = prep(x), base.fused(x)
    say(f"  decisions equal torch's: {bool(torch.equal(bm, v.mask.bool()))}; voiced {100 * float(v.mask.float().mean()):.0f} % of the frames; "
        f"lengths equal: {p.lengths == bl}; largest difference of the prepared rows {float((p.feats - by).abs().max()):.1e}")
    del x, y, v

say()
say("the chain at the bench batch: 256 waveforms of 3 s at 16 kHz -> MfccFrontEnd -> (VadCmvn) -> extract_x_vec, bf16 model")
sd = {k: torch.from_numpy(np.asarray(v)) for k, v in xa.synth.make_state_dict(seed=42).items()}
model = xa.XVectorModel(precision="bf16")
model.load_state_dict(sd)
model = model.to(dev).eval()
fe = xa.MfccFrontEnd(device=dev)
rng = np.random.default_rng(1)
wav = rng.standard_normal((256, 48000)).astype(np.float32)
wav *= np.repeat(np.where(rng.random((256, 30)) < 0.3, 0.01, 1.0), 1600, axis=1).astype(np.float32)       # 0.1 s stretches, 30 % quiet
waves = torch.from_numpy(wav * 3000).to(dev)
prep = vad.VadCmvn()


def plain():
    model.extract_x_vec(fe(waves))


def with_stage():
    p = prep(fe(waves))
    model.extract_x_vec(p.feats, p.lengths)


t_plain, t_stage, t_fe = interleaved([plain, with_stage, lambda: fe(waves)])
p = prep(fe(waves))
say(f"  MFCC -> extract_x_vec                 {fmt(t_plain)}")
say(f"  MFCC -> VadCmvn -> extract_x_vec      {fmt(t_stage)}   {t_stage[0] / t_plain[0]:.2f} x the plain chain")
say(f"  of it the MFCC front end              {fmt(t_fe)}")
say(f"  frames kept: {sum(p.lengths)} of {p.feats.shape[0] * p.feats.shape[1]} ({min(p.lengths)} .. {max(p.lengths)} per utterance)")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
