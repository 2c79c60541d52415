"""Timing of x-vectors over sliding windows (XVectorModel.extract_windows, xvec_forward_segments), one box, hipEvents, warm-up,
interleaved rounds, medians.

Workload: 64 recordings of 3000 frames, win = 300, hop = 75 / 150 / 300 (no overlap: the break-even case), fp32 / bf16x3 / bf16.
  new        extract_windows: the frame-level stack once over the recordings, every window pools its rows
  gathered   the existing extract_x_vec on the same windows gathered into a [n_windows, 300, 24] batch (the only way before;
             that path is untouched, so it is the parent commit's), timed with and without the gather
and the per-stage split of both (xvec_get_timings).  Then the segment-pooling kernel alone through xvec_stat_pool_segments on
the same row ranges of a [64 * 2986, 1536] matrix, with its bytes per second over its algorithmic bytes: every segment's rows
read once ("segment bytes"), and every distinct row read once ("distinct bytes") -- the gap is what the re-reads of
overlapping windows cost and what an XCD-aware segment order could at most win back.
Run it as one time-limited step:
    timeout -k 10 900 python profiles/diag/segments_timing.py [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import xvector_amd as xa
from xvector_amd import hip
from xvector_amd._device import stream

DEV, ROUNDS = "cuda:0", 7
B, T, WIN, HOPS = 64, 3000, 300, (75, 150, 300)
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)            # ms


def medians(fns, warm=2):
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    return np.median(np.array([[timed(f) for f in fns] for _ in range(ROUNDS)]), 0)


def stages(m, fn):
    m.set_profiling(True)
    fn()
    t = m.timings_ms()
    m.set_profiling(False)
    return " ".join(f"{k}={v:.3f}" for k, v in t.items() if v > 0)


def whole_path(sd, x):
    say(f"\n== 1. {B} recordings x {T} frames, win {WIN}: extract_windows against extract_x_vec on the gathered windows (ms)")
    say(f"{'precision':<8}{'hop':>5}{'windows':>9}{'new':>9}{'gathered':>10}{'no gather':>11}{'new/gathered':>14}")
    split = []
    for prec in ("fp32", "bf16x3", "bf16"):
        m = xa.XVectorModel(precision=prec)
        m.load_state_dict(sd)
        m = m.to(DEV).eval()
        for hop in HOPS:
            w = xa.sliding_windows([T] * B, WIN, hop)
            wt = torch.from_numpy(w.astype(np.int64)).to(DEV)
            rows = (wt[:, 0] * T + wt[:, 1])[:, None] + torch.arange(WIN, device=DEV)[None]
            gather = lambda: x.reshape(-1, x.shape[-1])[rows]
            batch = gather()
            new, gat, nog = medians([lambda: m.extract_segments(x, w), lambda: m.extract_x_vec(gather()),
                                     lambda: m.extract_x_vec(batch)])
            say(f"{prec:<8}{hop:>5}{len(w):>9}{new:>9.3f}{gat:>10.3f}{nog:>11.3f}{new / gat:>14.3f}")
            if hop == 75:
                split.append(f"{prec} hop 75 new:      " + stages(m, lambda: m.extract_segments(x, w)))
                split.append(f"{prec} hop 75 gathered: " + stages(m, lambda: m.extract_x_vec(batch)))
            del batch, rows
            torch.cuda.empty_cache()
        del m
        torch.cuda.empty_cache()
    say("\nper-stage split (xvec_get_timings; new: tdnn5_pool = layer 5 writing rows, pool_finalize = segment rows + segment pooling)")
    for line in split:
        say(line)


def pooling_kernel():
    rows, C, ldy = B * (T - 14), 1500, 1536
    say(f"\n== 2. the segment-pooling kernel alone: [{rows}, {ldy}] rows, {C} channels, segments of {WIN - 14} rows")
    say(f"{'rows':<6}{'hop':>5}{'segments':>10}{'ms':>9}{'segment GB/s':>14}{'distinct GB/s':>15}{'re-read factor':>16}")
    g = torch.Generator(device=DEV).manual_seed(1)
    for dtype, es in ((torch.float32, 4), (torch.bfloat16, 2)):
        y = torch.randn(rows, ldy, device=DEV, generator=g).to(dtype)
        for hop in HOPS:
            w = xa.sliding_windows([T] * B, WIN, hop).astype(np.int64)
            r0 = torch.from_numpy(w[:, 0] * (T - 14) + w[:, 1]).to(DEV)
            n = torch.from_numpy((w[:, 2] - 14).astype(np.int32)).to(DEV)
            out = torch.empty(len(w), 2 * C, device=DEV)

            def run():
                hip.check(hip.lib.xvec_stat_pool_segments(y.data_ptr(), int(es == 2), rows, ldy, C, r0.data_ptr(), n.data_ptr(),
                                                          len(w), None, None, out.data_ptr(), stream(DEV)))
            ms = medians([run])[0]
            covered = np.zeros(rows, dtype=bool)
            for a, k in zip(r0.cpu().numpy(), n.cpu().numpy()):
                covered[a:a + k] = True
            seg_b = float((w[:, 2] - 14).sum()) * C * es + out.numel() * 4
            dis_b = float(covered.sum()) * C * es + out.numel() * 4
            say(f"{'fp32' if es == 4 else 'bf16':<6}{hop:>5}{len(w):>10}{ms:>9.3f}{seg_b / ms / 1e6:>14.1f}{dis_b / ms / 1e6:>15.1f}"
                f"{seg_b / dis_b:>16.2f}")
        del y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()
    say(f"build {hip.version()}; device {torch.cuda.get_device_name(0)}; warm-up, {ROUNDS} interleaved "
        f"rounds, medians")
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in xa.synth.make_state_dict(seed=42).items()}
    x = torch.from_numpy(xa.synth.make_mfcc(B, T, seed=1)).to(DEV)
    whole_path(sd, x)
    pooling_kernel()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
