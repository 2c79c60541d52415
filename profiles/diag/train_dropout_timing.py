"""Timing of dropout in training (include/xvec_train.h, "Dropout"), one box, hipEvents, interleaved rounds, medians; collected the
way profiles/diag/train_ragged_timing.py collects (whose step_calls and medians this uses).

1. The unchanged path.  Every HIP call of one dropout_p = 0 step at the model's widths from this build and from ANOTHER build of
   the library (--other-lib: the parent commit's libxvec_hip.so), interleaved.  Dropout is a compile-time variant in a file of its
   own; the calls without it must not have moved (the project's 5 % margin).
2. The forward call per layer: xvec_tdnn_train_forward against xvec_tdnn_train_forward_dropout with p = 0.1 on the same tensors --
   what the Philox rounds in the product's epilogue cost.
3. The whole step.  XVectorTrainer(tail="hip").step with dropout_p = 0 and with dropout_p = 0.1, the same build, interleaved.
Run it as one time-limited step:
    timeout -k 10 600 python profiles/diag/train_dropout_timing.py [--other-lib PATH]"""
import argparse
import ctypes as C
import os
import socket
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import train_ragged_timing as base
import train_ref
import xvector_amd as xa
from xvector_amd import hip

DEV, K = base.DEV, base.K
BATCHES = ((256, 300), (512, 299))


def unchanged_path(other):
    lib = base.bind(other)
    print(f"\n== 1. the HIP calls of one dropout_p = 0 step: this build against {lib.xvec_version().decode()}")
    print(f"{'batch':<14}{'this ms':>10}{'other ms':>10}{'ratio':>8}")
    for B, T in BATCHES:
        mine, theirs = base.medians([base.step_calls(hip.lib, B, T), base.step_calls(lib, B, T)])
        print(f"{B} x {T:<8}{mine:>10.2f}{theirs:>10.2f}{mine / theirs:>8.3f}" + ("   MISS (> 1.05)" if mine / theirs > 1 + base.SPREAD else ""))
        torch.cuda.empty_cache()


def forward_per_layer():
    print("\n== 2. the forward call per layer: without dropout against p = 0.1 (the mask in the product's epilogue)")
    print(f"{'batch':<12}{'layer':<22}{'plain ms':>10}{'dropout ms':>12}{'ratio':>8}")
    for B, T in BATCHES:
        g = torch.Generator(device=DEV).manual_seed(B)
        rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
        p = lambda t: t.data_ptr()
        s = torch.cuda.current_stream().cuda_stream
        t = T
        for i, ((cin, cout), ctx) in enumerate(zip(base.WIDTHS, train_ref.CONTEXTS)):
            span = ctx[-1] - ctx[0]
            carr = (C.c_int32 * len(ctx))(*ctx)
            x, W, b = rnd(B, t, cin), rnd(cout, cin * len(ctx)) / np.sqrt(cin * len(ctx)), rnd(cout) * 0.1
            gamma, beta = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
            z, y = torch.empty(B, t - span, cout, device=DEV), torch.empty(B, t - span, cout, device=DEV)
            mean, var = torch.empty(cout, device=DEV), torch.empty(cout, device=DEV)
            need = hip.lib.xvec_tdnn_train_workspace_bytes(B, t, cin, cout, carr, len(ctx))
            ws = torch.empty(need, dtype=torch.uint8, device=DEV)
            args = (p(x), B, t, cin, p(W), p(b), cout, carr, len(ctx), p(gamma), p(beta), 1e-5, p(z), p(mean), p(var), p(y), p(ws), need, s)

            def plain(args=args):
                assert hip.lib.xvec_tdnn_train_forward(*args) == 0

            def dropout(args=args, i=i):
                assert hip.lib.xvec_tdnn_train_forward_dropout(*args, None, 0.1, 1234, i) == 0

            a, d = base.medians([plain, dropout])
            print(f"{B} x {T:<6}{i + 1} ({cin} x {len(ctx)} -> {cout}){'':<4}{a:>10.3f}{d:>12.3f}{d / a:>8.3f}")
            t -= span
            del x, W, z, y, ws
            torch.cuda.empty_cache()


def whole_step():
    print("\n== 3. the whole step (tail=\"hip\": forward, backward, Adam), this build")
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in xa.synth.make_state_dict(seed=42).items()}
    for B, T in BATCHES:
        x = torch.from_numpy(xa.synth.make_mfcc(B, T, seed=1)).to(DEV)
        labels = torch.from_numpy(np.random.default_rng(2).integers(0, K, B)).to(DEV)
        steps = []
        for p in (0.0, 0.1):
            model = xa.XVectorModel(dropout_p=p)
            model.load_state_dict(sd)
            trainer = xa.XVectorTrainer(model.to(DEV), tail="hip", dropout_seed=1234)
            steps.append(lambda trainer=trainer: trainer.step((x, labels, None)))
        none, drop = base.medians(steps)
        print(f"{B} x {T}: dropout_p = 0 {none:8.2f} ms   dropout_p = 0.1 {drop:8.2f} ms   ratio {drop / none:.3f}"
              + ("   (> 1.05)" if drop / none > 1 + base.SPREAD else ""))
        del steps, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib", help="another build of libxvec_hip.so (the parent commit's) for part 1")
    args = ap.parse_args()
    print(f"build {hip.version()}; device {torch.cuda.get_device_name(0)}; box {socket.gethostname()}; {base.ROUNDS} interleaved rounds, medians")
    if args.other_lib:
        unchanged_path(args.other_lib)
    forward_per_layer()
    whole_step()
