"""Timing of ragged training (include/xvec_train.h, "Ragged batches"), one box, hipEvents, interleaved rounds, medians.

1. The old path.  Every HIP call of one lengths=None step at the model's widths -- the five layers forward, the tail forward and
   backward, the five layers backward, through the C ABI on one set of tensors -- from this build and from ANOTHER build of the
   library (--other-lib: the parent commit's libxvec_hip.so), interleaved.  The masked kernels are compile-time variants; the
   unmasked calls must not have moved (the project's 5 % margin).
2. The ragged step.  XVectorTrainer(tail="hip").step on a 256 x 300 batch: lengths=None, all lengths 300, and lengths from
   default_rng(1234).integers(200, 301, 256), the same build, interleaved.  The layout stays padded: the ragged step does the
   padding's arithmetic by design, and adds the masks.
Run it as one time-limited step:
    timeout -k 10 600 python profiles/diag/train_ragged_timing.py [--other-lib PATH]"""
import argparse
import ctypes as C
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import train_ref
import xvector_amd as xa
from xvector_amd import hip

DEV, ROUNDS, SPREAD = "cuda:0", 7, 0.05
WIDTHS = [(24, 512), (512, 512), (512, 512), (512, 512), (512, 1500)]
H, K = 512, 1211
OLD = ("xvec_tdnn_train_workspace_bytes", "xvec_tdnn_train_forward", "xvec_tdnn_train_backward", "xvec_train_tail_workspace_bytes",
       "xvec_train_tail_forward", "xvec_train_tail_backward", "xvec_version")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)            # ms


def medians(fns):
    for f in fns:
        f()
    torch.cuda.synchronize()
    return np.median(np.array([[timed(f) for f in fns] for _ in range(ROUNDS)]), 0)


def bind(path):
    lib = C.CDLL(path)
    for name in OLD:
        fn, ref = getattr(lib, name), getattr(hip.lib, name)
        fn.restype, fn.argtypes = ref.restype, ref.argtypes
    return lib


def step_calls(lib, B, T):
    """The HIP calls of one lengths=None step from `lib`, as one callable."""
    g = torch.Generator(device=DEV).manual_seed(B)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
    p = lambda t: t.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    layers, t = [], T
    x = rnd(B, T, 24)
    for (cin, cout), ctx in zip(WIDTHS, train_ref.CONTEXTS):
        span = ctx[-1] - ctx[0]
        carr = (C.c_int32 * len(ctx))(*ctx)
        L = dict(x=x, B=B, T=t, cin=cin, cout=cout, carr=carr, n=len(ctx), W=rnd(cout, cin * len(ctx)) / np.sqrt(cin * len(ctx)),
                 b=rnd(cout) * 0.1, gamma=torch.ones(cout, device=DEV), beta=torch.zeros(cout, device=DEV),
                 z=torch.empty(B, t - span, cout, device=DEV), y=torch.empty(B, t - span, cout, device=DEV),
                 mean=torch.empty(cout, device=DEV), var=torch.empty(cout, device=DEV), dy=rnd(B, t - span, cout),
                 dx=torch.empty(B, t, cin, device=DEV), dW=torch.empty(cout, cin * len(ctx), device=DEV),
                 db=torch.empty(cout, device=DEV), dg=torch.empty(cout, device=DEV), dbeta=torch.empty(cout, device=DEV))
        L["need"] = lib.xvec_tdnn_train_workspace_bytes(B, t, cin, cout, carr, len(ctx))
        layers.append(L)
        x, t = L["y"], t - span
    need = max([L["need"] for L in layers] + [lib.xvec_train_tail_workspace_bytes(B, t, 1500, H, K)])
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    W6, b6, W7, b7, Wo, bo = rnd(H, 3000) / 55, rnd(H) * 0.1, rnd(H, H) / 23, rnd(H) * 0.1, rnd(K, H) / 23, rnd(K) * 0.1
    labels = torch.randint(0, K, (B,), device=DEV, generator=g)
    new = lambda *shape: torch.empty(shape, device=DEV)
    pooled, a6, a7, logits, loss, dloss = new(B, 3000), new(B, H), new(B, H), new(B, K), new(1), torch.ones(1, device=DEV)
    dW6, db6, dW7, db7, dWo, dbo = new(H, 3000), new(H), new(H, H), new(H), new(K, H), new(K)
    y5, dy5, tp = layers[-1]["y"], layers[-1]["dy"], t

    def run():
        for L in layers:
            rc = lib.xvec_tdnn_train_forward(p(L["x"]), L["B"], L["T"], L["cin"], p(L["W"]), p(L["b"]), L["cout"], L["carr"], L["n"],
                                             p(L["gamma"]), p(L["beta"]), 1e-5, p(L["z"]), p(L["mean"]), p(L["var"]), p(L["y"]),
                                             p(ws), need, s)
            assert rc == 0
        rc = lib.xvec_train_tail_forward(p(y5), B, tp, 1500, p(W6), p(b6), H, p(W7), p(b7), p(Wo), p(bo), K, p(labels), p(pooled),
                                         p(a6), p(a7), p(logits), p(loss), p(ws), need, s)
        assert rc == 0
        rc = lib.xvec_train_tail_backward(p(dloss), p(y5), B, tp, 1500, p(W6), H, p(W7), p(Wo), K, p(labels), p(pooled), p(a6), p(a7),
                                          p(logits), p(dy5), p(dW6), p(db6), p(dW7), p(db7), p(dWo), p(dbo), p(ws), need, s)
        assert rc == 0
        for i, L in reversed(list(enumerate(layers))):
            rc = lib.xvec_tdnn_train_backward(p(L["dy"]), p(L["x"]), p(L["z"]), L["B"], L["T"], L["cin"], p(L["W"]), L["cout"],
                                              L["carr"], L["n"], p(L["gamma"]), p(L["mean"]), p(L["var"]), 1e-5,
                                              p(L["dx"]) if i else None, p(L["dW"]), p(L["db"]), p(L["dg"]), p(L["dbeta"]), p(ws),
                                              need, s)
            assert rc == 0
    return run


def old_path(other):
    lib = bind(other)
    print(f"\n== 1. the HIP calls of one lengths=None step: this build against {lib.xvec_version().decode()}")
    print(f"{'batch':<14}{'this ms':>10}{'other ms':>10}{'ratio':>8}")
    for B, T in ((256, 300), (512, 299)):
        mine, theirs = medians([step_calls(hip.lib, B, T), step_calls(lib, B, T)])
        print(f"{B} x {T:<8}{mine:>10.2f}{theirs:>10.2f}{mine / theirs:>8.3f}" + ("   MISS (> 1.05)" if mine / theirs > 1 + SPREAD else ""))
        torch.cuda.empty_cache()


def ragged_step():
    B, T = 256, 300
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in xa.synth.make_state_dict(seed=42).items()}
    x = torch.from_numpy(xa.synth.make_mfcc(B, T, seed=1)).to(DEV)
    labels = torch.from_numpy(np.random.default_rng(2).integers(0, K, B)).to(DEV)
    drawn = np.random.default_rng(1234).integers(200, 301, B).tolist()
    steps = []
    for lengths in (None, [T] * B, drawn):
        model = xa.XVectorModel()
        model.load_state_dict(sd)
        trainer = xa.XVectorTrainer(model.to(DEV), tail="hip")
        steps.append(lambda trainer=trainer, lengths=lengths: trainer.step((x, labels, None), lengths=lengths))
    none, full, rag = medians(steps)
    share = sum(drawn) / (B * T)
    print(f"\n== 2. the whole step (tail=\"hip\": forward, backward, Adam) at {B} x {T}, this build")
    print(f"lengths=None                        {none:8.2f} ms")
    print(f"lengths = [300] * 256               {full:8.2f} ms   ratio {full / none:.3f}")
    print(f"lengths ~ integers(200, 301)        {rag:8.2f} ms   ratio {rag / none:.3f}   ({share:.1%} of the padded frames are valid: the "
          f"padded layout still does the padding's FLOPs)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib", help="another build of libxvec_hip.so (the parent commit's) for part 1")
    args = ap.parse_args()
    print(f"build {hip.version()}; device {torch.cuda.get_device_name(0)}; box {socket.gethostname()}; {ROUNDS} interleaved rounds, medians")
    if args.other_lib:
        old_path(args.other_lib)
    ragged_step()
