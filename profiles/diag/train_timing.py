"""Timing of the training-mode TDNN layers (include/xvec_train.h) at 256 x 300 x 24 and 512 x 299 x 24, one box: device time of
each layer's forward call and backward call (hipEvents around the C-ABI call alone), the algorithmic FLOPs (2 N K Cout forward,
twice that backward; layer 1 has no dx: 2 N K Cout) and the call's rate against the 157.3 TFLOP/s fp32 matrix peak -- a call is
its product(s) plus the element-wise passes around them, so the fraction is a floor for the products themselves.  The yardstick
is the same layer written with eager torch-ROCm ops (cat, F.linear, relu, batch_norm; autograd backward), on the same box,
interleaved with the HIP calls round by round (medians over the rounds), and the whole step: XVectorTrainer.step against
tests/train_ref.py's op sequence with torch.optim.Adam.  Run it as one time-limited step:
    timeout -k 10 900 python profiles/diag/train_timing.py"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.nn.functional as F

import train_ref
import xvector_amd as xa
from xvector_amd import hip

DEV, PEAK, ROUNDS = "cuda:0", 157.3, 7
SPREAD = 0.05      # the box-to-box spread README.md records


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3      # us


def layer_pair(B, T, cin, cout, ctx, need_dx):
    """(hip forward, hip backward, eager forward, eager backward) callables on one layer's tensors."""
    g = torch.Generator(device=DEV).manual_seed(cin + cout)
    k = 1.0 / np.sqrt(cin * len(ctx))
    x = torch.randn(B, T, cin, device=DEV, generator=g)
    W = (torch.rand(cout, cin * len(ctx), device=DEV, generator=g) * 2 - 1) * k
    b = (torch.rand(cout, device=DEV, generator=g) * 2 - 1) * k
    gamma, beta = torch.rand(cout, device=DEV, generator=g) + 0.5, torch.zeros(cout, device=DEV)
    tp = T - (ctx[-1] - ctx[0])
    dy = torch.randn(B, tp, cout, device=DEV, generator=g)
    z, y = torch.empty_like(dy), torch.empty_like(dy)
    mean, var = torch.empty(cout, device=DEV), torch.empty(cout, device=DEV)
    dx, dW = torch.empty_like(x), torch.empty_like(W)
    db, dg, dbe = torch.empty(cout, device=DEV), torch.empty(cout, device=DEV), torch.empty(cout, device=DEV)
    carr = (C.c_int32 * len(ctx))(*ctx)
    need = hip.lib.xvec_tdnn_train_workspace_bytes(B, T, cin, cout, carr, len(ctx))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream

    def hf():
        rc = hip.lib.xvec_tdnn_train_forward(x.data_ptr(), B, T, cin, W.data_ptr(), b.data_ptr(), cout, carr, len(ctx),
                                             gamma.data_ptr(), beta.data_ptr(), 1e-5, z.data_ptr(), mean.data_ptr(),
                                             var.data_ptr(), y.data_ptr(), ws.data_ptr(), need, s)
        assert rc == 0, hip.lib.xvec_train_last_error()

    def hb():
        rc = hip.lib.xvec_tdnn_train_backward(dy.data_ptr(), x.data_ptr(), z.data_ptr(), B, T, cin, W.data_ptr(), cout, carr,
                                              len(ctx), gamma.data_ptr(), mean.data_ptr(), var.data_ptr(), 1e-5,
                                              dx.data_ptr() if need_dx else None, dW.data_ptr(), db.data_ptr(), dg.data_ptr(),
                                              dbe.data_ptr(), ws.data_ptr(), need, s)
        assert rc == 0, hip.lib.xvec_train_last_error()

    leaves = [t.clone().requires_grad_() for t in (W, b, gamma, beta)]
    xe = x.clone().requires_grad_(need_dx)
    state = {}

    def ef():
        state["y"] = train_ref.layer_autograd(xe, leaves[0], leaves[1], ctx, leaves[2], leaves[3])

    def eb():
        torch.autograd.grad(state["y"], ([xe] if need_dx else []) + leaves, dy)

    return hf, hb, ef, eb


def run_shape(B, T):
    print(f"\n== batch {B} x {T} x 24")
    print(f"{'layer':<7}{'N':>8}{'K':>6}{'Cout':>6} | {'hip fwd us':>11}{'TF':>7}{'peak':>7} | {'hip bwd us':>11}{'TF':>7}{'peak':>7} | "
          f"{'eager fwd':>10}{'eager bwd':>10} | fwd+bwd hip/eager")
    tot_h = tot_e = 0.0
    t = T
    misses = []
    for i, (cin, cout, ctx) in enumerate(xa.synth.layer_dims()):
        fns = layer_pair(B, t, cin, cout, ctx, need_dx=i > 0)
        for f in fns[:2] + fns[2:]:
            f()                                           # warm (the eager backward needs its forward first: order kept)
        torch.cuda.synchronize()
        times = np.array([[timed(f) for f in fns] for _ in range(ROUNDS)])     # interleaved: hip, hip, eager, eager per round
        hf, hb, ef, eb = np.median(times, 0)
        tp = t - (ctx[-1] - ctx[0])
        n, k = B * tp, cin * len(ctx)
        fl_f = 2.0 * n * k * cout
        fl_b = fl_f * (2 if i > 0 else 1)
        tf_f, tf_b = fl_f / hf * 1e-6, fl_b / hb * 1e-6
        ratio = (hf + hb) / (ef + eb)
        print(f"tdnn{i + 1:<3}{n:>8}{k:>6}{cout:>6} | {hf:>11.1f}{tf_f:>7.1f}{tf_f / PEAK:>7.1%} | {hb:>11.1f}{tf_b:>7.1f}{tf_b / PEAK:>7.1%} | "
              f"{ef:>10.1f}{eb:>10.1f} | {ratio:.3f}")
        if ratio > 1 + SPREAD:
            misses.append(f"tdnn{i + 1}: HIP forward + backward {hf + hb:.0f} us is {ratio - 1:.1%} slower than eager {ef + eb:.0f} us "
                          f"(forward {hf / ef:.2f} x, backward {hb / eb:.2f} x eager)")
        tot_h += hf + hb
        tot_e += ef + eb
        t = tp
        del fns
        torch.cuda.empty_cache()
    print(f"frame-level forward + backward: HIP {tot_h / 1e3:.2f} ms, eager {tot_e / 1e3:.2f} ms, ratio {tot_h / tot_e:.3f} "
          f"(done means <= {1 + SPREAD:.2f})")
    for m in misses:
        print("MISS " + m)
    if tot_h / tot_e > 1 + SPREAD:
        print(f"MISS frame-level total: {tot_h / tot_e - 1:.1%} slower than eager")

    # the whole step
    sd = {k_: torch.from_numpy(np.asarray(v)) for k_, v in xa.synth.make_state_dict(seed=42).items()}
    model = xa.XVectorModel()
    model.load_state_dict(sd)
    trainer = xa.XVectorTrainer(model.to(DEV))
    x = torch.from_numpy(xa.synth.make_mfcc(B, T, seed=1)).to(DEV)
    labels = torch.from_numpy(np.random.default_rng(2).integers(0, 1211, B)).to(DEV)
    esd = train_ref.cast_state({k_: v.to(DEV) for k_, v in sd.items()}, torch.float32)
    opt = torch.optim.Adam([esd[k_] for k_ in train_ref.param_keys(esd)], lr=1e-3)

    def eager_step():
        opt.zero_grad(set_to_none=True)
        F.cross_entropy(train_ref.logits(esd, x), labels).backward()
        opt.step()

    hip_step = lambda: trainer.step((x, labels, None))
    for _ in range(2):
        hip_step(); eager_step()
    torch.cuda.synchronize()
    times = np.array([[timed(hip_step), timed(eager_step)] for _ in range(ROUNDS)])
    h, e = np.median(times, 0)
    print(f"whole step (forward, backward, Adam): HIP frame-level layers + torch tail {h / 1e3:.2f} ms, all eager {e / 1e3:.2f} ms, "
          f"ratio {h / e:.3f}")


if __name__ == "__main__":
    print(f"build {hip.version()}; device {torch.cuda.get_device_name(0)}; {ROUNDS} interleaved rounds, medians")
    for B, T in ((256, 300), (512, 299)):
        run_shape(B, T)
        torch.cuda.empty_cache()
