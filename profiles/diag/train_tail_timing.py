"""Timing of the training step's tail (include/xvec_train.h: xvec_train_tail_forward / _backward, xvec_adam_step) at the model's
widths for the batches 256 x 300 and 512 x 299 (286 and 285 pooled frames), one box: device time of each HIP call (hipEvents
around the C-ABI call alone) against the same work in eager torch-ROCm ops in the same process -- mean / std / linear / relu /
cross_entropy forward, their autograd backward, torch.optim.Adam.step over the model's 26 parameters -- interleaved round by
round, medians over the rounds.  Each pooling pass's rate against HBM (bench.py's HBM_PEAK) on its algorithmic bytes (one
read of y5 forward; one read plus one write backward): the pass's time is the call's time minus the same call at Tp = 2,
where the pooling is a few microseconds and everything else is unchanged.  Then the whole step: XVectorTrainer(tail="hip").step
against tail="torch", the same build, interleaved.  Run it as one time-limited step:
    timeout -k 10 900 python profiles/diag/train_tail_timing.py"""
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
import train_tail_ref
import xvector_amd as xa
from bench import HBM_PEAK
from xvector_amd import hip

DEV, ROUNDS = "cuda:0", 7
SPREAD = 0.05      # the box-to-box spread README.md records (train_timing.py)
C5, H, K = 1500, 512, 1211


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3      # us


def medians(fns):
    for f in fns:
        f()                                              # warm (a backward needs its forward first: order kept)
    torch.cuda.synchronize()
    return np.median(np.array([[timed(f) for f in fns] for _ in range(ROUNDS)]), 0)


def tail_calls(B, tp):
    """(hip forward, hip backward, eager forward, eager backward) callables on one set of tensors."""
    g = torch.Generator(device=DEV).manual_seed(B + tp)
    uni = lambda fan_in, *shape: (torch.rand(*shape, device=DEV, generator=g) * 2 - 1) / np.sqrt(fan_in)
    y5 = torch.randn(B, tp, C5, device=DEV, generator=g)
    W6, b6, W7, b7, Wo, bo = uni(2 * C5, H, 2 * C5), uni(2 * C5, H), uni(H, H, H), uni(H, H), uni(H, K, H), uni(H, K)
    labels = torch.randint(0, K, (B,), device=DEV, generator=g)
    new = lambda *shape: torch.empty(shape, device=DEV)
    pooled, a6, a7, logits, loss = new(B, 2 * C5), new(B, H), new(B, H), new(B, K), new(1)
    dy5, dW6, db6, dW7, db7, dWo, dbo = new(B, tp, C5), new(H, 2 * C5), new(H), new(H, H), new(H), new(K, H), new(K)
    dloss = torch.ones(1, device=DEV)
    need = hip.lib.xvec_train_tail_workspace_bytes(B, tp, C5, H, K)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def hf():
        rc = hip.lib.xvec_train_tail_forward(p(y5), B, tp, C5, p(W6), p(b6), H, p(W7), p(b7), p(Wo), p(bo), K, p(labels), p(pooled),
                                             p(a6), p(a7), p(logits), p(loss), p(ws), need, s)
        assert rc == 0, hip.lib.xvec_train_last_error()

    def hb():
        rc = hip.lib.xvec_train_tail_backward(p(dloss), p(y5), B, tp, C5, p(W6), H, p(W7), p(Wo), K, p(labels), p(pooled), p(a6),
                                              p(a7), p(logits), p(dy5), p(dW6), p(db6), p(dW7), p(db7), p(dWo), p(dbo), p(ws),
                                              need, s)
        assert rc == 0, hip.lib.xvec_train_last_error()

    leaves = [t.clone().requires_grad_() for t in (y5, W6, b6, W7, b7, Wo, bo)]
    state = {}

    def ef():
        state["loss"] = train_tail_ref.tail_autograd(*leaves, labels)

    def eb():
        torch.autograd.grad(state["loss"], leaves)

    return hf, hb, ef, eb


def adam_calls():
    """(xvec_adam_step, torch.optim.Adam.step) over tensors of the model's 26 parameter shapes."""
    shapes = [tuple(v.shape) for k, v in xa.synth.make_state_dict(seed=42).items()
              if k.endswith(train_ref.PARAM_SUFFIXES)]
    assert len(shapes) == 26, len(shapes)
    params = [torch.randn(sh, device=DEV).requires_grad_() for sh in shapes]
    for q in params:
        q.grad = torch.randn_like(q)
    twins = [q.detach().clone().requires_grad_() for q in params]
    for q, t in zip(params, twins):
        t.grad = q.grad.clone()
    dev_opt, torch_opt = xa.DeviceAdam(params, lr=1e-3), torch.optim.Adam(twins, lr=1e-3)
    return dev_opt.step, torch_opt.step


def report(name, h, e, misses):
    ratio = h / e
    print(f"{name:<34}{h:>11.1f}{e:>12.1f}{ratio:>9.3f}")
    if ratio > 1 + SPREAD:
        misses.append(f"{name}: HIP {h:.0f} us is {ratio - 1:.1%} slower than torch ops {e:.0f} us")


def run_shape(B, T):
    tp = T - 14
    print(f"\n== batch {B} x {T}: y5 [{B}, {tp}, {C5}] = {B * tp * C5 * 4 / 1e6:.0f} MB, H = {H}, K = {K}")
    print(f"{'call':<34}{'HIP us':>11}{'torch us':>12}{'ratio':>9}")
    misses = []
    hf, hb, ef, eb = medians(tail_calls(B, tp))
    report("tail forward", hf, ef, misses)
    report("tail backward", hb, eb, misses)
    torch.cuda.empty_cache()
    hf2, hb2 = medians(tail_calls(B, 2)[:2])
    ha, ea = medians(adam_calls())
    report("adam step (26 tensors)", ha, ea, misses)
    report("tail forward + backward + adam", hf + hb + ha, ef + eb + ea, misses)
    nbytes = B * tp * C5 * 4.0
    for name, t, passes in (("pooling forward", hf - hf2, 1), ("pooling backward", hb - hb2, 2)):
        rate = passes * nbytes / (t * 1e-6)
        print(f"{name}: {t:.1f} us for {passes} pass(es) over y5 (the call minus the same call at Tp = 2): {rate / 1e12:.2f} TB/s, "
              f"{rate / HBM_PEAK:.1%} of the {HBM_PEAK / 1e12:.1f} TB/s HBM figure")
    torch.cuda.empty_cache()

    # the whole step, both tails in this build
    sd = {k_: torch.from_numpy(np.asarray(v)) for k_, v in xa.synth.make_state_dict(seed=42).items()}
    x = torch.from_numpy(xa.synth.make_mfcc(B, T, seed=1)).to(DEV)
    labels = torch.from_numpy(np.random.default_rng(2).integers(0, K, B)).to(DEV)
    steps = []
    for tail in ("hip", "torch"):
        model = xa.XVectorModel()
        model.load_state_dict(sd)
        trainer = xa.XVectorTrainer(model.to(DEV), tail=tail)
        steps.append(lambda trainer=trainer: trainer.step((x, labels, None)))
    h, e = medians(steps)
    print(f"whole step (forward, backward, Adam): tail=\"hip\" {h / 1e3:.2f} ms, tail=\"torch\" {e / 1e3:.2f} ms, ratio {h / e:.3f} "
          f"(done means <= {1 + SPREAD:.2f})")
    if h / e > 1 + SPREAD:
        misses.append(f"whole step: tail=\"hip\" is {h / e - 1:.1%} slower than tail=\"torch\"")
    for m in misses:
        print("MISS " + m)


if __name__ == "__main__":
    print(f"build {hip.version()}; device {torch.cuda.get_device_name(0)}; box {socket.gethostname()}; {ROUNDS} interleaved rounds, "
          f"medians")
    for B, T in ((256, 300), (512, 299)):
        run_shape(B, T)
        torch.cuda.empty_cache()
