"""The tail of the training step on the GPU (include/xvec_train.h: xvec_train_tail_forward / _backward, xvec_adam_step;
csrc/train_tail.hip) and XVectorTrainer(tail="hip") / DeviceAdam, against the fp64 restatement tests/train_tail_ref.py on the
same fp32 inputs, at the project's fp32 bar: assert_parity at 1e-4.  The worst conditioning of dy5 on these inputs is
max|y| / std of about 100 at Tp = 4, which puts fp32 at about 6e-6: more than a decade inside the bar.

The backward is discontinuous in the ReLU masks [a6 > 0] and [a7 > 0]: the reference backward takes them from the GPU's own a6
and a7, and every case asserts that they differ from the reference's on no more elements than the reference has
pre-activations within 1e-4 mean|pre| of zero -- a share that itself must stay at or below 2e-4.

Every output and the workspace sit inside NaN-poisoned windows of exactly the stated size; the guards on both sides must come
back untouched."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import train_tail_ref as ref
from conftest import assert_parity, load_golden
from test_train import check_buffers, check_grads
from test_train_gpu import ADAM_LOSS_BOUND, fixture_batch, fixture_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                     # floats on either side of every output
FWD = ("pooled", "a6", "a7", "logits")
GRADS = ("dW6", "db6", "dW7", "db7", "dWo", "dbo")


class Window:
    """A NaN-poisoned device buffer of exactly `shape` between two NaN guards."""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        self.t = self.buf[GUARD: GUARD + n].view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what, finite=True):
        assert torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all(), f"{what}: guard overwritten"
        if finite:
            assert torch.isfinite(self.t).all(), f"{what}: window not fully written"
        return self.t.cpu()


def run_tail(case, dloss=1.0, need_dy5=True, nan_loss=False):
    """Both C-ABI calls on one case, every output in a guarded window, the workspace of exactly the queried size between two
    guards and poisoned before each call.  Returns {name: cpu tensor}."""
    from xvector_amd import hip
    d = {k: v.to(DEV).contiguous() for k, v in case.items()}
    B, tp, c = case["y5"].shape
    h, k = case["W6"].shape[0], case["Wo"].shape[0]
    need = hip.lib.xvec_train_tail_workspace_bytes(B, tp, c, h, k)
    assert need > 0 and need % 256 == 0
    wsbuf = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = wsbuf[256: 256 + need]
    ws.view(torch.float32).fill_(float("nan"))
    assert ws.data_ptr() % 256 == 0
    out = {"pooled": Window(B, 2 * c), "a6": Window(B, h), "a7": Window(B, h), "logits": Window(B, k), "loss": Window(1),
           "dW6": Window(h, 2 * c), "db6": Window(h), "dW7": Window(h, h), "db7": Window(h), "dWo": Window(k, h), "dbo": Window(k)}
    if need_dy5:
        out["dy5"] = Window(B, tp, c)
    p = lambda name: out[name].ptr() if name in out else None
    dp = lambda name: d[name].data_ptr()
    dl = torch.tensor([dloss], dtype=torch.float32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    rc = hip.lib.xvec_train_tail_forward(dp("y5"), B, tp, c, dp("W6"), dp("b6"), h, dp("W7"), dp("b7"), dp("Wo"), dp("bo"), k,
                                         dp("labels"), p("pooled"), p("a6"), p("a7"), p("logits"), p("loss"), ws.data_ptr(), need, s)
    assert rc == 0, hip.lib.xvec_train_last_error().decode()
    ws.view(torch.float32).fill_(float("nan"))          # the backward may rely on nothing the forward left there
    rc = hip.lib.xvec_train_tail_backward(dl.data_ptr(), dp("y5"), B, tp, c, dp("W6"), h, dp("W7"), dp("Wo"), k, dp("labels"),
                                          p("pooled"), p("a6"), p("a7"), p("logits"), p("dy5"), p("dW6"), p("db6"), p("dW7"),
                                          p("db7"), p("dWo"), p("dbo"), ws.data_ptr(), need, s)
    assert rc == 0, hip.lib.xvec_train_last_error().decode()
    torch.cuda.synchronize()
    assert (wsbuf[:256] == 0xA5).all() and (wsbuf[-256:] == 0xA5).all(), "workspace guard overwritten"
    return {name: w.check(name, finite=not (nan_loss and name == "loss")) for name, w in out.items()}


def forward64(case):
    c64 = {k: (v.double() if v.is_floating_point() else v) for k, v in case.items()}
    return c64, ref.tail_forward(c64["y5"], c64["W6"], c64["b6"], c64["W7"], c64["b7"], c64["Wo"], c64["bo"], c64["labels"])


def check_tail(case, got, dloss=1.0, need_dy5=True):
    """Everything the two calls wrote against train_tail_ref in fp64, the backward on the GPU's own ReLU masks."""
    c64, f = forward64(case)
    for name in FWD:
        assert_parity(got[name], f[name], what=name)
    loss, want = float(got["loss"][0]), float(f["loss"])
    print(f"[tail] loss {loss:.9f} reference {want:.9f}")
    assert abs(loss - want) <= 1e-4 * abs(want)
    masks = {}
    for name, pre in (("a6", f["pre6"]), ("a7", f["pre7"])):
        masks[name] = got[name] > 0
        near = pre.abs() <= 1e-4 * pre.abs().mean()
        flips = int((masks[name] != (pre > 0)).sum())
        share = float(near.double().mean())
        print(f"[tail] {name} mask: {flips} flips, {int(near.sum())} of {near.numel()} pre-activations near zero ({share:.2e})")
        assert share <= 2e-4, share
        assert flips <= int(near.sum()), (flips, int(near.sum()))
    r = ref.tail_backward(torch.tensor(dloss, dtype=torch.float64), c64["y5"], c64["W6"], c64["W7"], c64["Wo"], c64["labels"],
                          f["pooled"], f["a6"], f["a7"], f["logits"], masks["a6"], masks["a7"])
    for name in GRADS + (("dy5",) if need_dy5 else ()):
        assert_parity(got[name], r[name], what=name)
    assert ("dy5" in got) == need_dy5
    return f, r


@functools.lru_cache(maxsize=None)
def case_of(shape, seed):
    return ref.make_case(*shape, seed)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tail_forward_and_backward(shape, seed):
    case = case_of(shape, seed)
    check_tail(case, run_tail(case))


def test_constant_channels():
    """A channel that is constant over an utterance: std exactly 0, and of dy5 only the mean's share is left, the same value
    dmean / Tp in every frame.  The call's own dmean lives in its workspace and is no output, so "exactly dmean / Tp" is
    asserted as: bit-equal over the utterance's frames (any std term would vary with the frame) and equal to the
    reference's dmean / Tp at the common bar."""
    shape = (3, 7, 65, 33, 5)
    case = {k: v.clone() for k, v in case_of(shape, 1).items()}
    case["y5"][:, :, 11] = 3.25
    case["y5"][1, :, 40] = -1e3
    got = run_tail(case)
    f, r = check_tail(case, got)
    c = shape[2]
    assert (got["pooled"][:, c + 11] == 0).all() and got["pooled"][1, c + 40] == 0
    assert (got["pooled"][:, 11] == 3.25).all() and got["pooled"][1, 40] == -1e3
    assert (got["pooled"][[0, 2], c + 40] > 0).all()
    assert all(torch.isfinite(v).all() for k, v in got.items())
    for dy, dmean in ((got["dy5"][:, :, 11], r["dpooled"][:, 11]), (got["dy5"][1:2, :, 40], r["dpooled"][1:2, 40])):
        assert (dy == dy[:, :1]).all()                                   # one value per utterance: dmean / Tp, no std term
        assert_parity(dy[:, 0], dmean / shape[1], what="dmean / Tp")


@pytest.mark.parametrize("shape", [(3, 7, 65, 33, 5), (2, 300, 96, 16, 3)], ids=lambda s: "x".join(map(str, s)))
def test_ill_conditioned_pooling(shape):
    """y5 = 1e4 + randn: mean^2 = 1e8 var.  The std survives because the sums run over deviations about a pivot; the
    mean-squared-minus-squared-mean formula loses every digit here."""
    case = {k: v.clone() for k, v in case_of(shape, 2).items()}
    case["y5"] += 1e4
    got = run_tail(case)
    _, f = forward64(case)
    c = shape[2]
    std, want = got["pooled"][:, c:].double(), f["pooled"][:, c:]
    err = ((std - want).abs() / want).max().item()
    print(f"[tail] ill-conditioned std: max relative error {err:.3e}")
    assert err <= 1e-4
    assert_parity(got["pooled"][:, :c], f["pooled"][:, :c], what="mean")


def test_label_out_of_range():
    shape = (130, 5, 64, 129, 1211)
    case = {k: v.clone() for k, v in case_of(shape, 1).items()}
    good = run_tail(case)
    case["labels"][7] = shape[4]
    got = run_tail(case, nan_loss=True)                  # the guards of every window and of the workspace are checked in there
    assert torch.isnan(got["loss"]).all()
    assert torch.equal(got["logits"], good["logits"])
    case["labels"][7] = -1
    assert torch.isnan(run_tail(case, nan_loss=True)["loss"]).all()


def test_null_dy5_leaves_the_parameter_gradients_bit_equal():
    case = case_of((3, 7, 65, 33, 5), 3)
    with_dy5, without = run_tail(case), run_tail(case, need_dy5=False)
    assert "dy5" not in without
    check_tail(case, without, need_dy5=False)
    for name in FWD + GRADS + ("loss",):
        assert torch.equal(with_dy5[name], without[name]), name


@pytest.mark.parametrize("shape", [(3, 7, 65, 33, 5), (256, 4, 1500, 512, 1211)], ids=lambda s: "x".join(map(str, s)))
def test_repeat_calls_are_bit_identical(shape):
    case = case_of(shape, 2)
    a, b = run_tail(case), run_tail(case)
    assert sorted(a) == sorted(b) and len(a) == 12
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_dloss_scales_every_gradient():
    case = case_of((4, 26, 1500, 32, 7), 2)
    one, got = run_tail(case), run_tail(case, dloss=0.37)
    check_tail(case, got, dloss=0.37)
    for name in GRADS + ("dy5",):
        assert_parity(got[name], 0.37 * one[name].double(), tol=1e-5, what=name)       # the scale enters before the products
    for name in FWD + ("loss",):
        assert torch.equal(one[name], got[name]), name


# ---------------------------------------------------------------- xvec_adam_step alone
ADAM_LENGTHS = (1, 3, 4, 5, 1211, 4097, 1536000)        # the last: segment_layer6.weight
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def _guarded(values, lead):
    """`values` as a device slice `lead` floats into its allocation, NaN on both sides."""
    buf = torch.full((lead + values.numel() + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    t = buf[lead: lead + values.numel()]
    t.copy_(values)
    return buf, t


def test_adam_step_alone():
    """34 tensors (two launches), every length class, every tensor one float into its allocation: a base that is 4-byte
    aligned only.  On odd tensors the gradient starts two floats in, so the four bases do not share their misalignment and
    the tensor goes element by element.  Steps t = 1, 2, 1000, each from the GPU's own state before it, against the fp64
    formulas on the same fp32 values:
      m, v   within 1e-6 relative: two fp32 roundings each plus room (m and g share their sign, v's terms are positive:
             nothing cancels);
      p      |p' - p_ref'| <= 2^-23 |p| + 1e-5 lr max(1, |u_ref|), u the normalised update: a dozen fp32 roundings cost about
             1e-6 of the update, u is Lipschitz in a relative error of g with constant at most 1/4 even where |g| is about
             eps, the rest is one decade of room; the first term is the rounding of p itself."""
    from xvector_amd import hip
    gen = torch.Generator().manual_seed(7)
    lengths = [ADAM_LENGTHS[i % len(ADAM_LENGTHS)] for i in range(34)]
    tensors = []
    for i, n in enumerate(lengths):
        g = 10.0 ** (torch.rand(n, generator=gen) * 14 - 12) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()
        g[torch.rand(n, generator=gen) < 0.05] = 0.0
        if n >= 4:
            g[1] = 0.0
        m = g * torch.rand(n, generator=gen)
        v = g * g * 2 * torch.rand(n, generator=gen)
        p = torch.randn(n, generator=gen)
        tensors.append({"p": _guarded(p, 1), "g": _guarded(g, 1 + i % 2), "m": _guarded(m, 1), "v": _guarded(v, 1)})
    assert tensors[0]["p"][1].data_ptr() % 16 == 4 and tensors[1]["g"][1].data_ptr() % 16 == 8
    table = lambda key: (C.c_void_p * 34)(*[t[key][1].data_ptr() for t in tensors])
    n_arr = (C.c_int64 * 34)(*lengths)
    s = torch.cuda.current_stream().cuda_stream
    for step in (1, 2, 1000):
        before = [{k: t[k][1].cpu().double() for k in "pgmv"} for t in tensors]
        rc = hip.lib.xvec_adam_step(table("p"), table("g"), table("m"), table("v"), n_arr, 34, LR, B1, B2, EPS, step, s)
        assert rc == 0, hip.lib.xvec_train_last_error().decode()
        torch.cuda.synchronize()
        worst = {"m": 0.0, "v": 0.0, "p": 0.0}
        for i, (t, b) in enumerate(zip(tensors, before)):
            for k in "pgmv":
                buf, view = t[k]
                lead = 1 + i % 2 if k == "g" else 1
                assert torch.isnan(buf[:lead]).all() and torch.isnan(buf[lead + view.numel():]).all(), f"tensor {i} {k}: guard"
            assert torch.equal(t["g"][1].cpu().double(), b["g"]), f"tensor {i}: the gradient was written"
            p_ref, m_ref, v_ref, u_ref = ref.adam_step(b["p"], b["g"], b["m"], b["v"], LR, B1, B2, EPS, step)
            got = {k: t[k][1].cpu().double() for k in "pmv"}
            for k, want in (("m", m_ref), ("v", v_ref)):
                err = (got[k] - want).abs()
                assert (err <= 1e-6 * want.abs()).all(), f"step {step} tensor {i} {k}: {(err / want.abs().clamp_min(1e-300)).max():.3e}"
                worst[k] = max(worst[k], float((err / want.abs().clamp_min(1e-300)).max()))
            bound = 2.0 ** -23 * b["p"].abs() + 1e-5 * LR * u_ref.abs().clamp_min(1.0)
            err = (got["p"] - p_ref).abs()
            assert (err <= bound).all(), f"step {step} tensor {i} p: {(err / bound).max():.3e} of the bound"
            worst["p"] = max(worst["p"], float((err / bound).max()))
            still = (b["g"] == 0) & (b["m"] == 0) & (b["v"] == 0)
            assert still.any() or t["p"][1].numel() < 4
            assert torch.equal(got["p"][still], b["p"][still]), f"step {step} tensor {i}: a zero gradient moved p"
            assert (got["m"][still] == 0).all() and (got["v"][still] == 0).all()
        print(f"[adam] t = {step}: worst relative error m {worst['m']:.2e}, v {worst['v']:.2e}; p at {worst['p']:.2e} of its bound")


# ---------------------------------------------------------------- the whole step
@pytest.fixture(scope="module")
def g10():
    return load_golden("g10_train.npz")


def test_training_step_matches_the_reference(g10, synth):
    import xvector_amd as xa
    model = fixture_model(g10, synth)
    out = xa.XVectorTrainer(model, tail="hip").training_step(fixture_batch(g10), 0)
    assert sorted(out) == ["loss", "train_id", "train_labels", "train_preds"]
    assert out["train_preds"].shape == (int(g10["B"]), int(g10["num_classes"])) and out["train_id"] == fixture_batch(g10)[2]
    assert out["loss"].requires_grad and out["loss"].dim() == 0 and not out["train_preds"].requires_grad
    out["loss"].backward()
    print(f"[tail] loss {out['loss'].item():.9f} fixture {float(g10['loss']):.9f}")
    assert abs(out["loss"].item() - float(g10["loss"])) <= 1e-4 * float(g10["loss"])
    check_grads(g10, {k: p.grad for k, p in model.named_parameters()}, 1e-4, "step")
    check_buffers(g10, model.state_dict(), 1e-4, "step")


def _check_adam_losses(g10, losses):
    dev = np.abs(np.array(losses) - g10["adam_losses"]) / g10["adam_losses"]
    print(f"[tail] adam losses {list(losses)} relative deviation {dev.tolist()} bound {ADAM_LOSS_BOUND:.3e}")
    assert dev[0] <= 1e-4
    assert dev[1:].max() <= ADAM_LOSS_BOUND, dev


def test_adam_losses_of_steps_two_and_three(g10, synth):
    import xvector_amd as xa
    trainer = xa.XVectorTrainer(fixture_model(g10, synth), tail="hip")
    batch = fixture_batch(g10)
    losses = [float(trainer.step(batch)) for _ in range(3)]
    assert isinstance(trainer.optimizer, xa.DeviceAdam) and len(trainer.optimizer.state) == 26
    _check_adam_losses(g10, losses)


def test_one_step_twice_is_bit_identical(g10, synth):
    import xvector_amd as xa
    results = []
    for _ in range(2):
        model = fixture_model(g10, synth)
        trainer = xa.XVectorTrainer(model, tail="hip")
        loss = trainer.step(fixture_batch(g10))
        opt = trainer.optimizer.state_dict()["state"]
        results.append([loss.cpu()] + [v.detach().cpu() for v in model.state_dict().values()]
                       + [st[k].cpu() for _, st in sorted(opt.items()) for k in ("step", "exp_avg", "exp_avg_sq")])
    assert len(results[0]) == len(results[1]) > 20 + 3 * 26
    for a, b in zip(*results):
        assert torch.equal(a, b)


@pytest.mark.parametrize("first", ["device", "torch"])
def test_a_run_can_switch_optimizer_either_way(g10, synth, first):
    """One step under one optimizer, its state_dict loaded into the other, two more steps: the fixture's Adam losses."""
    import xvector_amd as xa
    model = fixture_model(g10, synth)
    trainer = xa.XVectorTrainer(model, tail="hip")
    batch = fixture_batch(g10)
    make = {"device": lambda: xa.DeviceAdam(model.parameters(), lr=model.learning_rate),
            "torch": lambda: torch.optim.Adam(model.parameters(), lr=model.learning_rate)}
    trainer.optimizer = make[first]()
    losses = [float(trainer.step(batch))]
    sd = trainer.optimizer.state_dict()
    assert sorted(sd["state"]) == list(range(26)) and sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    trainer.optimizer = make["torch" if first == "device" else "device"]()
    trainer.optimizer.load_state_dict(sd)
    losses += [float(trainer.step(batch)) for _ in range(2)]
    _check_adam_losses(g10, losses)
    assert int(trainer.optimizer.state_dict()["state"][0]["step"]) == 3


def test_checkpoint_round_trip(g10, synth, tmp_path):
    import xvector_amd as xa
    model = fixture_model(g10, synth)
    model.x_vec_extract_layer = 7
    trainer = xa.XVectorTrainer(model, tail="hip")
    trainer.step(fixture_batch(g10))
    path = str(tmp_path / "last.ckpt")
    trainer.save_checkpoint(path)
    back = xa.XVectorModel.load_from_checkpoint(path)
    assert back.x_vec_extract_layer == 7 and back.hparams == model.hparams and back.learning_rate == model.learning_rate
    sd, sd2 = model.state_dict(), back.state_dict()
    assert list(sd) == list(sd2)
    for k in sd:
        assert torch.equal(sd[k].cpu(), sd2[k]), k


def test_device_adam_skips_and_refuses(g10, synth):
    """A parameter without a gradient is skipped, as torch skips it; a parameter that is not contiguous raises."""
    import xvector_amd as xa
    a = torch.nn.Parameter(torch.ones(5, device=DEV))
    b = torch.nn.Parameter(torch.ones(3, device=DEV))
    opt = xa.DeviceAdam([a, b], lr=0.1)
    a.grad = torch.full((5,), 2.0, device=DEV)
    opt.step()
    assert sorted(opt.state) == [0] and torch.equal(b.detach().cpu(), torch.ones(3))
    assert torch.allclose(a.detach().cpu(), torch.full((5,), 0.9), rtol=1e-6)          # the first step moves by lr sign(g)
    opt.zero_grad()
    assert a.grad is None
    with pytest.raises(RuntimeError, match="not contiguous"):
        xa.DeviceAdam([torch.nn.Parameter(torch.ones(4, 4, device=DEV).t())]).step()
    val = xa.XVectorTrainer(fixture_model(g10, synth), tail="hip").validation_step(fixture_batch(g10))
    assert sorted(val) == ["loss", "val_id", "val_labels", "val_preds"] and not val["loss"].requires_grad
