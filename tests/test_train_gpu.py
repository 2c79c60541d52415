"""The training-mode TDNN layer (include/xvec_train.h, csrc/tdnn_train.hip) and xvector_amd.train on the GPU, against the fp64
restatement tests/train_ref.py on the same fp32 inputs, at the project's fp32 bar: assert_parity at 1e-4 (row-wise relative
plus element-wise).  fp32 torch stays at or below 1e-6 of fp64 torch on these quantities, so the bar has two decades of room.

The backward is discontinuous in the ReLU mask [z > 0]: the reference backward takes the mask from the GPU's own z, and every
case asserts that this mask differs from the reference's on no more elements than the reference has pre-activations within
1e-4 mean|pre| of zero -- a share that itself must stay at or below 2e-4 (Gaussian inputs, default-initialised weights).

Every output and the workspace sit inside NaN-poisoned windows of exactly the stated size; the guards on both sides must come
back untouched.  Sizes at the kernels' boundaries: profiles/train_edges.txt."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import train_ref
import xvector_oracle as oracle
from conftest import assert_parity, float_params, load_golden
from test_train import KW, check_buffers, check_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                     # floats on either side of every output
CTX = train_ref.CONTEXTS
# 10 x the deviation of train_ref run in fp32 on the CPU from the fixture's Adam losses of steps 2 and 3 (8.08e-8 relative,
# measured with one and with eight threads; profiles/train_edges.txt): Adam's first steps are close to lr * sign(g), so no bar
# can be derived for them
ADAM_LOSS_BOUND = 10 * 8.08e-8


class Window:
    """A NaN-poisoned device buffer of exactly `shape` between two NaN guards."""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        self.t = self.buf[GUARD: GUARD + n].view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        assert torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all(), f"{what}: guard overwritten"
        assert torch.isfinite(self.t).all(), f"{what}: window not fully written"
        return self.t.cpu()


def make_case(B, T, cin, cout, context, bn, seed, bias_edit=None):
    rng = np.random.default_rng(seed)
    k = 1.0 / np.sqrt(cin * len(context))
    c = {"x": rng.standard_normal((B, T, cin), dtype=np.float32),
         "W": rng.uniform(-k, k, (cout, cin * len(context))).astype(np.float32),
         "b": rng.uniform(-k, k, cout).astype(np.float32)}
    if bias_edit:
        for ch, v in bias_edit.items():
            c["b"][ch] = v
    if bn:
        c["gamma"] = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        c["beta"] = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    tp = T - (context[-1] - context[0])
    c["dy"] = rng.standard_normal((B, tp, cout), dtype=np.float32)
    return {k_: torch.from_numpy(v) for k_, v in c.items()}


def run_layer(case, context, need_dx=True, eps=train_ref.EPS):
    """Both C-ABI calls on one case, every output in a guarded window, the workspace of exactly the queried size between two
    guards.  Returns {name: cpu tensor}."""
    from xvector_amd import hip
    bn = "gamma" in case
    d = {k: v.to(DEV).contiguous() for k, v in case.items()}
    B, T, cin = case["x"].shape
    cout = case["W"].shape[0]
    tp = case["dy"].shape[1]
    carr = (C.c_int32 * len(context))(*context)
    need = hip.lib.xvec_tdnn_train_workspace_bytes(B, T, cin, cout, carr, len(context))
    assert need > 0 and need % 256 == 0
    wsbuf = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = wsbuf[256: 256 + need]
    ws.view(torch.float32).fill_(float("nan"))
    assert ws.data_ptr() % 256 == 0
    out = {"z": Window(B, tp, cout), "dW": Window(cout, cin * len(context)), "db": Window(cout)}
    if bn:
        out.update(y=Window(B, tp, cout), mean=Window(cout), var=Window(cout), dgamma=Window(cout), dbeta=Window(cout))
    if need_dx:
        out["dx"] = Window(B, T, cin)
    p = lambda name: out[name].ptr() if name in out else None
    dp = lambda name: d[name].data_ptr() if name in d else None
    s = torch.cuda.current_stream().cuda_stream
    rc = hip.lib.xvec_tdnn_train_forward(dp("x"), B, T, cin, dp("W"), dp("b"), cout, carr, len(context), dp("gamma"), dp("beta"),
                                         eps, p("z"), p("mean"), p("var"), p("y"), ws.data_ptr(), need, s)
    assert rc == 0, hip.lib.xvec_train_last_error().decode()
    ws.view(torch.float32).fill_(float("nan"))          # the backward may rely on nothing the forward left there
    rc = hip.lib.xvec_tdnn_train_backward(dp("dy"), dp("x"), p("z"), B, T, cin, dp("W"), cout, carr, len(context), dp("gamma"),
                                          p("mean"), p("var"), eps, p("dx"), p("dW"), p("db"), p("dgamma"), p("dbeta"),
                                          ws.data_ptr(), need, s)
    assert rc == 0, hip.lib.xvec_train_last_error().decode()
    torch.cuda.synchronize()
    assert (wsbuf[:256] == 0xA5).all() and (wsbuf[-256:] == 0xA5).all(), "workspace guard overwritten"
    return {k: w.check(k) for k, w in out.items()}


def check_layer(case, context, got, need_dx=True, eps=train_ref.EPS, edited=()):
    """Everything the two calls wrote against train_ref in fp64, the backward on the GPU's own ReLU mask.  `edited`: channels
    whose bias a test moved far from zero; they stay out of mean|pre|, the scale of "near zero"."""
    c64 = {k: v.double() for k, v in case.items()}
    bn = "gamma" in case
    f = train_ref.layer_forward(c64["x"], c64["W"], c64["b"], context, c64.get("gamma"), c64.get("beta"), eps)
    mask = got["z"] > 0
    keep = [ch for ch in range(f["pre"].shape[-1]) if ch not in edited]
    near = (f["pre"].abs() <= 1e-4 * f["pre"][..., keep].abs().mean())
    flips = int((mask != (f["pre"] > 0)).sum())
    share = float(near.double().mean())
    print(f"[train] mask: {flips} flips, {int(near.sum())} of {near.numel()} pre-activations near zero ({share:.2e})")
    assert share <= 2e-4, share
    assert flips <= int(near.sum()), (flips, int(near.sum()))
    assert_parity(got["z"], f["z"], what="z")
    if bn:
        assert_parity(got["y"], f["y"], what="y")
        assert_parity(got["mean"], f["mean"], what="batch_mean")
        assert_parity(1.0 / torch.sqrt(got["var"].double() + eps), f["invstd"], what="1/sqrt(var+eps)")
    r = train_ref.layer_backward(c64["dy"], c64["x"], f["z"], mask, c64["W"], context, c64.get("gamma"), f.get("mean"),
                                 f.get("var"), eps)
    names = ["dW", "db"] + (["dgamma", "dbeta"] if bn else []) + (["dx"] if need_dx else [])
    for name in names:
        assert_parity(got[name], r[name], what=name)
    assert ("dx" in got) == need_dx
    return f, r


LAYER_CASES = [
    # B, T, Cin, Cout, context, BatchNorm, dx, seed
    (5, 33, 24, 512, CTX[0], True, False, 1),        # layer 1 as the model runs it: no dx
    (3, 40, 512, 512, CTX[1], True, True, 2),
    (2, 19, 512, 512, CTX[2], True, True, 3),
    (3, 40, 512, 512, CTX[3], True, True, 4),
    (3, 40, 512, 1500, CTX[4], True, True, 5),
    (5, 33, 24, 512, CTX[0], False, True, 6),        # no BatchNorm
    (3, 40, 512, 1500, CTX[4], False, False, 7),
    (3, 104, 20, 72, CTX[1], True, True, 8),         # odd widths, N = 300: two dW slices, utterance ends inside a slice
    (3, 104, 20, 72, CTX[2], False, True, 9),
    (2, 37, 7, 13, CTX[0], True, True, 10),          # widths that are no multiple of 4: the element-wise loaders
    (2, 37, 13, 7, CTX[2], True, True, 11),
    (2, 150, 130, 129, [-4, -1, 0, 3], True, True, 12),   # one past the tile in both widths, an uneven context
]


@pytest.mark.parametrize("B,T,cin,cout,context,bn,need_dx,seed", LAYER_CASES)
def test_layer_forward_and_backward(B, T, cin, cout, context, bn, need_dx, seed):
    case = make_case(B, T, cin, cout, context, bn, seed)
    check_layer(case, context, run_layer(case, context, need_dx), need_dx)


EDGE_CASES = [
    (1, 30, 20, 72, CTX[0], 21),                     # B = 1
    (40, 5, 20, 72, CTX[0], 22),                     # T' = 1 (40 utterances: over a handful of rows the BatchNorm backward
                                                     # is a difference of nearly equal numbers, in any fp32 arithmetic)
    (3, 8, 24, 40, CTX[2], 23),                      # T' = 2 with [-3, 0, 3]: a dx row gets one tap (rows 2 and 5: none)
] + [(1, n, 20, 72, [0], 30 + i) for i, n in enumerate((127, 128, 129, 255, 256, 257))] \
  + [(1, n + 4, 20, 72, CTX[1], 40 + i) for i, n in enumerate((255, 256, 257, 513))]
# N around the 128-row tile of the products and around 256 rows, which is both the chunk of the column sums and the row count
# at which dW gets a second slice (257 rows: slices of 144 and 113; 513: three slices)


@pytest.mark.parametrize("B,T,cin,cout,context,seed", EDGE_CASES)
def test_layer_edges(B, T, cin, cout, context, seed):
    case = make_case(B, T, cin, cout, context, True, seed)
    got = run_layer(case, context)
    check_layer(case, context, got)
    if context == CTX[2] and T == 8:                # dx[b, q] = dz[b, q - off] W_tap for the one tap that reaches q, if any
        dz = train_ref.layer_backward(case["dy"].double(), case["x"].double(), got["z"].double(), got["z"] > 0,
                                      case["W"].double(), context, case["gamma"].double(), got["mean"].double(),
                                      got["var"].double())["dz"]
        for q in range(8):
            taps = [(i, q - 3 * i) for i in range(3) if 0 <= q - 3 * i < 2]
            if not taps:
                assert q in (2, 5) and (got["dx"][:, q] == 0).all()
                continue
            (tap, p), = taps
            assert_parity(got["dx"][:, q], dz[:, p] @ case["W"].double()[:, tap * cin:(tap + 1) * cin], what=f"dx row {q}")


def test_dead_and_offset_channels():
    """A channel that is never on (bias -1e3): y = beta, its dW row, db and dgamma exactly 0, dbeta = sum dy.  A channel with
    bias +100: mean^2 = 1e4 var, the cancellation case for the variance (checked at the common bar by check_layer)."""
    B, T, cin, cout, context = 3, 104, 20, 72, CTX[1]
    dead, big = 5, 9
    case = make_case(B, T, cin, cout, context, True, 50, bias_edit={dead: -1e3, big: 100.0})
    got = run_layer(case, context)
    f, r = check_layer(case, context, got, edited=(dead, big))
    assert float(f["mean"][big]) ** 2 > 1e3 * float(f["var"][big])
    assert (got["z"][..., dead] == 0).all() and got["mean"][dead] == 0 and got["var"][dead] == 0
    assert (got["y"][..., dead] == case["beta"][dead]).all()
    assert (got["dW"][dead] == 0).all() and got["db"][dead] == 0 and got["dgamma"][dead] == 0
    want = case["dy"][..., dead].double().sum()
    assert abs(float(got["dbeta"][dead]) - float(want)) <= 1e-4 * float(case["dy"][..., dead].abs().sum())


def test_autograd_function_and_buffers():
    """tdnn_layer_train on a TdnnLayer's own parameters: gradients reach x and the five parameters, the BatchNorm buffers
    move as nn.BatchNorm1d moves them in training mode (momentum 0.1, unbiased variance, the counter)."""
    import xvector_amd as xa
    torch.manual_seed(0)
    layer = xa.TdnnLayer(20, 72, CTX[1]).to(DEV)
    with torch.no_grad():
        layer.norm.running_mean.normal_()
        layer.norm.running_var.uniform_(0.5, 2.0)
    twin = copy.deepcopy(layer).double().cpu()
    x = torch.randn(3, 30, 20, device=DEV, requires_grad=True)
    dy = torch.randn(3, 26, 72, device=DEV)
    y = xa.tdnn_layer_train(x, layer)
    y.backward(dy)
    x64 = x.detach().cpu().double().requires_grad_()
    y64 = train_ref.layer_autograd(x64, twin.linear.weight, twin.linear.bias, CTX[1], twin.norm.weight, twin.norm.bias)
    twin.norm.train()
    twin.norm(torch.relu(torch.nn.functional.linear(train_ref.gather(x64, CTX[1]), twin.linear.weight,
                                                    twin.linear.bias)).transpose(1, 2))
    y64.backward(dy.cpu().double())
    assert_parity(y.detach(), y64.detach(), what="y")
    assert_parity(x.grad, x64.grad, what="dx")
    for (name, p), (_, q) in zip(layer.named_parameters(), twin.named_parameters()):
        assert_parity(p.grad, q.grad, what="d " + name)
    assert_parity(layer.norm.running_mean, twin.norm.running_mean, what="running_mean")
    assert_parity(layer.norm.running_var, twin.norm.running_var, what="running_var")
    assert int(layer.norm.num_batches_tracked) == int(twin.norm.num_batches_tracked) == 1


# ---------------------------------------------------------------- the whole step
@pytest.fixture(scope="module")
def g10():
    return load_golden("g10_train.npz")


def fixture_model(g, synth):
    import xvector_amd as xa
    kw = {k: int(g[k]) for k in KW}
    m = xa.XVectorModel(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict(seed=int(g["seed_w"]), **kw).items()})
    return m.to(DEV)


def fixture_batch(g):
    B = int(g["B"])
    return (torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["labels"]).to(DEV), [f"id{i}" for i in range(B)])


def test_training_step_matches_the_reference(g10, synth):
    import xvector_amd as xa
    model = fixture_model(g10, synth)
    out = xa.XVectorTrainer(model).training_step(fixture_batch(g10), 0)
    assert sorted(out) == ["loss", "train_id", "train_labels", "train_preds"]
    assert out["train_preds"].shape == (int(g10["B"]), int(g10["num_classes"])) and out["train_id"] == fixture_batch(g10)[2]
    out["loss"].backward()
    print(f"[train] loss {out['loss'].item():.9f} fixture {float(g10['loss']):.9f}")
    assert abs(out["loss"].item() - float(g10["loss"])) <= 1e-4 * float(g10["loss"])
    check_grads(g10, {k: p.grad for k, p in model.named_parameters()}, 1e-4, "step")
    check_buffers(g10, model.state_dict(), 1e-4, "step")


def test_adam_losses_of_steps_two_and_three(g10, synth):
    import xvector_amd as xa
    trainer = xa.XVectorTrainer(fixture_model(g10, synth))
    batch = fixture_batch(g10)
    losses = np.array([float(trainer.step(batch)) for _ in range(3)])
    dev = np.abs(losses - g10["adam_losses"]) / g10["adam_losses"]
    print(f"[train] adam losses {losses.tolist()} relative deviation {dev.tolist()} bound {ADAM_LOSS_BOUND:.3e}")
    assert dev[0] <= 1e-4
    assert dev[1:].max() <= ADAM_LOSS_BOUND, dev


def test_one_step_twice_is_bit_identical(g10, synth):
    import xvector_amd as xa
    results = []
    for _ in range(2):
        model = fixture_model(g10, synth)
        trainer = xa.XVectorTrainer(model)
        loss = trainer.step(fixture_batch(g10))
        results.append([loss.cpu()] + [v.detach().cpu() for v in model.state_dict().values()])
    assert len(results[0]) == len(results[1]) > 20
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_extraction_after_a_step_uses_the_new_weights(g10, synth):
    import xvector_amd as xa
    model = fixture_model(g10, synth).eval()
    x = torch.from_numpy(synth.make_mfcc(3, 40, seed=61))
    before = model.extract_x_vec(x.to(DEV)).cpu()
    trainer = xa.XVectorTrainer(model)
    for _ in range(3):
        trainer.step(fixture_batch(g10))
    val = trainer.validation_step(fixture_batch(g10))
    assert sorted(val) == ["loss", "val_id", "val_labels", "val_preds"] and not val["loss"].requires_grad
    assert not model.training
    after = model.extract_x_vec(x.to(DEV)).cpu()
    with torch.no_grad():
        ref = oracle.extract_x_vec(x, float_params({k: v.detach().cpu() for k, v in model.state_dict().items()}))
        ref_logits = oracle.forward(torch.from_numpy(g10["x"]), float_params({k: v.detach().cpu() for k, v in model.state_dict().items()}))
    assert_parity(after, ref, what="x-vectors after three steps")
    assert_parity(val["val_preds"], ref_logits, what="validation logits")
    assert ((after - before).norm(dim=1) / before.norm(dim=1)).min() > 1e-3       # the steps did move them


def test_checkpoint_round_trip(g10, synth, tmp_path):
    import xvector_amd as xa
    model = fixture_model(g10, synth)
    model.x_vec_extract_layer = 7
    trainer = xa.XVectorTrainer(model)
    trainer.step(fixture_batch(g10))
    path = str(tmp_path / "last.ckpt")
    trainer.save_checkpoint(path)
    ckpt = torch.load(path, weights_only=False)
    assert sorted(ckpt) == ["hyper_parameters", "state_dict"]
    back = xa.XVectorModel.load_from_checkpoint(path)
    assert back.x_vec_extract_layer == 7 and back.hparams == model.hparams and back.learning_rate == model.learning_rate
    sd, sd2 = model.state_dict(), back.state_dict()
    assert list(sd) == list(sd2)
    for k in sd:
        assert torch.equal(sd[k].cpu(), sd2[k]), k


def test_refusals_and_the_unchanged_model(g10, synth):
    import xvector_amd as xa
    model = fixture_model(g10, synth)
    x = fixture_batch(g10)[0]
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        model(x)
    out = xa.XVectorTrainer(model).training_step(fixture_batch(g10))        # the trainer does not look at model.training
    assert out["loss"].requires_grad and model.training
    model.eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        xa.XVectorTrainer(model).logits(x.cpu())
    kw = {k: int(g10[k]) for k in KW}
    with pytest.raises(RuntimeError, match="dropout_p"):
        xa.XVectorTrainer(xa.XVectorModel(dropout_p=0.2, **kw).to(DEV))
    with pytest.raises(RuntimeError, match="fp32 only"):
        xa.XVectorTrainer(xa.XVectorModel(precision="bf16x3", **kw).to(DEV))
    with pytest.raises(ValueError, match="T=15"):
        xa.XVectorTrainer(model).logits(x[:, :15])


def test_thirty_steps_halve_the_loss(g10, synth):
    import xvector_amd as xa
    trainer = xa.XVectorTrainer(fixture_model(g10, synth))
    x = torch.from_numpy(synth.make_mfcc(8, 40, seed=71)).to(DEV)
    labels = torch.from_numpy(np.random.default_rng(72).integers(0, int(g10["num_classes"]), 8)).to(DEV)
    batch = (x, labels, list(range(8)))
    losses = [float(trainer.step(batch)) for _ in range(30)]
    print(f"[train] loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
