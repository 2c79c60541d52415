"""Dropout in the training layers on the GPU (include/xvec_train.h, "Dropout"; csrc/tdnn_train_dropout.hip; xvector_amd.train with
dropout_seed=) against tests/train_dropout_ref.py in fp64 on the same fp32 inputs, by the method and at the bar of
tests/test_train_gpu.py: assert_parity at 1e-4; every output and the workspace in NaN-poisoned windows of exactly the stated size
between guards; the backward of the reference on the GPU's own [z > 0], whose difference from the reference's own pattern
(keep & pre > 0, keep from the numpy restatement of the generator) is counted against the pre-activations within 1e-4 mean|pre| of
zero -- a share that itself must stay at or below 2e-4.

Sizes: the layers as the model runs them, widths that are no multiple of 4 (the element-wise loaders), one past the 128 x 128
tile in both widths, and N one past the 128-row tile and the 256-row chunk with N no multiple of 4 (the last Philox call of a
column is used in part)."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import train_dropout_ref as dref
import train_ragged_ref as rref
import train_ref
from conftest import assert_parity
from test_train_gpu import Window, make_case
from test_train_gpu import run_layer as run_plain_layer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTX = train_ref.CONTEXTS
NAN = float("nan")
SEED, STREAM = (0xC0FFEE << 32) | 0x12345678, (7 << 32) | 9          # both words of seed and stream in use


def run_layer(case, context, p, lengths=None, need_dx=True, seed=SEED, stream=STREAM, eps=train_ref.EPS):
    """The two *_dropout calls on one case (lengths=None: the fixed-length form), every output in a guarded window, the workspace
    of exactly the queried size between two guards and poisoned before each call.  Returns {name: cpu tensor}."""
    from xvector_amd import hip
    bn = "gamma" in case
    d = {k: v.to(DEV).contiguous() for k, v in case.items()}
    nb, nt, cin = case["x"].shape
    cout = case["W"].shape[0]
    tp = case["dy"].shape[1]
    carr = (C.c_int32 * len(context))(*context)
    need = hip.lib.xvec_tdnn_train_workspace_bytes(nb, nt, cin, cout, carr, len(context))
    assert need > 0 and need % 256 == 0
    wsbuf = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = wsbuf[256: 256 + need]
    ws.view(torch.float32).fill_(NAN)
    out = {"z": Window(nb, tp, cout), "dW": Window(cout, cin * len(context)), "db": Window(cout)}
    if bn:
        out.update(y=Window(nb, tp, cout), mean=Window(cout), var=Window(cout), dgamma=Window(cout), dbeta=Window(cout))
    if need_dx:
        out["dx"] = Window(nb, nt, cin)
    ptr = lambda name: out[name].ptr() if name in out else None
    dp = lambda name: d[name].data_ptr() if name in d else None
    ldev = None if lengths is None else torch.tensor(lengths, dtype=torch.int32).to(DEV)
    lp = None if ldev is None else ldev.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    rc = hip.lib.xvec_tdnn_train_forward_dropout(dp("x"), nb, nt, cin, dp("W"), dp("b"), cout, carr, len(context), dp("gamma"),
                                                 dp("beta"), eps, ptr("z"), ptr("mean"), ptr("var"), ptr("y"), ws.data_ptr(), need, s,
                                                 lp, p, seed, stream)
    assert rc == 0, hip.lib.xvec_train_last_error().decode()
    ws.view(torch.float32).fill_(NAN)          # the backward may rely on nothing the forward left there
    rc = hip.lib.xvec_tdnn_train_backward_dropout(dp("dy"), dp("x"), ptr("z"), nb, nt, cin, dp("W"), cout, carr, len(context),
                                                  dp("gamma"), ptr("mean"), ptr("var"), eps, ptr("dx"), ptr("dW"), ptr("db"),
                                                  ptr("dgamma"), ptr("dbeta"), ws.data_ptr(), need, s, lp, p)
    assert rc == 0, hip.lib.xvec_train_last_error().decode()
    torch.cuda.synchronize()
    assert (wsbuf[:256] == 0xA5).all() and (wsbuf[-256:] == 0xA5).all(), "workspace guard overwritten"
    return {k: w.check(k) for k, w in out.items()}


def keep_of(case, p, seed=SEED, stream=STREAM):
    nb, tp, cout = case["dy"].shape
    return torch.from_numpy(dref.keep_mask(nb * tp, cout, p, seed, stream)).view(nb, tp, cout)


def check_flips(got_z, pre, keep, valid=None):
    """The zero pattern of z is ~(keep & pre > 0) outside the near-zero set: flips <= near-zero pre-activations, whose share is
    itself <= 2e-4.  `valid`: the rows that count (a ragged case)."""
    valid = torch.ones_like(keep) if valid is None else valid
    near = (pre.abs() <= 1e-4 * pre[valid].abs().mean()) & valid
    flips = int((((got_z > 0) != (keep & (pre > 0))) & valid).sum())
    share = float(near.sum()) / float(valid.sum())
    print(f"[dropout] mask: {flips} flips, {int(near.sum())} of {int(valid.sum())} pre-activations near zero ({share:.2e}); "
          f"dropped share {1.0 - float(keep[valid].double().mean()):.4f}")
    assert share <= 2e-4, share
    assert flips <= int(near.sum()), (flips, int(near.sum()))
    assert int((((got_z > 0) != (keep & (pre > 0))) & valid & ~near).sum()) == 0


def check_layer(case, context, p, got, need_dx=True, eps=train_ref.EPS):
    c64 = {k: v.double() for k, v in case.items()}
    bn = "gamma" in case
    keep = keep_of(case, p)
    f = dref.layer_forward(c64["x"], c64["W"], c64["b"], context, keep, p, c64.get("gamma"), c64.get("beta"), eps)
    check_flips(got["z"], f["pre"], keep)
    assert (got["z"][~keep] == 0).all()                      # a dropped element is exactly 0
    assert_parity(got["z"], f["z"], what="z")
    if bn:
        assert_parity(got["y"], f["y"], what="y")
        assert_parity(got["mean"], f["mean"], what="batch_mean")
        assert_parity(1.0 / torch.sqrt(got["var"].double() + eps), f["invstd"], what="1/sqrt(var+eps)")
    r = dref.layer_backward(c64["dy"], c64["x"], f["z"], got["z"] > 0, c64["W"], context, p, c64.get("gamma"), f.get("mean"),
                            f.get("var"), eps)
    for name in ["dW", "db"] + (["dgamma", "dbeta"] if bn else []) + (["dx"] if need_dx else []):
        assert_parity(got[name], r[name], what=name)
    assert ("dx" in got) == need_dx


LAYER_CASES = [
    # B, T, Cin, Cout, context, BatchNorm, dx, seed (those of tests/test_train_gpu.py where the case is one of its own)
    (3, 40, 512, 512, CTX[1], True, True, 2),
    (5, 33, 24, 512, CTX[0], True, False, 1),            # layer 1 as the model runs it: no dx
    (3, 40, 512, 1500, CTX[4], False, True, 7),          # no BatchNorm
    (2, 37, 7, 13, CTX[0], True, True, 10),              # widths that are no multiple of 4: the element-wise loaders
    (2, 150, 130, 129, [-4, -1, 0, 3], True, True, 12),  # one past the tile in both widths, an uneven context
    (1, 129 + 4, 20, 72, CTX[1], True, True, 60),        # N = 129: past the 128-row tile, the last row quad holds one row
    (1, 257 + 4, 20, 72, CTX[1], True, True, 42),        # N = 257: past the 256-row chunk and into a second dW slice
]


@functools.lru_cache(maxsize=None)
def layer_case(i):
    B, T, cin, cout, context, bn, _, seed = LAYER_CASES[i]
    return make_case(B, T, cin, cout, context, bn, seed)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("i", range(len(LAYER_CASES)))
def test_layer_forward_and_backward(i, p):
    _, _, _, _, context, _, need_dx, _ = LAYER_CASES[i]
    case = layer_case(i)
    check_layer(case, context, p, run_layer(case, context, p, need_dx=need_dx), need_dx)


# ---------------------------------------------------------------- bit-identity
@pytest.mark.parametrize("i", [0, 2, 3, 6])
def test_p_zero_is_bit_identical_to_the_calls_without_dropout(i):
    _, _, _, _, context, _, need_dx, _ = LAYER_CASES[i]
    case = layer_case(i)
    old = run_plain_layer(case, context, need_dx)
    new = run_layer(case, context, 0.0, need_dx=need_dx)
    assert sorted(old) == sorted(new)
    for k in old:
        assert torch.equal(old[k], new[k]), k


@pytest.mark.parametrize("i", [0, 3, 4, 6])
def test_ragged_form_with_every_length_T_and_a_second_run_are_bit_identical(i):
    B, T, _, _, context, _, need_dx, _ = LAYER_CASES[i]
    case = layer_case(i)
    fixed = run_layer(case, context, 0.1, need_dx=need_dx)
    ragged = run_layer(case, context, 0.1, [T] * B, need_dx=need_dx)
    again = run_layer(case, context, 0.1, need_dx=need_dx)
    for k in fixed:
        assert torch.equal(fixed[k], ragged[k]), k
        assert torch.equal(fixed[k], again[k]), k
    other = run_layer(case, context, 0.1, need_dx=need_dx, stream=STREAM + 1)
    assert not torch.equal(fixed["z"], other["z"])


# ---------------------------------------------------------------- ragged
RAGGED = (4, 40, 20, 72, CTX[1], [40, 17, 5, 33], 70)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_ragged_layer_with_poisoned_padding(p):
    """The mask of a valid row is that of its PADDED index; invalid rows are exactly 0; parity on the valid rows against the
    valid rows alone as one BatchNorm batch.  The reference backward is autograd through pre * M * scale with M = the GPU's own
    [z > 0] on the valid rows: linear in what it differentiates, as train_ref.layer_backward is in its mask."""
    B, T, cin, cout, context, lengths, seed = RAGGED
    case = make_case(B, T, cin, cout, context, True, seed)
    span = rref.span_of(context)
    tp = T - span
    counts = rref.valid_rows(lengths, T, context)
    assert counts == [36, 13, 1, 29]
    for b, (l, v) in enumerate(zip(lengths, counts)):
        case["x"][b, l:] = NAN
        case["dy"][b, v:] = NAN
    got = run_layer(case, context, p, lengths)
    keep = keep_of(case, p)
    valid = (torch.arange(tp)[None, :] < torch.tensor(counts)[:, None])[:, :, None].expand(B, tp, cout)
    c64 = {k: v.double() for k, v in case.items()}
    names = ["x", "W", "b", "gamma", "beta"]
    leaves = {k: c64[k].clone().requires_grad_(True) for k in names}
    rows = torch.cat([train_ref.gather(x[None], context)[0] for x in rref.cut(leaves["x"], lengths, span + 1)], 0)
    pre = rows @ leaves["W"].T + leaves["b"]
    pre_padded = torch.zeros(B, tp, cout, dtype=torch.float64)
    pre_padded[valid] = pre.detach().reshape(-1)
    check_flips(got["z"], pre_padded, keep, valid)
    sel = lambda t: t[valid].view(-1, cout)
    z = torch.where(sel(keep), pre.detach().clamp_min(0) * dref.scale(p), torch.zeros_like(pre))
    mean, var = z.mean(0), z.var(0, unbiased=False)
    y = c64["gamma"] * (z - mean) / torch.sqrt(var + train_ref.EPS) + c64["beta"]
    assert_parity(sel(got["z"]), z, what="z")
    assert_parity(sel(got["y"]), y, what="y")
    assert_parity(got["mean"], mean, what="batch_mean")
    assert_parity(1.0 / torch.sqrt(got["var"].double() + train_ref.EPS), 1.0 / torch.sqrt(var + train_ref.EPS), what="1/sqrt(var+eps)")
    z_lin = pre * sel(got["z"] > 0).double() * dref.scale(p)
    y_lin = torch.nn.functional.batch_norm(z_lin, None, None, leaves["gamma"], leaves["beta"], True, 0.1, train_ref.EPS)
    grads = dict(zip(("dx", "dW", "db", "dgamma", "dbeta"), torch.autograd.grad(y_lin, [leaves[k] for k in names], sel(c64["dy"]))))
    for name, want in grads.items():
        assert_parity(got[name], want, what=name)
    for b, (l, v) in enumerate(zip(lengths, counts)):
        assert (got["z"][b, v:] == 0).all() and (got["y"][b, v:] == 0).all(), f"rows of utterance {b} past {v}"
        assert (got["dx"][b, l:] == 0).all(), f"dx rows of utterance {b} past its length"
    assert (got["z"][~keep] == 0).all()


# ---------------------------------------------------------------- the autograd function and the whole step
def test_autograd_function_and_buffers():
    """tdnn_layer_train with dropout=(seed, stream) on a TdnnLayer's own parameters against autograd with the mask injected; the
    BatchNorm buffers move with the post-dropout batch statistics."""
    import xvector_amd as xa
    torch.manual_seed(0)
    p = 0.2
    layer = xa.TdnnLayer(20, 72, CTX[1], dropout_p=p).to(DEV)
    twin = copy.deepcopy(layer).double().cpu()
    x = torch.randn(3, 30, 20, device=DEV, requires_grad=True)
    dy = torch.randn(3, 26, 72, device=DEV)
    with pytest.raises(RuntimeError, match="dropout="):
        xa.tdnn_layer_train(x, layer)
    y = xa.tdnn_layer_train(x, layer, dropout=(SEED, STREAM))
    y.backward(dy)
    keep = torch.from_numpy(dref.keep_mask(3 * 26, 72, p, SEED, STREAM)).view(3, 26, 72)
    x64 = x.detach().cpu().double().requires_grad_()
    y64 = dref.layer_autograd(x64, twin.linear.weight, twin.linear.bias, CTX[1], keep, p, twin.norm.weight, twin.norm.bias)
    twin.norm.train()
    with torch.no_grad():
        f = dref.layer_forward(x64, twin.linear.weight, twin.linear.bias, CTX[1], keep, p)
        twin.norm(f["z"].transpose(1, 2))
    y64.backward(dy.cpu().double())
    assert_parity(y.detach(), y64.detach(), what="y")
    assert_parity(x.grad, x64.grad, what="dx")
    for (name, q), (_, q64) in zip(layer.named_parameters(), twin.named_parameters()):
        assert_parity(q.grad, q64.grad, what="d " + name)
    assert_parity(layer.norm.running_mean, twin.norm.running_mean, what="running_mean")
    assert_parity(layer.norm.running_var, twin.norm.running_var, what="running_var")
    assert int(layer.norm.num_batches_tracked) == 1


KW = dict(hidden_size=32, num_classes=5, x_vector_size=8)
P_STEP, STEP_SEED, B_STEP, T_STEP = 0.2, 23, 6, 40
TRAINER_SEED = (5 << 32) | 77


def step_model(synth, p=P_STEP):
    import xvector_amd as xa
    m = xa.XVectorModel(dropout_p=p, **KW)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict(seed=STEP_SEED, input_size=24, **KW).items()})
    return m.to(DEV)


def step_batch(synth):
    x = torch.from_numpy(synth.make_mfcc(B_STEP, T_STEP, seed=STEP_SEED + 1))
    return x.to(DEV), torch.tensor([0, 3, 1, 4, 2, 3]).to(DEV), list(range(B_STEP))


@pytest.fixture(scope="module")
def step_oracle(synth):
    """Two fp64 steps' losses and gradients with the masks of steps 0 and 1 injected, on the SAME weights (no optimizer)."""
    x, labels, _ = step_batch(synth)
    out = []
    for k in (0, 1):
        sd = train_ref.cast_state(synth.make_state_dict(seed=STEP_SEED, input_size=24, **KW), torch.float64)
        loss, grads = dref.training_step(sd, x.cpu().double(), labels.cpu(), P_STEP, TRAINER_SEED, k)
        out.append({"loss": float(loss), "grads": grads, "sd": sd})
    return out


@pytest.mark.parametrize("tail", ["torch", "hip"])
def test_whole_step_matches_autograd_with_injected_masks(synth, step_oracle, tail):
    import xvector_amd as xa
    for k in (0, 1):                                    # step 1 on fresh weights: the streams are 8 k + i
        model = step_model(synth)
        tr = xa.XVectorTrainer(model, tail=tail, dropout_seed=TRAINER_SEED)
        tr.load_dropout_state({"seed": TRAINER_SEED, "step": k})
        out = tr.training_step(step_batch(synth), 0)
        assert tr.dropout_state() == {"seed": TRAINER_SEED, "step": k + 1}
        out["loss"].backward()
        want = step_oracle[k]
        print(f"[dropout] {tail} step {k} loss {out['loss'].item():.9f} oracle {want['loss']:.9f}")
        assert abs(out["loss"].item() - want["loss"]) <= 1e-4 * want["loss"]
        grads = {name: q.grad for name, q in model.named_parameters()}
        assert sorted(grads) == sorted(want["grads"]) and len(grads) == 26
        for name, g in grads.items():
            assert_parity(g, want["grads"][name], what=f"{tail} step {k} d {name}")
        n = 0
        for name, v in model.state_dict().items():
            if "running" in name:
                assert_parity(v, want["sd"][name], what=f"{tail} {name}")
                n += 1
        assert n == 10
    assert abs(step_oracle[0]["loss"] - step_oracle[1]["loss"]) > 1e-3 * step_oracle[0]["loss"]      # the two steps' masks differ


def run_steps(synth, tail, seed, n, lengths=None, resume_after=None, tmp_path=None):
    """The losses of n optimizer steps; `resume_after`: after that many steps the run goes through a checkpoint into a new
    trainer (weights and buffers from the file, the optimizer's state by its state_dict, the dropout state from the file)."""
    import xvector_amd as xa
    tr = xa.XVectorTrainer(step_model(synth), tail=tail, dropout_seed=seed)
    batch = step_batch(synth)
    losses = []
    for k in range(n):
        if k == resume_after:
            path = str(tmp_path / f"{tail}.ckpt")
            tr.save_checkpoint(path)
            ckpt = torch.load(path, weights_only=False)
            assert ckpt["xvec_dropout"] == {"seed": seed, "step": k}
            new = xa.XVectorTrainer(xa.XVectorModel.load_from_checkpoint(path).to(DEV), tail=tail, dropout_seed=0)
            new.load_dropout_state(ckpt["xvec_dropout"])
            new.optimizer = new.configure_optimizers()
            new.optimizer.load_state_dict(tr.optimizer.state_dict())
            tr = new
        losses.append(tr.step(batch, lengths=lengths).cpu())
    return losses


@pytest.mark.parametrize("tail", ["torch", "hip"])
def test_runs_repeat_bit_for_bit_and_resume_from_a_checkpoint(synth, tail, tmp_path):
    a = run_steps(synth, tail, TRAINER_SEED, 3)
    b = run_steps(synth, tail, TRAINER_SEED, 3)
    c = run_steps(synth, tail, TRAINER_SEED + 1, 1)
    d = run_steps(synth, tail, TRAINER_SEED, 3, resume_after=2, tmp_path=tmp_path)
    e = run_steps(synth, tail, TRAINER_SEED, 1, lengths=[T_STEP] * B_STEP)
    print(f"[dropout] {tail} losses {[float(v) for v in a]}; another seed {float(c[0])}")
    assert all(torch.isfinite(v) for v in a)
    for u, v, w in zip(a, b, d):
        assert torch.equal(u, v) and torch.equal(u, w)
    assert not torch.equal(a[0], c[0])
    assert torch.equal(a[0], e[0])                     # lengths= with every length T: the ragged calls, the same masks


def test_a_seed_without_dropout_changes_nothing(synth):
    import xvector_amd as xa
    losses = []
    for seed in (None, 5):
        tr = xa.XVectorTrainer(step_model(synth, p=0.0), dropout_seed=seed)
        losses.append([tr.step(step_batch(synth)).cpu() for _ in range(2)])
    assert all(torch.equal(u, v) for u, v in zip(*losses))
