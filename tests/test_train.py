"""CPU-only checks of the training path: tests/train_ref.py (the fp64 restatement the GPU tests compare against) reproduces
the reference's own training step (g10_train.npz: tests/golden/make_golden_train.py), its formula form equals its autograd
form, and the argument checks of the two new C-ABI calls (include/xvec_train.h) return before a device is touched, through an
error channel of their own."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_ref
from conftest import assert_parity, load_golden

KW = ("input_size", "hidden_size", "num_classes", "x_vector_size")


@pytest.fixture(scope="module")
def g10():
    return load_golden("g10_train.npz")


def fixture_state(g, synth, dtype):
    kw = {k: int(g[k]) for k in KW}
    return train_ref.cast_state(synth.make_state_dict(seed=int(g["seed_w"]), **kw), dtype)


def check_grads(g, grads, tol, what):
    """{parameter: gradient} against the fixture: whole tensors, or the stored rows and sums of the two large ones."""
    seen = 0
    for key in g.files:
        kind, _, name = key.partition("/")
        if kind == "grad":
            assert_parity(grads[name], g[key], tol=tol, what=f"{what} d {name}")
        elif kind == "grad_rows":
            got = torch.as_tensor(grads[name]).detach().cpu().double()
            assert_parity(got[g["grad_rows_idx/" + name].tolist()], g[key], tol=tol, what=f"{what} d {name} rows")
            assert_parity(got.sum(1), g["grad_rowsum/" + name], tol=tol, what=f"{what} d {name} row sums")
            assert_parity(got.sum(0), g["grad_colsum/" + name], tol=tol, what=f"{what} d {name} column sums")
        else:
            continue
        seen += 1
    assert seen == len(grads) == 26


def check_buffers(g, sd, tol, what):
    n = 0
    for key in g.files:
        if key.startswith("buf/"):
            name = key[4:]
            if name.endswith("num_batches_tracked"):
                assert int(sd[name]) == int(g[key]), name
            else:
                assert_parity(sd[name], g[key], tol=tol, what=f"{what} {name}")
            n += 1
    assert n == 15


def test_train_ref_reproduces_the_reference_step(g10, synth):
    sd = fixture_state(g10, synth, torch.float64)
    x, labels = torch.from_numpy(g10["x"]).double(), torch.from_numpy(g10["labels"])
    loss, grads = train_ref.training_step(sd, x, labels)
    assert abs(float(loss) - float(g10["loss"])) <= 1e-12 * float(g10["loss"])
    check_grads(g10, grads, 1e-10, "train_ref")
    check_buffers(g10, sd, 1e-12, "train_ref")


def test_train_ref_reproduces_the_reference_adam_losses(g10, synth):
    sd = fixture_state(g10, synth, torch.float64)
    x, labels = torch.from_numpy(g10["x"]).double(), torch.from_numpy(g10["labels"])
    losses = train_ref.adam_losses(sd, x, labels, 3, float(g10["lr"]))
    np.testing.assert_allclose(losses, g10["adam_losses"], rtol=1e-10)
    assert losses[2] < losses[1] < losses[0]


@pytest.mark.parametrize("bn", [True, False])
@pytest.mark.parametrize("context,cin,cout", [([-2, -1, 0, 1, 2], 6, 10), ([-3, 0, 3], 5, 7), ([0], 8, 3), ([-1, 0, 2], 4, 4)])
def test_formula_form_equals_autograd_form(context, cin, cout, bn):
    rng = np.random.default_rng(5)
    B, T = 3, 12
    t = lambda *s: torch.from_numpy(rng.standard_normal(s))
    x, W, b = t(B, T, cin).requires_grad_(), (0.3 * t(cout, len(context) * cin)).requires_grad_(), t(cout).requires_grad_()
    gamma, beta = ((1 + 0.2 * t(cout)).requires_grad_(), t(cout).requires_grad_()) if bn else (None, None)
    y = train_ref.layer_autograd(x, W, b, context, gamma, beta)
    dy = t(*y.shape)
    leaves = [x, W, b] + ([gamma, beta] if bn else [])
    want = dict(zip(("dx", "dW", "db", "dgamma", "dbeta"), torch.autograd.grad(y, leaves, dy)))
    with torch.no_grad():
        f = train_ref.layer_forward(x, W, b, context, gamma, beta)
        np.testing.assert_allclose(f["y"].numpy(), y.detach().numpy(), rtol=1e-11, atol=1e-12)
        got = train_ref.layer_backward(dy, x, f["z"], f["pre"] > 0, W, context, gamma, f.get("mean"), f.get("var"))
    for k, v in want.items():
        np.testing.assert_allclose(got[k].numpy(), v.numpy(), rtol=1e-9, atol=1e-11, err_msg=k)


# ---------------------------------------------------------------- argument checks through ctypes
FAKE = C.c_void_p(0x1000)      # never dereferenced: every check below returns before the device is touched
CTX5 = (C.c_int32 * 5)(-2, -1, 0, 1, 2)


def _forward(hip, x=FAKE, B=2, T=20, cin=24, W=FAKE, cout=32, ctx=CTX5, n_ctx=5, gamma=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = hip.lib.xvec_tdnn_train_workspace_bytes(B, T, cin, cout, ctx, n_ctx)
    return hip.lib.xvec_tdnn_train_forward(x, B, T, cin, W, FAKE, cout, ctx, n_ctx, gamma, FAKE, 1e-5, FAKE, FAKE, FAKE, FAKE,
                                           ws, ws_bytes, None)


def _backward(hip, dy=FAKE, B=2, T=20, cin=24, cout=32, ctx=CTX5, n_ctx=5, dW=FAKE, dgamma=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = hip.lib.xvec_tdnn_train_workspace_bytes(B, T, cin, cout, ctx, n_ctx)
    return hip.lib.xvec_tdnn_train_backward(dy, FAKE, FAKE, B, T, cin, FAKE, cout, ctx, n_ctx, FAKE, FAKE, FAKE, 1e-5, None, dW,
                                            FAKE, dgamma, FAKE, ws, ws_bytes, None)


@pytest.mark.parametrize("call", [_forward, _backward], ids=["forward", "backward"])
def test_argument_errors_return_before_the_device_is_touched(call):
    from xvector_amd import hip
    err = lambda: hip.lib.xvec_train_last_error().decode()
    need = hip.lib.xvec_tdnn_train_workspace_bytes(2, 20, 24, 32, CTX5, 5)
    assert need > 0
    first = dict(x=None) if call is _forward else dict(dy=None)
    assert call(hip, **first) == hip.ERR_ARG and "null pointer" in err()
    assert call(hip, ws=None) == hip.ERR_ARG and "null pointer: workspace" in err()
    assert call(hip, ctx=None) == hip.ERR_ARG and "null pointer: context_host" in err()
    if call is _forward:
        assert call(hip, W=None) == hip.ERR_ARG and "null pointer" in err()
    else:
        assert call(hip, dW=None) == hip.ERR_ARG and "null pointer" in err()
        assert call(hip, dgamma=None) == hip.ERR_ARG and "with gamma" in err()
    assert call(hip, T=4) == hip.ERR_ARG and err() == "T = 4 is not longer than the context span 4"
    assert call(hip, ctx=(C.c_int32 * 3)(-2, 0, 0), n_ctx=3) == hip.ERR_ARG and "not strictly increasing at entry 2" in err()
    assert call(hip, ctx=(C.c_int32 * 2)(1, -1), n_ctx=2) == hip.ERR_ARG and "not strictly increasing" in err()
    assert call(hip, n_ctx=0) == hip.ERR_ARG and "n_ctx = 0" in err()
    assert call(hip, cout=0) == hip.ERR_ARG and "must be >= 1" in err()
    assert call(hip, ws_bytes=need - 1) == hip.ERR_ARG and err() == f"workspace too small: {need - 1} < {need} bytes"
    assert call(hip, B=1 << 20, T=1 << 12, ws_bytes=1 << 40) == hip.ERR_TOO_LARGE and "row indices are int32" in err()
    assert call(hip, cin=1 << 30, cout=1 << 30, ws_bytes=1 << 40) == hip.ERR_TOO_LARGE and "column indices are int32" in err()


def test_workspace_query_refuses_what_the_calls_refuse():
    from xvector_amd import hip
    q = hip.lib.xvec_tdnn_train_workspace_bytes
    assert q(2, 20, 24, 32, CTX5, 5) > 0
    assert q(2, 4, 24, 32, CTX5, 5) == 0
    assert q(2, 20, 24, 32, None, 5) == 0
    assert q(2, 20, 24, 32, (C.c_int32 * 2)(0, 0), 2) == 0
    assert q(1 << 20, 1 << 12, 24, 32, CTX5, 5) == 0
    # one size serves both calls and grows with every dimension
    assert q(4, 20, 24, 32, CTX5, 5) > q(2, 20, 24, 32, CTX5, 5)
    assert q(2, 20, 24, 64, CTX5, 5) > q(2, 20, 24, 32, CTX5, 5)


def test_train_error_channel_is_separate():
    """The fifth channel next to the four of tests/test_error_channels.py: provoking it leaves theirs alone and theirs leave
    it alone, and another thread reads an empty text."""
    import threading
    from xvector_amd import hip
    from test_error_channels import _provokers
    others = _provokers(hip)
    for name, (provoke, last_error, want) in others.items():
        assert provoke() == hip.ERR_ARG, name
    assert _forward(hip, T=4) == hip.ERR_ARG
    mine = "T = 4 is not longer than the context span 4"
    assert hip.lib.xvec_train_last_error().decode() == mine
    assert mine not in [w for _, _, w in others.values()]
    for name, (_, last_error, want) in others.items():
        assert last_error().decode() == want, name
    for name, (provoke, _, _) in others.items():
        provoke()
        assert hip.lib.xvec_train_last_error().decode() == mine, name
    seen = []
    t = threading.Thread(target=lambda: seen.append(hip.lib.xvec_train_last_error().decode()))
    t.start()
    t.join()
    assert seen == [""]
    assert hip.last_error() == "" or "T = 4" not in hip.last_error()


def test_trainer_refuses_what_it_cannot_do(synth):
    import xvector_amd as xa
    kw = dict(hidden_size=32, num_classes=5, x_vector_size=8)
    with pytest.raises(RuntimeError, match="dropout_p"):
        xa.XVectorTrainer(xa.XVectorModel(dropout_p=0.1, **kw))
    with pytest.raises(RuntimeError, match="fp32 only"):
        xa.XVectorTrainer(xa.XVectorModel(precision="bf16", **kw))
    tr = xa.XVectorTrainer(xa.XVectorModel(**kw))
    with pytest.raises(RuntimeError, match="no CPU path"):
        tr.training_step((torch.zeros(2, 40, 24), torch.zeros(2, dtype=torch.long), ["a", "b"]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        xa.tdnn_layer_train(torch.zeros(2, 40, 24), tr.model.time_context_layers[0])
    assert isinstance(tr.configure_optimizers(), torch.optim.Adam)
    assert tr.configure_optimizers().param_groups[0]["lr"] == tr.model.learning_rate
