"""CPU-only checks of the training step's tail (include/xvec_train.h: xvec_train_tail_*, xvec_adam_step; xvector_amd.train:
tail="hip", DeviceAdam): tests/train_tail_ref.py -- the fp64 restatement the GPU tests compare against -- equals autograd over
the reference's own op sequence and torch.optim.Adam, the new calls are exported and refuse bad arguments before a device is
touched, and the Python surface refuses what it cannot do."""
import ctypes as C

import pytest
import torch

import train_tail_ref as ref

FAKE = C.c_void_p(0x1000)      # never dereferenced: every check below returns before the device is touched


def _case64(shape, seed):
    case = ref.make_case(*shape, seed)
    return {k: (v.double() if v.is_floating_point() else v) for k, v in case.items()}


def _assert_close(got, want, tol, what):
    scale = max(float(want.abs().max()), 1e-300)
    err = float((got - want).abs().max()) / scale
    assert err <= tol, f"{what}: {err:.3e} > {tol}"


PARAMS = ("y5", "W6", "b6", "W7", "b7", "Wo", "bo")
GRADS = ("dy5", "dW6", "db6", "dW7", "db7", "dWo", "dbo")


def _formula_against_autograd(c):
    leaves = [c[k].clone().requires_grad_() for k in PARAMS]
    loss = ref.tail_autograd(*leaves, c["labels"])
    want = dict(zip(GRADS, torch.autograd.grad(loss, leaves)))
    f = ref.tail_forward(*(c[k] for k in PARAMS), c["labels"])
    _assert_close(f["loss"], loss.detach(), 1e-10, "loss")
    got = ref.tail_backward(torch.ones((), dtype=torch.float64), c["y5"], c["W6"], c["W7"], c["Wo"], c["labels"], f["pooled"],
                            f["a6"], f["a7"], f["logits"], f["pre6"] > 0, f["pre7"] > 0)
    for k in GRADS:
        _assert_close(got[k], want[k], 1e-10, k)
    return f, got, want


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_formula_form_equals_autograd_form(shape):
    _formula_against_autograd(_case64(shape, 1))


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_has_no_pre_activation_near_zero_in_the_small_cases(shape):
    """What the GPU tests' ReLU-mask rule needs of its inputs, a property of the reference alone: the share of pre-activations
    within 1e-4 mean|pre| of zero is 0 in the small shapes (one element would exceed the cap of 2e-4) and at most 1.2e-4 in
    the two large ones, at seeds 1, 2 and 3."""
    for seed in (1, 2, 3):
        c = _case64(shape, seed)
        f = ref.tail_forward(*(c[k] for k in PARAMS), c["labels"])
        for pre in (f["pre6"], f["pre7"]):
            near = int((pre.abs() <= 1e-4 * pre.abs().mean()).sum())
            assert near <= (1.2e-4 * pre.numel() if pre.numel() > 10000 else 0), (seed, near, pre.numel())


def test_constant_channel_has_zero_gradient_through_std():
    c = _case64((3, 7, 65, 33, 5), 2)
    c["y5"][:, :, 11] = 3.25
    c["y5"][1, :, 40] = -1e3
    f, got, want = _formula_against_autograd(c)
    assert (f["pooled"][:, 65 + 11] == 0).all() and f["pooled"][1, 65 + 40] == 0
    for name, g in (("formula", got["dy5"]), ("autograd", want["dy5"])):
        assert torch.isfinite(g).all(), name
        # only the mean's share is left, the same in every frame
        assert (g[:, :, 11] == g[:, :1, 11]).all() and (g[1, :, 40] == g[1, 0, 40]).all(), name
    assert torch.equal(got["dy5"][:, :, 11], (got["dpooled"][:, 11] / 7)[:, None].expand(3, 7))


def test_adam_formulas_match_three_steps_of_torch_adam():
    gen = torch.Generator().manual_seed(3)
    p0 = [torch.randn(n, dtype=torch.float64, generator=gen) for n in (1, 5, 1211)]
    grads = [[torch.randn(p.shape, dtype=torch.float64, generator=gen) * 10.0 ** (s - 1) for p in p0] for s in range(3)]
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    params = [p.clone().requires_grad_() for p in p0]
    opt = torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps)
    mine = [(p.clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in p0]
    for t in range(1, 4):
        for p, g in zip(params, grads[t - 1]):
            p.grad = g.clone()
        opt.step()
        mine = [ref.adam_step(p, g, m, v, lr, b1, b2, eps, t)[:3] for (p, m, v), g in zip(mine, grads[t - 1])]
        for i, ((p, m, v), q) in enumerate(zip(mine, params)):
            _assert_close(p, q.detach(), 1e-12, f"step {t} p[{i}]")
            _assert_close(m, opt.state[q]["exp_avg"], 1e-12, f"step {t} m[{i}]")
            _assert_close(v, opt.state[q]["exp_avg_sq"], 1e-12, f"step {t} v[{i}]")


# ---------------------------------------------------------------- argument checks through ctypes
def _forward(hip, y5=FAKE, B=2, Tp=5, c=8, h=8, k=3, labels=FAKE, loss=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = hip.lib.xvec_train_tail_workspace_bytes(B, Tp, c, h, k)
    return hip.lib.xvec_train_tail_forward(y5, B, Tp, c, FAKE, FAKE, h, FAKE, FAKE, FAKE, FAKE, k, labels, FAKE, FAKE, FAKE, FAKE,
                                           loss, ws, ws_bytes, None)


def _backward(hip, y5=FAKE, B=2, Tp=5, c=8, h=8, k=3, labels=FAKE, loss=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = hip.lib.xvec_train_tail_workspace_bytes(B, Tp, c, h, k)
    # `loss` stands for a required output here too: dWo
    return hip.lib.xvec_train_tail_backward(FAKE, y5, B, Tp, c, FAKE, h, FAKE, FAKE, k, labels, FAKE, FAKE, FAKE, FAKE, None, FAKE,
                                            FAKE, FAKE, FAKE, loss, FAKE, ws, ws_bytes, None)


def test_new_symbols_are_exported():
    from xvector_amd import hip
    for name in ("xvec_train_tail_workspace_bytes", "xvec_train_tail_forward", "xvec_train_tail_backward", "xvec_adam_step"):
        assert name in hip.EXPORTS and hasattr(hip.lib, name), name


@pytest.mark.parametrize("call", [_forward, _backward], ids=["forward", "backward"])
def test_argument_errors_return_before_the_device_is_touched(call):
    from xvector_amd import hip
    err = lambda: hip.lib.xvec_train_last_error().decode()
    need = hip.lib.xvec_train_tail_workspace_bytes(2, 5, 8, 8, 3)
    assert need > 0 and need % 256 == 0
    for kw in (dict(y5=None), dict(labels=None), dict(loss=None)):
        assert call(hip, **kw) == hip.ERR_ARG and "null pointer" in err(), kw
    assert call(hip, ws=None) == hip.ERR_ARG and "null pointer: workspace" in err()
    assert call(hip, Tp=1, ws_bytes=1 << 20) == hip.ERR_ARG and "Tp = 1" in err()
    assert call(hip, B=0, ws_bytes=1 << 20) == hip.ERR_ARG and "B = 0" in err()
    assert call(hip, k=0, ws_bytes=1 << 20) == hip.ERR_ARG and "K = 0" in err()
    assert call(hip, c=0, ws_bytes=1 << 20) == hip.ERR_ARG and "must be >= 1" in err()
    assert call(hip, ws_bytes=need - 1) == hip.ERR_ARG and err() == f"workspace too small: {need - 1} < {need} bytes"
    assert call(hip, B=1 << 20, ws_bytes=1 << 40) == hip.ERR_TOO_LARGE and "65535" in err()


def test_workspace_query_refuses_what_the_calls_refuse():
    from xvector_amd import hip
    q = hip.lib.xvec_train_tail_workspace_bytes
    assert q(2, 5, 8, 8, 3) > 0
    for bad in ((2, 1, 8, 8, 3), (0, 5, 8, 8, 3), (2, 5, 8, 8, 0), (2, 5, 0, 8, 3), (2, 5, 8, 0, 3), (1 << 20, 5, 8, 8, 3)):
        assert q(*bad) == 0, bad
    # one size serves both calls and grows with the batch and the widths
    assert q(256, 5, 64, 512, 1211) > q(128, 5, 64, 512, 1211)
    assert q(256, 5, 1500, 512, 1211) > q(256, 5, 64, 512, 1211)


def test_adam_argument_errors_return_before_the_device_is_touched():
    from xvector_amd import hip
    err = lambda: hip.lib.xvec_train_last_error().decode()
    tab = (C.c_void_p * 1)(0x1000)
    odd = (C.c_void_p * 1)(0x1002)
    null = (C.c_void_p * 1)(None)
    n = (C.c_int64 * 1)(5)
    call = lambda p=tab, g=tab, n_=n, count=1, b1=0.9, t=1: hip.lib.xvec_adam_step(p, g, tab, tab, n_, count, 1e-3, b1, 0.999, 1e-8,
                                                                                  t, None)
    assert call(p=None) == hip.ERR_ARG and "null pointer" in err()
    assert call(n_=None) == hip.ERR_ARG and "null pointer" in err()
    assert call(g=null) == hip.ERR_ARG and err() == "tensor 0: null pointer"
    assert call(p=odd) == hip.ERR_ARG and "4-byte aligned" in err()
    assert call(t=0) == hip.ERR_ARG and "starts at 1" in err()
    assert call(b1=1.0) == hip.ERR_ARG and "[0, 1)" in err()
    assert call(count=-1) == hip.ERR_ARG and "n_tensors = -1" in err()
    assert call(n_=(C.c_int64 * 1)(-2)) == hip.ERR_ARG and "length -2" in err()
    assert call(count=0) == hip.OK                       # nothing to do, nothing launched


# ---------------------------------------------------------------- the Python surface
KW = dict(hidden_size=32, num_classes=5, x_vector_size=8)


def test_trainer_refuses_an_unknown_tail():
    import xvector_amd as xa
    from xvector_amd.train import DeviceAdam
    with pytest.raises(ValueError, match="bogus"):
        xa.XVectorTrainer(xa.XVectorModel(**KW), tail="bogus")
    tr = xa.XVectorTrainer(xa.XVectorModel(**KW))
    assert tr.tail == "torch" and isinstance(tr.configure_optimizers(), torch.optim.Adam)
    tr = xa.XVectorTrainer(xa.XVectorModel(**KW), tail="hip")
    with pytest.raises(RuntimeError, match="no CPU path"):
        tr.training_step((torch.zeros(2, 40, 24), torch.zeros(2, dtype=torch.long), ["a", "b"]))
    opt = tr.configure_optimizers()
    assert isinstance(opt, DeviceAdam) and opt.param_groups[0]["lr"] == tr.model.learning_rate
    assert len(opt.param_groups[0]["params"]) == 26


def test_device_adam_refusals():
    """No fallback: step() raises before anything is launched."""
    import xvector_amd as xa
    from xvector_amd.train import DeviceAdam
    assert xa.DeviceAdam is DeviceAdam
    with pytest.raises(ValueError, match="no parameters"):
        DeviceAdam([])
    with pytest.raises(ValueError, match="betas"):
        DeviceAdam([torch.zeros(4)], betas=(1.0, 0.999))
    with pytest.raises(RuntimeError, match="HIP device only"):
        DeviceAdam([torch.zeros(4, requires_grad=True)]).step()
    with pytest.raises(RuntimeError, match="fp32 only"):
        DeviceAdam([torch.zeros(4, dtype=torch.float64, requires_grad=True)]).step()


def test_device_adam_state_dict_has_torch_adams_layout():
    """`state` (empty before the first step) and one parameter group with torch.optim.Adam's own keys, the parameters as
    indices; a state in torch's layout loads."""
    from xvector_amd.train import DeviceAdam
    params = [torch.zeros(3, 2, requires_grad=True), torch.zeros(5, requires_grad=True)]
    kw = dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-7)
    want = torch.optim.Adam(params, **kw).state_dict()
    opt = DeviceAdam(params, **kw)
    got = opt.state_dict()
    assert sorted(got) == sorted(want) == ["param_groups", "state"]
    assert got["state"] == want["state"] == {}
    assert got["param_groups"] == want["param_groups"]
    opt.load_state_dict({"state": {1: {"step": torch.tensor(4.0), "exp_avg": torch.ones(5), "exp_avg_sq": torch.full((5,), 2.0)}},
                         "param_groups": want["param_groups"]})
    assert opt.state[1]["step"] == 4 and sorted(opt.state_dict()["state"][1]) == ["exp_avg", "exp_avg_sq", "step"]
    assert opt.param_groups[0]["lr"] == 2e-3 and opt.param_groups[0]["params"] is opt.params
    torch.optim.Adam(params, **kw).load_state_dict(opt.state_dict())         # ... and torch takes it back
    opt.zero_grad()
