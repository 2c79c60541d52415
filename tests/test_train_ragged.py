"""CPU-only checks of ragged training (include/xvec_train.h, "Ragged batches"): tests/train_ragged_ref.py -- the fp64 oracle on
per-utterance slices that the GPU tests compare against -- equals tests/train_ref.py when every length is T; the four *_ragged
calls are exported, declared and bound; their argument checks return before a device is touched; XVectorTrainer refuses bad
lengths on the host; and the length-masked kernel instantiations (csrc/tdnn_train_ragged.hip, csrc/train_tail_ragged.hip),
compiled for gfx950 on the CPU, use no scratch and the product kernel's LDS of the unmasked form."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import train_ragged_ref as rref
import train_ref
from conftest import ROOT
from hipcc_support import kernel_resources, needs_hipcc
from test_train import CTX5, FAKE

RAGGED = ("xvec_tdnn_train_forward_ragged", "xvec_tdnn_train_backward_ragged", "xvec_train_tail_forward_ragged",
          "xvec_train_tail_backward_ragged")
KW = dict(hidden_size=32, num_classes=5, x_vector_size=8)


def small_state(synth, dtype=torch.float64):
    return train_ref.cast_state(synth.make_state_dict(seed=7, input_size=24, **KW), dtype)


def test_equal_lengths_reproduce_train_ref(synth):
    B, T = 4, 30
    x = torch.from_numpy(synth.make_mfcc(B, T, seed=11)).double()
    labels = torch.tensor([0, 3, 1, 4])
    a, b = small_state(synth), small_state(synth)
    np.testing.assert_allclose(rref.logits(a, x, [T] * B, update_buffers=False).detach().numpy(),
                               train_ref.logits(b, x, update_buffers=False).detach().numpy(), rtol=1e-10, atol=1e-12)
    loss_a, grads_a = rref.training_step(a, x, [T] * B, labels)
    loss_b, grads_b = train_ref.training_step(b, x, labels)
    assert abs(float(loss_a) - float(loss_b)) <= 1e-12 * float(loss_b)
    assert sorted(grads_a) == sorted(grads_b) and len(grads_a) == 26
    for k in grads_a:
        np.testing.assert_allclose(grads_a[k].numpy(), grads_b[k].numpy(), rtol=1e-8, atol=1e-12, err_msg=k)
    for k in a:
        if "running" in k or "num_batches" in k:
            np.testing.assert_allclose(a[k].numpy(), b[k].numpy(), rtol=1e-12, err_msg=k)


def test_oracle_ignores_the_padding(synth):
    """The oracle's own independence from the padding, NaN included, and its zeros: dx past the lengths, z and y on invalid rows."""
    rng = np.random.default_rng(3)
    ctx = train_ref.CONTEXTS[1]
    t = lambda *s: torch.from_numpy(rng.standard_normal(s))
    case = {"x": t(3, 12, 5), "W": 0.3 * t(7, 15), "b": t(7), "gamma": 1 + 0.2 * t(7), "beta": t(7), "dy": t(3, 8, 7)}
    lengths = [12, 5, 9]
    want = rref.layer(case, lengths, ctx)
    poisoned = {k: v.clone() for k, v in case.items()}
    for b, l in enumerate(lengths):
        poisoned["x"][b, l:] = float("nan")
        poisoned["dy"][b, l - 4:] = float("nan")
    got = rref.layer(poisoned, lengths, ctx)
    assert want["counts"] == [8, 1, 5]
    for k in ("z", "y", "mean", "var", "dx", "dW", "db", "dgamma", "dbeta"):
        assert torch.equal(got[k], want[k]), k
    assert (got["dx"][1, 5:] == 0).all() and (got["y"][1, 1:] == 0).all() and (got["z"][2, 5:] == 0).all()
    # an utterance with a length outside [span + 1, T] has no rows
    assert rref.layer(case, [12, 4, 13], ctx)["counts"] == [8, 0, 0]


def test_ragged_calls_are_exported_declared_and_bound():
    from xvector_amd import hip
    header = open(os.path.join(ROOT, "include", "xvec_train.h")).read()
    for name in RAGGED:
        assert name in hip.EXPORTS and hasattr(hip.lib, name), name
        assert f"int {name}(" in header, name
        assert getattr(hip.lib, name).argtypes[-1] is C.c_void_p          # the lengths come last: the old argument list, plus one


LEN = C.c_void_p(0x2000)       # never dereferenced either


def _forward(hip, x=FAKE, B=2, T=20, ws=FAKE, ws_bytes=None, lengths=LEN):
    if ws_bytes is None:
        ws_bytes = hip.lib.xvec_tdnn_train_workspace_bytes(B, T, 24, 32, CTX5, 5)
    return hip.lib.xvec_tdnn_train_forward_ragged(x, B, T, 24, FAKE, FAKE, 32, CTX5, 5, FAKE, FAKE, 1e-5, FAKE, FAKE, FAKE, FAKE,
                                                  ws, ws_bytes, None, lengths)


def _backward(hip, x=FAKE, B=2, T=20, ws=FAKE, ws_bytes=None, lengths=LEN):
    if ws_bytes is None:
        ws_bytes = hip.lib.xvec_tdnn_train_workspace_bytes(B, T, 24, 32, CTX5, 5)
    return hip.lib.xvec_tdnn_train_backward_ragged(x, FAKE, FAKE, B, T, 24, FAKE, 32, CTX5, 5, FAKE, FAKE, FAKE, 1e-5, None, FAKE,
                                                   FAKE, FAKE, FAKE, ws, ws_bytes, None, lengths)


@pytest.mark.parametrize("call", [_forward, _backward], ids=["forward", "backward"])
def test_layer_argument_errors_return_before_the_device_is_touched(call):
    from xvector_amd import hip
    err = lambda: hip.lib.xvec_train_last_error().decode()
    need = hip.lib.xvec_tdnn_train_workspace_bytes(2, 20, 24, 32, CTX5, 5)
    assert need > 0
    assert call(hip, lengths=None) == hip.ERR_ARG and err() == "null pointer: lengths_dev"
    assert call(hip, x=None) == hip.ERR_ARG and "null pointer" in err() and "lengths_dev" not in err()
    assert call(hip, ws=None) == hip.ERR_ARG and "null pointer: workspace" in err()
    assert call(hip, T=4) == hip.ERR_ARG and err() == "T = 4 is not longer than the context span 4"
    assert call(hip, ws_bytes=need - 1) == hip.ERR_ARG and err() == f"workspace too small: {need - 1} < {need} bytes"
    assert call(hip, B=1 << 20, T=1 << 12, ws_bytes=1 << 40) == hip.ERR_TOO_LARGE and "row indices are int32" in err()


def _tail_forward(hip, y5=FAKE, Tp=5, ws=FAKE, ws_bytes=None, lengths=LEN):
    if ws_bytes is None:
        ws_bytes = hip.lib.xvec_train_tail_workspace_bytes(2, Tp, 8, 8, 3)
    return hip.lib.xvec_train_tail_forward_ragged(y5, 2, Tp, 8, FAKE, FAKE, 8, FAKE, FAKE, FAKE, FAKE, 3, FAKE, FAKE, FAKE, FAKE, FAKE,
                                                  FAKE, ws, ws_bytes, None, lengths)


def _tail_backward(hip, y5=FAKE, Tp=5, ws=FAKE, ws_bytes=None, lengths=LEN):
    if ws_bytes is None:
        ws_bytes = hip.lib.xvec_train_tail_workspace_bytes(2, Tp, 8, 8, 3)
    return hip.lib.xvec_train_tail_backward_ragged(FAKE, y5, 2, Tp, 8, FAKE, 8, FAKE, FAKE, 3, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE,
                                                   FAKE, FAKE, FAKE, FAKE, FAKE, ws, ws_bytes, None, lengths)


@pytest.mark.parametrize("call", [_tail_forward, _tail_backward], ids=["forward", "backward"])
def test_tail_argument_errors_return_before_the_device_is_touched(call):
    from xvector_amd import hip
    err = lambda: hip.lib.xvec_train_last_error().decode()
    need = hip.lib.xvec_train_tail_workspace_bytes(2, 5, 8, 8, 3)
    assert need > 0
    assert call(hip, lengths=None) == hip.ERR_ARG and err() == "null pointer: lengths_dev"
    assert call(hip, y5=None) == hip.ERR_ARG and "null pointer" in err() and "lengths_dev" not in err()
    assert call(hip, ws=None) == hip.ERR_ARG and "null pointer: workspace" in err()
    assert call(hip, Tp=1, ws_bytes=1 << 20) == hip.ERR_ARG and "at least 2 pooled frames" in err()
    assert call(hip, ws_bytes=need - 1) == hip.ERR_ARG and err() == f"workspace too small: {need - 1} < {need} bytes"


def test_workspace_queries_serve_both_forms_unchanged():
    """The sizes the parent commit reported for these shapes (the ragged calls use the same workspace)."""
    from xvector_amd import hip
    assert hip.lib.xvec_tdnn_train_workspace_bytes(2, 20, 24, 32, CTX5, 5) == 256 + 4096
    assert hip.lib.xvec_tdnn_train_workspace_bytes(7, 61, 40, 24, (C.c_int32 * 3)(-3, 0, 3), 3) == 512 + 37120 + 23040


def test_trainer_refuses_bad_lengths_on_the_host():
    import xvector_amd as xa
    tr = xa.XVectorTrainer(xa.XVectorModel(**KW))
    B, T = 3, 40
    batch = (torch.zeros(B, T, 24), torch.zeros(B, dtype=torch.long), ["a", "b", "c"])      # a CPU batch: refused AFTER the lengths
    for tail in ("torch", "hip"):
        tr.tail = tail
        with pytest.raises(ValueError, match="3 integers"):
            tr.training_step(batch, lengths=[40, 40])
        with pytest.raises(ValueError, match=r"\[16, T=40\]"):
            tr.training_step(batch, lengths=[40, 15, 40])
        with pytest.raises(ValueError, match=r"\[16, T=40\]"):
            tr.training_step(batch, lengths=torch.tensor([40, 41, 40]))
        with pytest.raises(ValueError, match="integers"):
            tr.step(batch, lengths=[40, 20.5, 40])
        with pytest.raises(RuntimeError, match="no CPU path"):
            tr.training_step(batch, lengths=[40, 16, 40])                                   # good lengths: the usual refusal
    with pytest.raises(ValueError, match=r"\[16, T=40\]"):
        tr.logits(batch[0], lengths=[16, 16, 0])


LAYER_KERNELS = tuple(f"train_gemm_kernelILi{op}ELb{vec}ELb1E" for op in (0, 1, 2) for vec in (0, 1)) + (
    "train_stats_kernelILb1E", "train_stats_merge_kernelILb1E", "train_norm_kernelILb1E", "train_bn_sums_kernelILb1E",
    "train_dz_kernelILb1E", "train_slab_reduce_kernel", "train_col_reduce_kernel")
TAIL_KERNELS = ("tail_pool_kernelILi4ELb1E", "tail_pool_kernelILi1ELb1E", "tail_pool_bwd_kernelILi4ELb1E",
                "tail_pool_bwd_kernelILi1ELb1E")
GEMM_LDS = 2 * 2 * 16 * 132 * 4


@needs_hipcc
@pytest.mark.parametrize("src,names", [("tdnn_train_ragged.hip", LAYER_KERNELS), ("train_tail_ragged.hip", TAIL_KERNELS)])
def test_masked_kernels_use_no_scratch(src, names):
    kernels = kernel_resources(src)
    assert len(kernels) == len(names), sorted(kernels)
    for want in names:
        name = [k for k in kernels if want in k]
        assert len(name) == 1, (want, sorted(kernels))
        r = kernels[name[0]]
        assert r["scratch"] == 0 and r.get("spill", 0) == 0, (want, r)
        if "gemm" in want:                                  # the row mask of the forward epilogue reuses the operand buffers
            assert r["lds"] == GEMM_LDS and r["occupancy"] >= 2, (want, r)


@needs_hipcc
def test_unmasked_units_hold_no_masked_kernel():
    """RAGGED is the last template argument of every kernel that has the two forms: a masked one ends in Lb1EEEv."""
    assert not [k for k in kernel_resources("tdnn_train.hip") if "Lb1EEEv" in k]
    assert not [k for k in kernel_resources("train_tail.hip") if "tail_pool" in k and "Lb1EEEv" in k]
    assert len([k for k in kernel_resources("tdnn_train_ragged.hip") if "Lb1EEEv" in k]) == 11
