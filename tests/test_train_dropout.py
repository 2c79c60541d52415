"""CPU-only checks of dropout in the training layers (include/xvec_train.h, "Dropout"): tests/train_dropout_ref.py -- Philox4x32-10
and the keep rule restated in numpy -- gives the generator's known answers; xvec_dropout_keep_host, which evaluates the header
the kernels use (csrc/dropout_mask.h), equals it element for element; the keep rule's properties and statistics; the three new
calls are exported, declared and bound, and their argument checks return before a device is touched; XVectorTrainer wants a
seed with dropout_p != 0."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import train_dropout_ref as dref

BIG_SEED, BIG_STREAM = (0xC0FFEE << 32) | 0x12345678, (7 << 32) | 9          # both words of seed and stream in use


def host_mask(N, cout, p, seed, stream):
    from xvector_amd import hip
    buf = np.full(N * cout + 16, 0xA5, dtype=np.uint8)                       # a guard behind the mask
    rc = hip.lib.xvec_dropout_keep_host(buf.ctypes.data, N, cout, p, seed, stream)
    assert rc == 0, hip.lib.xvec_train_last_error().decode()
    assert (buf[N * cout:] == 0xA5).all(), "written past N * Cout"
    assert set(np.unique(buf[:N * cout])) <= {0, 1}
    return buf[:N * cout].reshape(N, cout).astype(bool)


# ---------------------------------------------------------------- the generator
KNOWN = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = dref.philox4x32_10([np.array([v]) for v in counter], key)
    assert " ".join(f"{int(w[0]):08x}" for w in got) == want


def test_threshold_and_scale():
    assert dref.threshold(0.0) == 0 and dref.scale(0.0) == 1.0
    assert dref.threshold(0.5) == 1 << 31 and dref.scale(0.5) == 2.0
    assert dref.threshold(0.1) == math.floor(float(np.float32(0.1)) * 2 ** 32)
    assert dref.threshold(np.nextafter(np.float32(1), np.float32(0))) == 2 ** 32 - 256


@pytest.mark.parametrize("N,cout", [(1, 1), (5, 7), (131, 129), (2048, 512)])
@pytest.mark.parametrize("p,seed,stream", [(0.1, BIG_SEED, BIG_STREAM), (0.5, 1234, 3), (0.37, (1 << 64) - 1, (1 << 64) - 1)])
def test_host_mask_equals_the_numpy_restatement(N, cout, p, seed, stream):
    assert np.array_equal(host_mask(N, cout, p, seed, stream), dref.keep_mask(N, cout, p, seed, stream))


def test_keep_rule_properties():
    N, cout = 131, 129
    assert host_mask(N, cout, 0.0, BIG_SEED, BIG_STREAM).all()
    almost_one = float(np.nextafter(np.float32(1), np.float32(0)))          # thr = 2^32 - 256: a word survives with 2^-24
    assert host_mask(2048, 512, almost_one, BIG_SEED, BIG_STREAM).sum() <= 4
    base = host_mask(N, cout, 0.3, BIG_SEED, BIG_STREAM)
    assert np.array_equal(host_mask(N + 5, cout, 0.3, BIG_SEED, BIG_STREAM)[:N], base)      # rows are named by n alone
    assert np.array_equal(host_mask(N, cout + 3, 0.3, BIG_SEED, BIG_STREAM)[:, :cout], base)    # and columns by c
    for seed, stream in [(BIG_SEED + 1, BIG_STREAM), (BIG_SEED, BIG_STREAM + 1), (BIG_SEED ^ (1 << 40), BIG_STREAM),
                         (BIG_SEED, BIG_STREAM ^ (1 << 40))]:            # each word of seed and stream reaches the mask
        other = host_mask(N, cout, 0.3, seed, stream)
        assert 0.3 < (other != base).mean() < 0.55                        # independent masks differ on 2 p (1 - p) = 0.42
    lower = host_mask(N, cout, 0.1, BIG_SEED, BIG_STREAM)
    assert (lower | ~base).all()                                          # what p = 0.3 keeps, p = 0.1 keeps too


@pytest.mark.parametrize("seed,stream,p", [(1234, 0, 0.1), (1234, 3, 0.5), (7, 9, 0.2)])
def test_drop_share_statistics(seed, stream, p):
    N, cout = 2048, 512
    dropped = ~host_mask(N, cout, p, seed, stream)
    overall = abs(dropped.mean() - p) / math.sqrt(p * (1 - p) / (N * cout))
    per_channel = (np.abs(dropped.mean(0) - p) / math.sqrt(p * (1 - p) / N)).max()
    per_row = (np.abs(dropped.mean(1) - p) / math.sqrt(p * (1 - p) / cout)).max()
    print(f"[dropout] p = {p}: overall {overall:.2f} sigma, worst channel {per_channel:.2f} sigma, worst row {per_row:.2f} sigma")
    assert overall <= 4.0
    assert per_channel <= 5.0


# ---------------------------------------------------------------- argument checks through ctypes
FAKE = C.c_void_p(0x1000)      # never dereferenced: every check below returns before the device is touched
CTX5 = (C.c_int32 * 5)(-2, -1, 0, 1, 2)


def _forward(hip, x=FAKE, T=20, ws=FAKE, ws_bytes=None, lengths=None, p=0.1):
    if ws_bytes is None:
        ws_bytes = hip.lib.xvec_tdnn_train_workspace_bytes(2, 20, 24, 32, CTX5, 5)
    return hip.lib.xvec_tdnn_train_forward_dropout(x, 2, T, 24, FAKE, FAKE, 32, CTX5, 5, FAKE, FAKE, 1e-5, FAKE, FAKE, FAKE, FAKE, ws,
                                                   ws_bytes, None, lengths, p, BIG_SEED, BIG_STREAM)


def _backward(hip, x=FAKE, T=20, ws=FAKE, ws_bytes=None, lengths=None, p=0.1):
    if ws_bytes is None:
        ws_bytes = hip.lib.xvec_tdnn_train_workspace_bytes(2, 20, 24, 32, CTX5, 5)
    return hip.lib.xvec_tdnn_train_backward_dropout(x, FAKE, FAKE, 2, T, 24, FAKE, 32, CTX5, 5, FAKE, FAKE, FAKE, 1e-5, None, FAKE,
                                                    FAKE, FAKE, FAKE, ws, ws_bytes, None, lengths, p)


def test_the_three_calls_are_exported_and_bound():
    from xvector_amd import hip
    for name in ("xvec_tdnn_train_forward_dropout", "xvec_tdnn_train_backward_dropout", "xvec_dropout_keep_host"):
        assert name in hip.EXPORTS and getattr(hip.lib, name).argtypes
    assert hip.lib.xvec_tdnn_train_forward_dropout.argtypes[-3:] == [C.c_float, C.c_uint64, C.c_uint64]
    assert hip.lib.xvec_tdnn_train_backward_dropout.argtypes[-1] is C.c_float


@pytest.mark.parametrize("call", [_forward, _backward], ids=["forward", "backward"])
@pytest.mark.parametrize("lengths", [None, FAKE], ids=["fixed", "ragged"])
def test_argument_errors_return_before_the_device_is_touched(call, lengths):
    from xvector_amd import hip
    err = lambda: hip.lib.xvec_train_last_error().decode()
    need = hip.lib.xvec_tdnn_train_workspace_bytes(2, 20, 24, 32, CTX5, 5)
    assert need > 0
    for p in (-0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        assert call(hip, lengths=lengths, p=p) == hip.ERR_ARG and "0 <= p < 1" in err() and "dropout p" in err(), p
    assert call(hip, lengths=lengths, x=None) == hip.ERR_ARG and "null pointer" in err()
    assert call(hip, lengths=lengths, ws=None) == hip.ERR_ARG and "null pointer: workspace" in err()
    assert call(hip, lengths=lengths, T=4) == hip.ERR_ARG and err() == "T = 4 is not longer than the context span 4"
    assert call(hip, lengths=lengths, ws_bytes=need - 1) == hip.ERR_ARG and err() == f"workspace too small: {need - 1} < {need} bytes"
    assert call(hip, lengths=lengths, p=float("nan"), x=None) == hip.ERR_ARG and "dropout p" in err()      # p is looked at first


def test_keep_host_argument_errors():
    from xvector_amd import hip
    err = lambda: hip.lib.xvec_train_last_error().decode()
    buf = np.zeros(64, dtype=np.uint8)
    q = hip.lib.xvec_dropout_keep_host
    assert q(None, 4, 4, 0.1, 1, 2) == hip.ERR_ARG and "null pointer: keep_host" in err()
    assert q(buf.ctypes.data, 0, 4, 0.1, 1, 2) == hip.ERR_ARG and "must be >= 1" in err()
    assert q(buf.ctypes.data, 4, 0, 0.1, 1, 2) == hip.ERR_ARG and "must be >= 1" in err()
    assert q(buf.ctypes.data, 1 << 31, 4, 0.1, 1, 2) == hip.ERR_TOO_LARGE and "row indices are int32" in err()
    for p in (-1e-9, 1.0, float("nan")):
        assert q(buf.ctypes.data, 4, 4, p, 1, 2) == hip.ERR_ARG and "0 <= p < 1" in err()
    assert not buf.any()


# ---------------------------------------------------------------- the trainer, on the host
def test_trainer_wants_a_seed_with_dropout(tmp_path):
    import xvector_amd as xa
    kw = dict(hidden_size=32, num_classes=5, x_vector_size=8)
    with pytest.raises(RuntimeError, match=r"dropout_p = 0\.1.*dropout_seed="):
        xa.XVectorTrainer(xa.XVectorModel(dropout_p=0.1, **kw))
    tr = xa.XVectorTrainer(xa.XVectorModel(dropout_p=0.1, **kw), dropout_seed=5)
    assert tr.dropout_state() == {"seed": 5, "step": 0}
    tr.load_dropout_state({"seed": BIG_SEED, "step": 12})
    assert tr.dropout_state() == {"seed": BIG_SEED, "step": 12}
    tr.save_checkpoint(str(tmp_path / "drop.ckpt"))
    ckpt = torch.load(str(tmp_path / "drop.ckpt"), weights_only=False)
    assert sorted(ckpt) == ["hyper_parameters", "state_dict", "xvec_dropout"] and ckpt["xvec_dropout"] == tr.dropout_state()
    assert xa.XVectorModel.load_from_checkpoint(str(tmp_path / "drop.ckpt")).hparams["dropout_p"] == 0.1
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError, match="dropout_seed"):
            xa.XVectorTrainer(xa.XVectorModel(dropout_p=0.1, **kw), dropout_seed=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):             # dropout or not, there is no CPU path
        xa.tdnn_layer_train(torch.zeros(2, 40, 24), tr.model.time_context_layers[0], dropout=(5, 0))


def test_a_seed_without_dropout_changes_nothing(tmp_path):
    import xvector_amd as xa
    kw = dict(hidden_size=32, num_classes=5, x_vector_size=8)
    torch.manual_seed(0)
    model = xa.XVectorModel(**kw)
    plain, seeded = xa.XVectorTrainer(model), xa.XVectorTrainer(model, dropout_seed=5)
    assert seeded.dropout_state() is None and plain.dropout_state() is None
    with pytest.raises(RuntimeError, match="no dropout"):
        seeded.load_dropout_state({"seed": 5, "step": 1})
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    plain.save_checkpoint(str(tmp_path / "a" / "last.ckpt"))          # (one file name: torch.save writes it into the archive)
    seeded.save_checkpoint(str(tmp_path / "b" / "last.ckpt"))
    assert open(str(tmp_path / "a" / "last.ckpt"), "rb").read() == open(str(tmp_path / "b" / "last.ckpt"), "rb").read()
    assert sorted(torch.load(str(tmp_path / "a" / "last.ckpt"), weights_only=False)) == ["hyper_parameters", "state_dict"]
