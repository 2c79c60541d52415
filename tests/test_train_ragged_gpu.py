"""Ragged training on the GPU (include/xvec_train.h, "Ragged batches"; csrc/tdnn_train_ragged.hip, csrc/train_tail_ragged.hip;
xvector_amd.train with lengths=) against tests/train_ragged_ref.py, the fp64 autograd oracle on per-utterance slices, at the bar
of tests/test_train_gpu.py and tests/test_train_tail_gpu.py: assert_parity at 1e-4 (row-wise relative plus element-wise).

Sizes.  The product kernel's row tile is 128 rows (its column tile 128, its K step 16), the column reductions work in chunks of
256 rows, dW in slices of at least 256 rows.  B = 7, T = 61 gives T' = 55 .. 61 and 385 .. 427 padded rows: utterances end in
mid-tile and in mid-chunk, one has ONE valid output row, one two, two are full.  An in-range length always leaves an utterance
its first row valid, so with T' < 128 no tile and no chunk is without a valid row; the all-invalid tile and chunk (and a batch
that STARTS with one) come from the case with B = 17, where ten utterances carry lengths outside [span + 1, T] and so, by the
contract, contribute no rows: 5 x 57 = 285 leading rows and 285 more in the middle.

The oracle takes its gradients from autograd, so its ReLU mask is its own: every parity case first asserts, on the CPU, that
the fp64 pre-activation of every valid element is further from 0 than the fp32 rounding error of the product can reach
(train_ragged_ref.fp32_product_error) -- a property of the seeds chosen here, not a filter: no element is left out.

x beyond each length and dy on the invalid rows are NaN in every parity case; every output and the workspace sit in poisoned
windows of exactly the stated size between guards (the pattern of tests/test_augment_edges_gpu.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import train_ragged_ref as rref
import train_ref
import train_tail_ref
from conftest import assert_parity
from test_train_gpu import ADAM_LOSS_BOUND, Window, make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTX = train_ref.CONTEXTS
B, T = 7, 61
WIDTHS = [(24, 40), (40, 24), (40, 40), (24, 24), (40, 24)]         # (Cin, Cout) per context
# seeds per (context index, BatchNorm) for which the margin precondition holds.  To re-pick one after a change of make_case
# or of the shapes: on the CPU, count up from 100 until rref.layer(<the case in float64>, lengths_of(context), context) has
# (pre.abs() / err).min() > 1.5 -- the tests assert > 1 -- (the same for the B = 17 case from 131 and for STEP_SEED from 7 with
# rref.training_step(..., pre_margin=[])).
SEEDS = {(i, bn): 101 if i == 0 else 100 for i in range(5) for bn in (True, False)}
NAN = float("nan")


def lengths_of(context):
    s = rref.span_of(context)
    return [61, s + 1, 47, 20, 33, 61, s + 2]


def poison(case, lengths, context):
    """NaN in x past each length and in dy on every invalid row (in-range or not)."""
    c = {k: v.clone() for k, v in case.items()}
    Tx = c["x"].shape[1]
    for b, (l, v) in enumerate(zip(lengths, rref.valid_rows(lengths, Tx, context))):
        c["x"][b, (l if v else 0):] = NAN
        c["dy"][b, v:] = NAN
    return c


def run_layer(case, context, lengths=None, need_dx=True, eps=train_ref.EPS):
    """Both C-ABI calls of one form (lengths=None: the unmasked calls) on one case; every output in a guarded window, the
    workspace of exactly the queried size between two guards and poisoned before each call.  Returns {name: cpu tensor}."""
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
    p = lambda name: out[name].ptr() if name in out else None
    dp = lambda name: d[name].data_ptr() if name in d else None
    s = torch.cuda.current_stream().cuda_stream
    extra = ()
    fwd, bwd = hip.lib.xvec_tdnn_train_forward, hip.lib.xvec_tdnn_train_backward
    if lengths is not None:
        ldev = torch.tensor(lengths, dtype=torch.int32).to(DEV)
        extra = (ldev.data_ptr(),)
        fwd, bwd = hip.lib.xvec_tdnn_train_forward_ragged, hip.lib.xvec_tdnn_train_backward_ragged
    rc = fwd(dp("x"), nb, nt, cin, dp("W"), dp("b"), cout, carr, len(context), dp("gamma"), dp("beta"), eps, p("z"), p("mean"),
             p("var"), p("y"), ws.data_ptr(), need, s, *extra)
    assert rc == 0, hip.lib.xvec_train_last_error().decode()
    ws.view(torch.float32).fill_(NAN)
    rc = bwd(dp("dy"), dp("x"), p("z"), nb, nt, cin, dp("W"), cout, carr, len(context), dp("gamma"), p("mean"), p("var"), eps,
             p("dx"), p("dW"), p("db"), p("dgamma"), p("dbeta"), ws.data_ptr(), need, s, *extra)
    assert rc == 0, hip.lib.xvec_train_last_error().decode()
    torch.cuda.synchronize()
    assert (wsbuf[:256] == 0xA5).all() and (wsbuf[-256:] == 0xA5).all(), "workspace guard overwritten"
    return {k: w.check(k) for k, w in out.items()}           # check: guards intact, the window fully written, nothing NaN


@functools.lru_cache(maxsize=None)
def layer_case(i, bn, nb=B, seed=None):
    cin, cout = WIDTHS[i]
    return make_case(nb, T, cin, cout, CTX[i], bn, SEEDS[(i, bn)] if seed is None else seed)


@functools.lru_cache(maxsize=None)
def layer_oracle(i, bn, lengths, nb=B, seed=None):
    case = layer_case(i, bn, nb, seed)
    return rref.layer({k: v.double() for k, v in case.items()}, list(lengths), CTX[i])


def check_layer(case, context, lengths, got, want):
    margin = float((want["pre"].abs() / want["err"]).min())
    print(f"[ragged] {sum(want['counts'])} valid rows; min |pre| / fp32 error bound = {margin:.2f}")
    bn = "gamma" in case
    assert_parity(got["z"], want["z"], what="z")
    if bn:
        assert_parity(got["y"], want["y"], what="y")
        assert_parity(got["mean"], want["mean"], what="batch_mean")
        assert_parity(1.0 / torch.sqrt(got["var"].double() + train_ref.EPS), 1.0 / torch.sqrt(want["var"] + train_ref.EPS),
                      what="1/sqrt(var+eps)")
    for name in ["dW", "db", "dx"] + (["dgamma", "dbeta"] if bn else []):
        assert_parity(got[name], want[name], what=name)
    for b, (l, v) in enumerate(zip(lengths, want["counts"])):
        assert (got["z"][b, v:] == 0).all(), f"z rows of utterance {b} past {v}"
        if bn:
            assert (got["y"][b, v:] == 0).all(), f"y rows of utterance {b} past {v}"
        assert (got["dx"][b, (l if v else 0):] == 0).all(), f"dx rows of utterance {b} past its length"


# ---------------------------------------------------------------- 1. equal lengths: nothing existing moved
@pytest.mark.parametrize("bn", [True, False], ids=["bn", "nobn"])
@pytest.mark.parametrize("i", range(5))
def test_equal_lengths_are_bit_identical_to_the_unmasked_calls(i, bn):
    case = layer_case(i, bn)
    old = run_layer(case, CTX[i])
    new = run_layer(case, CTX[i], [T] * B)
    assert sorted(old) == sorted(new) and len(old) == (9 if bn else 4)
    for k in old:
        assert torch.equal(old[k], new[k]), k


# ---------------------------------------------------------------- 2. parity on poisoned padding
@pytest.mark.parametrize("bn", [True, False], ids=["bn", "nobn"])
@pytest.mark.parametrize("i", range(5))
def test_layer_parity_with_poisoned_padding(i, bn):
    lengths = lengths_of(CTX[i])
    want = layer_oracle(i, bn, tuple(lengths))
    assert (want["pre"].abs() > want["err"]).all(), "seed: a pre-activation within the fp32 error of zero"
    assert want["counts"][1] == 1 and want["counts"][6] == 2 and want["counts"][0] == want["counts"][5] == T - rref.span_of(CTX[i])
    case = poison(layer_case(i, bn), lengths, CTX[i])
    check_layer(case, CTX[i], lengths, run_layer(case, CTX[i], lengths), want)


def test_tiles_and_chunks_without_a_valid_row():
    """B = 17: the first five and five more utterances have lengths outside [span + 1, T] (0, negative, T + 1, span): they
    contribute no rows, everything of theirs is 0, and the batch starts with 285 invalid rows -- two row tiles and the first
    chunk hold none that is valid."""
    i, bn, nb = 1, True, 17
    s = rref.span_of(CTX[i])
    lengths = [0, -3, T + 1, s, 1 << 30] + [61, s + 1, 47] + [T + 1, 0, s, -1, 70] + [20, 33, 61, s + 2]
    want = layer_oracle(i, bn, tuple(lengths), nb, 131)
    assert (want["pre"].abs() > want["err"]).all(), "seed: a pre-activation within the fp32 error of zero"
    assert want["counts"][:5] == [0] * 5 and want["counts"][8:13] == [0] * 5 and 5 * (T - s) > 256
    case = poison(layer_case(i, bn, nb, 131), lengths, CTX[i])
    check_layer(case, CTX[i], lengths, run_layer(case, CTX[i], lengths), want)


# ---------------------------------------------------------------- 3. the tail
TAIL_SHAPE = (6, 9, 40, 8, 5)          # B, Tp, C, H, K
TAIL_LENGTHS = [2, 9, 5, 7, 9, 3]
TAIL_NAMES = ("pooled", "a6", "a7", "logits", "loss", "dW6", "db6", "dW7", "db7", "dWo", "dbo", "dy5")


def run_tail(case, lengths=None):
    from xvector_amd import hip
    d = {k: v.to(DEV).contiguous() for k, v in case.items()}
    nb, tp, c = case["y5"].shape
    h, k = case["W6"].shape[0], case["Wo"].shape[0]
    need = hip.lib.xvec_train_tail_workspace_bytes(nb, tp, c, h, k)
    assert need > 0 and need % 256 == 0
    wsbuf = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = wsbuf[256: 256 + need]
    ws.view(torch.float32).fill_(NAN)
    out = {"pooled": Window(nb, 2 * c), "a6": Window(nb, h), "a7": Window(nb, h), "logits": Window(nb, k), "loss": Window(1),
           "dW6": Window(h, 2 * c), "db6": Window(h), "dW7": Window(h, h), "db7": Window(h), "dWo": Window(k, h), "dbo": Window(k),
           "dy5": Window(nb, tp, c)}
    p = lambda name: out[name].ptr()
    dp = lambda name: d[name].data_ptr()
    dl = torch.ones(1, dtype=torch.float32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    extra = ()
    fwd, bwd = hip.lib.xvec_train_tail_forward, hip.lib.xvec_train_tail_backward
    if lengths is not None:
        ldev = torch.tensor(lengths, dtype=torch.int32).to(DEV)
        extra = (ldev.data_ptr(),)
        fwd, bwd = hip.lib.xvec_train_tail_forward_ragged, hip.lib.xvec_train_tail_backward_ragged
    rc = fwd(dp("y5"), nb, tp, c, dp("W6"), dp("b6"), h, dp("W7"), dp("b7"), dp("Wo"), dp("bo"), k, dp("labels"), p("pooled"),
             p("a6"), p("a7"), p("logits"), p("loss"), ws.data_ptr(), need, s, *extra)
    assert rc == 0, hip.lib.xvec_train_last_error().decode()
    ws.view(torch.float32).fill_(NAN)
    rc = bwd(dl.data_ptr(), dp("y5"), nb, tp, c, dp("W6"), h, dp("W7"), dp("Wo"), k, dp("labels"), p("pooled"), p("a6"), p("a7"),
             p("logits"), p("dy5"), p("dW6"), p("db6"), p("dW7"), p("db7"), p("dWo"), p("dbo"), ws.data_ptr(), need, s, *extra)
    assert rc == 0, hip.lib.xvec_train_last_error().decode()
    torch.cuda.synchronize()
    assert (wsbuf[:256] == 0xA5).all() and (wsbuf[-256:] == 0xA5).all(), "workspace guard overwritten"
    return {name: w.check(name) for name, w in out.items()}


def tail_case():
    case = {k: v.clone() for k, v in train_tail_ref.make_case(*TAIL_SHAPE, 1).items()}
    case["y5"][2, :5] = case["y5"][2, 0]           # utterance 2 is constant over its five valid frames, in every channel
    case["y5"][4, :, 7] = 3.25                     # and one channel of a full utterance
    return case


def test_tail_equal_lengths_are_bit_identical_to_the_unmasked_calls():
    case = tail_case()
    old, new = run_tail(case), run_tail(case, [TAIL_SHAPE[1]] * TAIL_SHAPE[0])
    for k in TAIL_NAMES:
        assert torch.equal(old[k], new[k]), k


def test_tail_parity_with_poisoned_padding():
    case = tail_case()
    c64 = {k: (v.double() if v.is_floating_point() else v) for k, v in case.items()}
    want = rref.tail(c64, TAIL_LENGTHS)
    pre6 = want["pooled"] @ c64["W6"].T + c64["b6"]
    pre7 = pre6.clamp_min(0) @ c64["W7"].T + c64["b7"]
    for pre in (pre6, pre7):                       # the bar of tests/test_train_tail_gpu.py for "near zero": none is
        assert (pre.abs() > 1e-4 * pre.abs().mean()).all(), "seed: a segment-layer pre-activation near zero"
    for b, l in enumerate(TAIL_LENGTHS):
        case["y5"][b, l:] = NAN
    got = run_tail(case, TAIL_LENGTHS)
    c = TAIL_SHAPE[2]
    for name in ("pooled", "logits", "dW6", "db6", "dW7", "db7", "dWo", "dbo", "dy5"):
        assert_parity(got[name], want[name], what=name)
    assert abs(float(got["loss"][0]) - float(want["loss"])) <= 1e-4 * abs(float(want["loss"]))
    for b, l in enumerate(TAIL_LENGTHS):
        assert (got["dy5"][b, l:] == 0).all(), f"dy5 rows of utterance {b} past {l}"
    assert (got["pooled"][2, c:] == 0).all() and got["pooled"][4, c + 7] == 0 and got["pooled"][4, 7] == 3.25
    assert torch.equal(got["pooled"][2, :c], case["y5"][2, 0])
    assert (got["dy5"][2, :5] == got["dy5"][2, :1]).all()          # no std term: one value per channel, dmean / 5
    assert (got["dy5"][4, :, 7] == got["dy5"][4, 0, 7]).all()


# ---------------------------------------------------------------- 4. - 6. the whole step
KW = dict(hidden_size=32, num_classes=5, x_vector_size=8)
STEP_LENGTHS = [48, 16, 30, 48, 23, 41]
STEP_SEED = 23


def step_model(synth):
    import xvector_amd as xa
    m = xa.XVectorModel(**KW)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict(seed=STEP_SEED, input_size=24, **KW).items()})
    return m.to(DEV)


def step_batch(synth, pad=NAN):
    x = torch.from_numpy(synth.make_mfcc(6, 48, seed=STEP_SEED + 1)).clone()
    for b, l in enumerate(STEP_LENGTHS):
        x[b, l:] = pad
    return x, torch.tensor([0, 3, 1, 4, 2, 3])


@pytest.fixture(scope="module")
def step_oracle(synth):
    """One fp64 ragged step (loss, gradients, the state after it with its moved buffers, the margins) and three Adam losses."""
    x, labels = step_batch(synth)
    sd = train_ref.cast_state(synth.make_state_dict(seed=STEP_SEED, input_size=24, **KW), torch.float64)
    margins = []
    loss, grads = rref.training_step(sd, x.double(), STEP_LENGTHS, labels, pre_margin=margins)
    sd2 = train_ref.cast_state(synth.make_state_dict(seed=STEP_SEED, input_size=24, **KW), torch.float64)
    losses = rref.adam_losses(sd2, x.double(), STEP_LENGTHS, labels, 3, 1e-3)
    return {"loss": float(loss), "grads": grads, "sd": sd, "margins": margins, "adam": np.array(losses)}


def run_step(synth, tail):
    import xvector_amd as xa
    model = step_model(synth)
    x, labels = step_batch(synth)
    tr = xa.XVectorTrainer(model, tail=tail)
    out = tr.training_step((x.to(DEV), labels.to(DEV), list(range(6))), 0, lengths=STEP_LENGTHS)
    out["loss"].backward()
    return model, out


@pytest.mark.parametrize("tail", ["torch", "hip"])
def test_whole_step_matches_the_oracle(synth, step_oracle, tail):
    # The bound is the WORST case over K + 1 roundings, (K + 2) u; the roundings of a real product add up like a random walk,
    # ~sqrt(K) u.  The inputs of layers 2-5 carry the error of the layers before, a few u relative: 1.5 x the worst-case
    # bound of the product alone covers both.
    print(f"[ragged] step margins (min |pre| / fp32 bound per layer): {step_oracle['margins']}")
    assert min(step_oracle["margins"]) > 1.5, step_oracle["margins"]
    model, out = run_step(synth, tail)
    assert out["train_preds"].shape == (6, 5)
    print(f"[ragged] {tail} loss {out['loss'].item():.9f} oracle {step_oracle['loss']:.9f}")
    assert abs(out["loss"].item() - step_oracle["loss"]) <= 1e-4 * step_oracle["loss"]
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert sorted(grads) == sorted(step_oracle["grads"]) and len(grads) == 26
    for k, g in grads.items():
        assert g is not None, k
        assert_parity(g, step_oracle["grads"][k], what=f"{tail} d {k}")
    n = 0
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(step_oracle["sd"][k])
        elif "running" in k:
            assert_parity(v, step_oracle["sd"][k], what=f"{tail} {k}")
            n += 1
    assert n == 10


@pytest.mark.parametrize("tail", ["torch", "hip"])
def test_three_ragged_steps_follow_adam_on_the_oracle(synth, step_oracle, tail):
    import xvector_amd as xa
    assert step_model(synth).learning_rate == 1e-3
    x, labels = step_batch(synth)
    tr = xa.XVectorTrainer(step_model(synth), tail=tail)
    batch = (x.to(DEV), labels.to(DEV), list(range(6)))
    losses = np.array([float(tr.step(batch, lengths=STEP_LENGTHS)) for _ in range(3)])
    dev = np.abs(losses - step_oracle["adam"]) / step_oracle["adam"]
    print(f"[ragged] {tail} adam losses {losses.tolist()} relative deviation {dev.tolist()} bound {ADAM_LOSS_BOUND:.3e}")
    assert np.isfinite(losses).all() and losses[2] < losses[1] < losses[0]
    assert dev[0] <= 1e-4
    assert dev[1:].max() <= ADAM_LOSS_BOUND, dev


@pytest.mark.parametrize("tail", ["torch", "hip"])
def test_train_and_extract_agree_on_the_lengths(synth, tail):
    import xvector_amd as xa
    model = step_model(synth)
    x, labels = step_batch(synth, pad=0.0)
    tr = xa.XVectorTrainer(model, tail=tail)
    batch = (x.to(DEV), labels.to(DEV), list(range(6)))
    tr.step(batch, lengths=STEP_LENGTHS)
    val = tr.validation_step(batch, lengths=STEP_LENGTHS)
    model.eval()
    with torch.no_grad():
        direct = model(x.to(DEV), STEP_LENGTHS)
        full = model(x.to(DEV))
    assert torch.equal(val["val_preds"], direct)
    assert not torch.equal(direct, full)               # the lengths do reach the extraction


def test_layer_lengths_are_refused_on_the_host(synth):
    import xvector_amd as xa
    model = step_model(synth)
    x = torch.zeros(3, 40, 24, device=DEV)
    with pytest.raises(ValueError, match=r"\[5, T=40\]"):
        xa.tdnn_layer_train(x, model.time_context_layers[0], lengths=[40, 4, 40])
    y = xa.tdnn_layer_train(x, model.time_context_layers[0], lengths=torch.tensor([40, 5, 40]))
    assert y.shape == (3, 36, 32) and (y[1, 1:] == 0).all()


def test_ragged_runs_are_bit_identical(synth):
    i, bn = 0, True
    lengths = lengths_of(CTX[i])
    case = poison(layer_case(i, bn), lengths, CTX[i])
    a, b = run_layer(case, CTX[i], lengths), run_layer(case, CTX[i], lengths)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for tail in ("torch", "hip"):
        runs = []
        for _ in range(2):
            model, out = run_step(synth, tail)
            runs.append([out["loss"].detach().cpu()] + [p.grad.cpu() for p in model.parameters()]
                        + [v.cpu() for v in model.state_dict().values()])
        assert len(runs[0]) > 50
        for u, v in zip(*runs):
            assert torch.equal(u, v)
