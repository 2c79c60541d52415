"""The checkpoint-like BatchNorm the GPU tests of test_batchnorm_checkpoint_gpu.py run on, and their CPU references, checked
on the CPU: what the generator promises per layer, layer_ref against the oracle, the fp32 folded form's own distance from the
fp64 layer (the margin under the fp32 bar the kernels are held to), and what plain bf16's deferred-BatchNorm arithmetic costs
against the oracle whatever kernel runs it.  Lines marked [bn] are the ones profiles/batchnorm_edges.txt records (set
XVEC_BN_LOG to a file name to collect them)."""
import numpy as np
import pytest
import torch

import batchnorm_ref as bn
import xvector_oracle as oracle
from conftest import assert_parity, float_params

W4 = dict(input_size=24, hidden_size=136, batch_norm=True, x_vector_size=64, num_classes=5)


record = bn.record


@pytest.fixture(scope="module")
def ckpt(sd42):
    sd, info = bn.calibrated_state_dict(sd42, 42)
    return sd, info, oracle.cast_params(float_params(sd), torch.float64)


@pytest.fixture(scope="module")
def ckpt_w4(synth):
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict(704, **W4).items()}
    sd, info = bn.calibrated_state_dict(sd, 704, **W4)
    return sd, info, oracle.cast_params(float_params(sd), torch.float64)


def test_layer_ref_is_the_oracle_at_its_eps(ckpt, sd42, synth):
    x = torch.as_tensor(synth.make_mfcc(2, 40, seed=1)).double()
    for p64 in (ckpt[2], oracle.cast_params(float_params(sd42), torch.float64)):
        h = x
        for layer in range(5):
            ref = oracle.tdnn_layer(h, p64, f"time_context_layers.{layer}.", oracle.CONTEXTS[layer])
            assert torch.equal(bn.layer_ref(h, p64, layer, 1e-5), ref)
            assert torch.equal(bn.layer_ref(h, p64, layer), ref)
            assert not torch.equal(bn.layer_ref(h, p64, layer, 1e-3), ref)
            pre = f"time_context_layers.{layer}.norm."
            sc = p64[pre + "weight"] / torch.sqrt(p64[pre + "running_var"] + 1e-5)
            back = bn.relu_ref(h, p64, layer) * sc + (p64[pre + "bias"] - p64[pre + "running_mean"] * sc)
            assert torch.allclose(back, ref, rtol=1e-12, atol=1e-12)
            h = ref


@pytest.mark.parametrize("which", ["W0", "W4"])
def test_generator_properties(ckpt, ckpt_w4, synth, which):
    sd, info, p64 = ckpt if which == "W0" else ckpt_w4
    cin = 24
    x = torch.as_tensor(synth.make_mfcc(8, 120, input_size=cin, seed=42 if which == "W0" else 704)).double()
    for layer in range(5):
        pre = f"time_context_layers.{layer}."
        i = info[layer]
        gamma, var, mean = sd[pre + "norm.weight"], sd[pre + "norm.running_var"], sd[pre + "norm.running_mean"]
        cout = gamma.numel()
        assert all(sd[pre + k].dtype == torch.float32 for k in ("linear.bias", "norm.weight", "norm.bias", "norm.running_mean",
                                                                 "norm.running_var"))
        assert len(i["dead"]) == max(1, round(0.02 * cout)) and len(i["rare"]) == max(1, round(0.04 * cout))
        assert len(i["zero"]) == max(1, round(0.02 * cout)) and not set(i["dead"]) & set(i["rare"])
        assert (var[i["dead"]] == 0).all() and (mean[i["dead"]] == 0).all(), "dead channels: exactly 0 and 0"
        assert (gamma[i["zero"]] == 0).all() and int((gamma == 0).sum()) == len(i["zero"])
        r = bn.relu_ref(x, p64, layer).reshape(-1, cout)
        assert (r[:, i["dead"]] == 0).all()
        on = (r[:, i["rare"]] > 0).double().mean(0)
        assert (on > 0).all() and (on <= 0.025).all(), on
        # the running statistics ARE the statistics of the calibration rows
        assert torch.allclose(r.mean(0).float(), mean, rtol=1e-6, atol=0) and torch.allclose(r.var(0).float(), var, rtol=1e-6, atol=0)
        share = len(i["negative"]) / cout
        assert 0.2 < share < 0.4 or cout < 200, share
        live = gamma[gamma.abs() > 1e-20].abs()
        assert live.min() >= 0.05 * (1 - 1e-6) and live.max() <= 4.0 * (1 + 1e-6)
        if layer < 4:
            assert gamma[i["tiny"]].tolist() == [np.float32(1e-30), np.float32(1e-42)]
            assert 0 < float(gamma[i["tiny"][1]]) < float(np.finfo(np.float32).tiny), "1e-42 is denormal"
            sc, _ = bn.folded(sd, layer)
            assert (sc[i["tiny"]].abs() < bn.SCALE_GUARD).all() and (sc[i["tiny"]] > 0).all()
        else:
            assert len(i["tiny"]) == 0
        sc, sh = bn.folded(sd, layer)
        small_var = int((var < 1e-2).sum())
        record(f"generator {which} layer {layer + 1}: {cout} channels, {len(i['dead'])} dead (var == 0), {len(i['rare'])} rarely on, "
               f"{len(i['zero'])} gamma == 0, {len(i['negative'])} gamma < 0, {len(i['tiny'])} gamma tiny, {small_var} with var < 1e-2, "
               f"max |scale| {float(sc.abs().max()):.1f}, max |shift| {float(sh.abs().max()):.1f}")
        x = bn.layer_ref(x, p64, layer)
        # the output the next layer is calibrated on is centred where gamma is not tiny: mean of y = beta
        y = x.reshape(-1, cout)
        ok = gamma.abs() > 1e-20
        assert torch.allclose(y.mean(0)[ok], sd[pre + "norm.bias"].double()[ok], atol=2e-4 * float(sc.abs().max()))


@pytest.mark.parametrize("which", ["W0", "W4"])
def test_fp32_folded_arithmetic_against_the_fp64_layer(ckpt, ckpt_w4, synth, which):
    """The kernels' fp32 form, y = relu(x W^T + b) * scale + shift, on the CPU against layer_ref in fp64: it has to stay under a
    third of the fp32 bar (3.3e-5 row-wise, every element inside assert_parity at 1e-4), or the 1e-4 the GPU tests hold the
    kernels to would be a statement about the checkpoint and not about them."""
    sd, info, p64 = ckpt if which == "W0" else ckpt_w4
    h = torch.as_tensor(synth.make_mfcc(5, 61, seed=61)).double()
    for layer in range(5):
        ref = bn.layer_ref(h.float().double(), p64, layer)
        got = bn.fp32_folded_layer(h.float(), sd, layer)
        err = bn.row_rel(got, ref)
        record(f"fp32 folded form on the CPU, {which} layer {layer + 1}, (5, 61): worst row {err:.2e} (limit 3.3e-5)")
        assert err <= 3.3e-5, (layer, err)
        assert_parity(got, ref, 1e-4, f"{which} layer {layer}")
        const = bn.off_on(h.float().double(), p64, layer, info[layer]["dead"]).tolist() + info[layer]["zero"].tolist()
        beta = sd[f"time_context_layers.{layer}.norm.bias"]
        assert torch.equal(got[..., const], beta[const].expand_as(got[..., const])), "dead and zero-gamma channels are beta exactly"
        h = ref


def test_fp32_forms_differ_element_by_element(ckpt, sd42, synth):
    """Why the GPU tests hold two fp32 forms to each other frame by frame and not element by element.  An fp32 product on the CPU
    against the SAME layer correctly rounded to fp32 (the fp64 sum rounded once in front of the ReLU, then one multiply-add) stays
    inside 1e-5 in every frame, on the synthetic BatchNorm in every element too -- and on this checkpoint it leaves elements
    outside assert_parity's 1e-5 (mean |y| + |y|), where |scale| is large.  A list of the elements whose |scale| 2^-24 sum |w x|
    exceeds that bound is no way out: it is percent of a layer.  The counts depend on the host's matrix product and are recorded,
    not asserted."""
    x = torch.as_tensor(synth.make_mfcc(2, 300, seed=2300))
    for name, sd in (("calibrated", ckpt[0]), ("synthetic", sd42)):
        p64 = oracle.cast_params(float_params(sd), torch.float64)
        h = x.double()
        for layer in range(5):
            pre = f"time_context_layers.{layer}.linear."
            rows = bn._context_rows(h, layer)
            sc, sh = bn.folded(sd, layer)
            z32 = (rows @ p64[pre + "weight"].t() + p64[pre + "bias"]).float()
            ideal = torch.addcmul(sh, torch.relu(z32), sc).double()
            got = bn.fp32_folded_layer(h.float(), sd, layer).double()
            bound = 1e-5 * (ideal.abs().mean() + ideal.abs())
            bad = (got - ideal).abs() > bound
            unit = sc.abs().double() * 2.0 ** -24 * (rows.abs() @ p64[pre + "weight"].abs().t())
            listed = unit > bound
            worst = float(sc.abs()[bad.nonzero()[:, 2]].min()) if bad.any() else float("nan")
            record(f"fp32 product vs correctly rounded fp32 layer, {name}, layer {layer + 1}, (2, 300): worst frame {bn.row_rel(got, ideal):.2e}, "
                   f"{int(bad.sum())} of {bad.numel()} elements outside 1e-5 (smallest |scale| among them {worst:.1f}); |scale| 2^-24 sum|wx| "
                   f"above the bound on {float(listed.double().mean()):.1e} of the elements, {int((bad & ~listed).sum())} of the outside ones not among them")
            assert bn.row_rel(got, ideal) <= 1e-5
            h = bn.layer_ref(h, p64, layer)


def test_bf16_deferred_simulation_against_the_oracle(ckpt, sd42, synth):
    """What plain bf16 costs on this checkpoint whatever kernel runs it: the simulation chained over the five layers, pooled,
    and the layer-6 x-vector, against the fp64 oracle -- next to the same on the synthetic BatchNorm.  (Centring by the real
    mean makes the consumer's W' r and bias' cancel, and the bf16 rounding of W' does not cancel with them.)"""
    x = torch.as_tensor(synth.make_mfcc(5, 61, seed=61))
    for name, sd in (("calibrated", ckpt[0]), ("synthetic", sd42)):
        p64 = oracle.cast_params(float_params(sd), torch.float64)
        stored = bn.bf16_deferred_sim(x, sd)
        refs = bn.chain_ref(x.double(), p64)
        for layer in range(5):
            sc, sh = bn.folded(sd, layer)
            y = stored[layer] * sc.double() + sh.double()
            assert torch.isfinite(y).all()
            record(f"bf16 simulation vs oracle, {name}, layer {layer + 1} chained, (5, 61): worst row {bn.row_rel(y, refs[layer]):.2e}")
        pooled, xv = bn.bf16_pooled_xvec_sim(x, sd)
        ref_p, ref_x = bn.pooled_xvec_ref(x.double(), p64)
        ep, ex = bn.row_rel(pooled, ref_p), bn.row_rel(xv, ref_x)
        record(f"bf16 simulation vs oracle, {name}, (5, 61): pooled {ep:.2e}, x-vector {ex:.2e}")
        assert np.isfinite(ep) and np.isfinite(ex)
        if name == "synthetic":
            assert ep <= 1e-2 and ex <= 1e-2, "the simulation is not plain bf16's arithmetic: it misses the bar the kernels meet"
    # a per-layer entry on the oracle's input: what the unfold on the way in adds
    sd, info, p64 = ckpt
    refs = bn.chain_ref(x.double(), p64)
    for layer in range(1, 5):
        r = bn.bf16_deferred_sim(refs[layer - 1].float(), sd, upto=layer + 1, chained=False)
        sc, sh = bn.folded(sd, layer)
        y = r * sc.double() + sh.double()
        assert torch.isfinite(y).all()
        ref = bn.layer_ref(refs[layer - 1].float().double(), p64, layer)
        record(f"bf16 simulation vs oracle, calibrated, layer {layer + 1} alone on the oracle's input: worst row {bn.row_rel(y, ref):.2e}")
        # the tiny-gamma channels of the input carry nothing: any value there gives the same output
        xin = refs[layer - 1].float().clone()
        xin[..., info[layer - 1]["tiny"]] += 3.0
        assert torch.equal(bn.bf16_deferred_sim(xin, sd, upto=layer + 1, chained=False), r)
