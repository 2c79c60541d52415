"""fp32 layers 2 and 3 as Winograd F(2,3) on bf16_split3 operands (csrc/tdnn_wino_s3.hip) against the fp64 oracle, the direct
form and the fp32 Winograd kernel (csrc/tdnn_wino.hip).

Engines on the same weights, each created under its own environment (read once per handle in xvec_create):
  * "s3": the default (layers 2-3 take the split operands at large batches);
  * "f32": XVEC_WINO_SPLIT3=0, the fp32 Winograd kernel -- the A/B pair;
  * "direct": XVEC_WINOGRAD=0;
  * "s3all": XVEC_WINO_SPLIT3_MIN_ROWS=0, the split operands at every size (the tails).
"""
import numpy as np
import pytest
import torch

import xvector_oracle as oracle
from conftest import assert_parity, float_params
from tdnn_support import DEV, layer_input, make_model, oracle_layer, p64, worst_rel  # noqa: F401 (p64: a fixture)

pytestmark = pytest.mark.gpu
WINO_LAYERS = (1, 2)          # time_context_layers.1 / .2: contexts [-2, 0, 2] and [-3, 0, 3]


@pytest.fixture(scope="module")
def models(sd42):
    return {"s3": make_model(sd42), "f32": make_model(sd42, {"XVEC_WINO_SPLIT3": "0"}),
            "direct": make_model(sd42, {"XVEC_WINOGRAD": "0"}), "s3all": make_model(sd42, {"XVEC_WINO_SPLIT3_MIN_ROWS": "0"})}


def test_bench_size_every_element_and_error_ratios(models, p64, synth):
    ms, mf, md = models["s3"], models["f32"], models["direct"]
    h = layer_input(md, synth, 256, 300, 1, seed=9001)
    for layer in WINO_LAYERS:
        ref = oracle_layer(h.cpu(), p64, layer)
        gs = ms.time_context_layers[layer](h)
        assert ms.last_forms()[layer] == "winograd_f23" and ms.last_dispatch()[layer] == "tile128"
        assert ms.last_operands()[layer] == "bf16_split3"
        gf = mf.time_context_layers[layer](h)
        assert mf.last_forms()[layer] == "winograd_f23" and mf.last_operands()[layer] == "fp32"
        gd = md.time_context_layers[layer](h)
        assert md.last_forms()[layer] == "direct" and md.last_operands()[layer] == "fp32"
        assert_parity(gs, ref.float(), 1e-4, f"layer {layer} winograd split3 B=256 vs oracle")
        es, ef, ed = worst_rel(gs, ref), worst_rel(gf, ref), worst_rel(gd, ref)
        print(f"layer {layer}: worst-frame error split3 {es:.3e}, fp32 winograd {ef:.3e} ({es / ef:.2f}x), "
              f"direct {ed:.3e} ({es / ed:.2f}x)")
        assert es <= 1.5 * ed, f"layer {layer}: split3 {es:.3e} vs direct {ed:.3e}"
        assert es <= 1.25 * ef, f"layer {layer}: split3 {es:.3e} vs fp32 winograd {ef:.3e}"
        assert torch.equal(gs, ms.time_context_layers[layer](h)), f"layer {layer}: repeat run differs"
        h = gd


SHAPES = [(1, 15), (3, 15), (5, 24), (7, 25), (9, 26), (11, 27), (13, 28), (1, 29), (17, 31), (33, 300), (1, 30000)]


@pytest.mark.parametrize("B,T", SHAPES)
def test_shapes_and_tails(models, p64, synth, B, T):
    m0, md = models["s3all"], models["direct"]
    h = layer_input(md, synth, B, T, 1, seed=9100 + B * 31 + T)
    for layer in WINO_LAYERS:
        g = m0.time_context_layers[layer](h)
        assert m0.last_forms()[layer] == "winograd_f23" and m0.last_operands()[layer] == "bf16_split3"
        gd = md.time_context_layers[layer](h)
        assert_parity(g, oracle_layer(h.cpu(), p64, layer).float(), 1e-4, f"layer {layer} B={B} T={T}")
        assert_parity(g, gd, 1e-5, f"layer {layer} B={B} T={T}: split3 winograd vs direct")
        h = gd


def test_ragged_nan_padding_whole_path(models, sd42, synth):
    m0, md = models["s3all"], models["direct"]
    lens = [16 + (i * 7) % 24 for i in range(37)] + [300, 299, 298, 120]
    T = max(lens)
    x = synth.make_mfcc(len(lens), T, seed=9200)
    for i, n in enumerate(lens):
        x[i, n:] = np.nan
    xg = torch.as_tensor(x).to(DEV)
    g = m0.extract_x_vec(xg, lengths=lens)
    assert m0.last_operands()[1:3] == ["bf16_split3", "bf16_split3"]
    gd = md.extract_x_vec(xg, lengths=lens)
    with torch.no_grad():
        ref = torch.stack([oracle.extract_x_vec(torch.from_numpy(x[i:i + 1, :n]), float_params(sd42))[0]
                           for i, n in enumerate(lens)])
    assert torch.isfinite(g).all()
    assert_parity(g, ref, 1e-4, "ragged split3 winograd vs oracle")
    assert_parity(g, gd, 1e-5, "ragged split3 winograd vs direct")


def test_position_independence_and_determinism(models, synth):
    m0 = models["s3all"]
    h = layer_input(m0, synth, 40, 300, 1, seed=9300)
    probe = h[5].clone()
    outs = []
    for pos in (0, 17, 39):
        hp = h.clone()
        hp[pos] = probe
        y2 = m0.time_context_layers[1](hp)
        y3 = m0.time_context_layers[2](y2)
        assert m0.last_operands()[1:3] == ["bf16_split3", "bf16_split3"]
        outs.append((y2[pos], y3[pos]))
        assert torch.equal(y2, m0.time_context_layers[1](hp)), "layer 2: repeat run differs"
    for y2, y3 in outs[1:]:
        assert torch.equal(y2, outs[0][0]) and torch.equal(y3, outs[0][1]), "rows depend on the batch position"


def test_graph_replay_matches_eager(models, synth):
    m0 = models["s3all"]
    x = torch.as_tensor(synth.make_mfcc(64, 300, seed=9500)).to(DEV)
    eager = m0.extract_x_vec(x)
    assert m0.last_operands()[1:3] == ["bf16_split3", "bf16_split3"]
    g = m0.graphed(x)
    out = g(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(out, eager), "graph replay differs from eager"


def test_whole_path_default_vs_fp32_winograd(models, synth):
    ms, mf = models["s3"], models["f32"]
    x = torch.as_tensor(synth.make_mfcc(256, 300, seed=9600)).to(DEV)
    ys = ms.extract_x_vec(x)
    assert ms.last_operands() == ["fp32", "bf16_split3", "bf16_split3", "bf16_split3", "bf16_split3"]
    yf = mf.extract_x_vec(x)
    assert mf.last_operands() == ["fp32", "fp32", "fp32", "bf16_split3", "bf16_split3"]
    assert mf.last_forms() == ms.last_forms() == ["direct", "winograd_f23", "winograd_f23", "bf16_split3", "bf16_split3"]
    assert_parity(ys, yf, 1e-5, "B=256: default vs XVEC_WINO_SPLIT3=0")
    # below the threshold the default handle keeps the fp32 Winograd kernel
    x8 = torch.as_tensor(synth.make_mfcc(8, 300, seed=9601)).to(DEV)
    ms.extract_x_vec(x8)
    assert ms.last_operands()[1:3] == ["fp32", "fp32"]
