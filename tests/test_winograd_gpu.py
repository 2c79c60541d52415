"""fp32 layers 2 and 3 as Winograd F(2,3) along time (csrc/tdnn_wino.hip) against the fp64 oracle and against the direct form.

Two engines on the same weights: the default one (layers 2-3 of the fp32 path in the Winograd form) and one created under
XVEC_WINOGRAD=0 (read once per handle in xvec_create), which runs every layer in the direct form -- the A/B pair.
  * bench size (B = 256, T = 300): every element of layers 2 and 3 in both forms at the fp32 bar, and the Winograd form's
    worst-frame norm-wise error no more than 1.5x the direct form's on the same input;
  * tails: every residue of T_out mod 2d, the shortest legal utterance, odd batches that end in partial tiles, one long
    utterance; ragged batches with NaN-poisoned padding through the whole path;
  * position and determinism, dispatch / form reporting, graph replay.
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
    return make_model(sd42), make_model(sd42, {"XVEC_WINOGRAD": "0"})


def test_bench_size_every_element_both_forms(models, p64, synth):
    mw, md = models
    h = layer_input(md, synth, 256, 300, 1, seed=7001)
    for layer in WINO_LAYERS:
        ref = oracle_layer(h.cpu(), p64, layer)
        gw = mw.time_context_layers[layer](h)
        assert mw.last_forms()[layer] == "winograd_f23" and mw.last_dispatch()[layer] == "tile128"
        gd = md.time_context_layers[layer](h)
        assert md.last_forms()[layer] == "direct"
        assert_parity(gw, ref.float(), 1e-4, f"layer {layer} winograd B=256 vs oracle")
        assert_parity(gd, ref.float(), 1e-4, f"layer {layer} direct B=256 vs oracle")
        ew, ed = worst_rel(gw, ref), worst_rel(gd, ref)
        print(f"layer {layer}: worst-frame error winograd {ew:.3e}, direct {ed:.3e} ({ew / ed:.2f}x)")
        assert ew <= 1.5 * ed, f"layer {layer}: winograd {ew:.3e} vs direct {ed:.3e}"
        assert torch.equal(gw, mw.time_context_layers[layer](h)), f"layer {layer}: repeat run differs"
        h = gd


# B x T: T_out of layer 2 is T - 8 (residues mod 4), of layer 3 T - 14 (mod 6); T = 15 is the shortest utterance the
# stack accepts (one frame left after layer 3); odd batches end in partial tiles and partial 32-pair groups
SHAPES = [(1, 15), (3, 15), (5, 24), (7, 25), (9, 26), (11, 27), (13, 28), (1, 29), (17, 31), (33, 300), (1, 30000)]


@pytest.mark.parametrize("B,T", SHAPES)
def test_shapes_and_tails(models, p64, synth, B, T):
    mw, md = models
    h = layer_input(md, synth, B, T, 1, seed=7100 + B * 31 + T)
    for layer in WINO_LAYERS:
        gw = mw.time_context_layers[layer](h)
        assert mw.last_forms()[layer] == "winograd_f23"
        gd = md.time_context_layers[layer](h)
        assert_parity(gw, oracle_layer(h.cpu(), p64, layer).float(), 1e-4, f"layer {layer} B={B} T={T}")
        assert_parity(gw, gd, 1e-5, f"layer {layer} B={B} T={T}: winograd vs direct")
        h = gd


def test_ragged_nan_padding_whole_path(models, sd42, synth):
    """Ragged batch (lengths 16..39: every residue of T_out mod 4 and mod 6) with NaN in every padded frame, through the whole
    path: both forms against the oracle per utterance, and against each other."""
    mw, md = models
    lens = [16 + (i * 7) % 24 for i in range(37)]
    T = max(lens)
    x = synth.make_mfcc(len(lens), T, seed=7200)
    for i, n in enumerate(lens):
        x[i, n:] = np.nan
    xg = torch.as_tensor(x).to(DEV)
    gw = mw.extract_x_vec(xg, lengths=lens)
    assert mw.last_forms()[1:3] == ["winograd_f23", "winograd_f23"]
    gd = md.extract_x_vec(xg, lengths=lens)
    with torch.no_grad():
        ref = torch.stack([oracle.extract_x_vec(torch.from_numpy(x[i:i + 1, :n]), float_params(sd42))[0]
                           for i, n in enumerate(lens)])
    assert_parity(gw, ref, 1e-4, "ragged winograd vs oracle")
    assert_parity(gw, gd, 1e-5, "ragged winograd vs direct")


def test_position_independence_and_determinism(models, synth):
    """One utterance at several batch positions gives bit-identical layer-2/3 rows; repeat runs are bit-identical."""
    mw, _ = models
    B, T = 40, 300
    h = layer_input(mw, synth, B, T, 1, seed=7300)
    probe = h[5].clone()
    outs = []
    for pos in (0, 17, 39):
        hp = h.clone()
        hp[pos] = probe
        y2 = mw.time_context_layers[1](hp)
        y3 = mw.time_context_layers[2](y2)
        outs.append((y2[pos], y3[pos]))
        assert torch.equal(y2, mw.time_context_layers[1](hp)), "layer 2: repeat run differs"
    for y2, y3 in outs[1:]:
        assert torch.equal(y2, outs[0][0]) and torch.equal(y3, outs[0][1]), "rows depend on the batch position"


def test_forms_and_dispatch(models, synth):
    mw, md = models
    x = torch.as_tensor(synth.make_mfcc(8, 300, seed=7400)).to(DEV)
    mw.extract_x_vec(x)
    assert mw.last_dispatch() == ["tile128"] * 5
    assert mw.last_forms() == ["direct", "winograd_f23", "winograd_f23", "direct", "direct"]
    md.extract_x_vec(x)
    assert md.last_dispatch() == ["tile128"] * 5
    assert md.last_forms() == ["direct"] * 5


def test_graph_replay_matches_eager(models, synth):
    mw, _ = models
    x = torch.as_tensor(synth.make_mfcc(64, 300, seed=7500)).to(DEV)
    eager = mw.extract_x_vec(x)
    assert mw.last_forms()[1:3] == ["winograd_f23", "winograd_f23"]
    g = mw.graphed(x)
    out = g(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(out, eager), "graph replay differs from eager"
