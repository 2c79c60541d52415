"""The Winograd split3 kernel on 256-channel tiles (csrc/tdnn_wino_s3w.hip: eight waves, one block per CU, the two wave sets
staging alternate chunks) against the four-wave kernel (csrc/tdnn_wino_s3.hip), which computes every output with the same
arithmetic in the same order: layers 2 and 3 must be the same BITS, and both must meet the fp64 oracle at the fp32 bar (1e-4).

Handles: XVEC_WINO_SPLIT3_MIN_ROWS=0 sends every batch to the split3 Winograd form; with XVEC_BLOCKS_PER_CU=2 on top the
planner keeps the four-wave kernel.  Which kernel a layer went to is read from the launch record (last_launches: 512 threads
= the wide kernel, 256 = the four-wave one); forms, operands and the kernel family read as before.

  widths   256 (one wide column) and 512 (two); 384 and 32 are no multiple of 256: the planner must fall back and say so
  batches  B = 1, T = 15      fewer pairs than one tile, more blocks than tiles
           B = 3, T = 21, 22  one-output pairs: T' mod 2d < d and >= d for d = 2 and 3
           B = 5, T = 77      several tiles, an odd last tile of 32 pairs
           ragged (15, 40, 16, 133) with NaN in the padding, through the whole path
  replay   a repeated launch and a graph replay give the same bits"""
import numpy as np
import pytest
import torch

import xvector_oracle as oracle
from conftest import assert_parity, float_params
from tdnn_support import DEV, make_model, oracle_layer, workspace_rows, worst_rel

pytestmark = pytest.mark.gpu
WINO_LAYERS = (1, 2)          # time_context_layers.1 / .2: contexts [-2, 0, 2] and [-3, 0, 3]
SHAPES = [(1, 15), (3, 21), (3, 22), (5, 77)]
RAGGED = [15, 40, 16, 133]
_CACHE = {}


def _kw(hid):
    return dict(input_size=24, hidden_size=hid, num_classes=7, x_vector_size=16, batch_norm=True)


def _handles(hid):
    """(model on the default grid, model at XVEC_BLOCKS_PER_CU=2, weights, fp64 parameters) of hidden width `hid`, once per run."""
    if hid not in _CACHE:
        import xvector_amd as xa
        kw = _kw(hid)
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in xa.synth.make_state_dict(1300 + hid, **kw).items()}
        wide = make_model(sd, {"XVEC_WINO_SPLIT3_MIN_ROWS": "0"}, **kw)
        four = make_model(sd, {"XVEC_WINO_SPLIT3_MIN_ROWS": "0", "XVEC_BLOCKS_PER_CU": "2"}, **kw)
        _CACHE[hid] = (wide, four, sd, oracle.cast_params(float_params(sd), torch.float64))
    return _CACHE[hid]


def _names(m, layer, threads, what):
    assert m.last_forms()[layer] == "winograd_f23" and m.last_operands()[layer] == "bf16_split3", (what, m.last_forms(), m.last_operands())
    assert m.last_dispatch()[layer] == "tile128", (what, m.last_dispatch())
    thr, blocks = m.last_launches()[layer]
    assert thr == threads and blocks >= 1, (what, m.last_launches())
    return blocks


def _compare(synth, hid, B, T, wide_threads):
    wide, four, _, p64 = _handles(hid)
    h = wide.time_context_layers[0](torch.as_tensor(synth.make_mfcc(B, T, seed=7300 + 31 * B + T)).to(DEV))
    for layer in WINO_LAYERS:
        what = f"width {hid} layer {layer} B={B} T={T}"
        gw = wide.time_context_layers[layer](h)
        blocks = _names(wide, layer, wide_threads, what)
        g4 = four.time_context_layers[layer](h)
        _names(four, layer, 256, what)
        if wide_threads == 512:       # one block per CU over n_pad / 256 columns
            from xvector_amd import hip
            import ctypes
            lay = hip.WsLayout()
            hip.check(hip.lib.xvec_workspace_layout(wide._engine(torch.device(DEV)).h, B * T, B, ctypes.byref(lay)))
            assert blocks <= lay.num_cu and blocks % (lay.hidden_n_pad // 256) == 0, (what, blocks, lay.num_cu)
        assert torch.equal(gw, g4), f"{what}: {int((gw != g4).sum())} values differ between the two tilings"
        ref = oracle_layer(h.cpu(), p64, layer)
        for name, g in (("wide", gw), ("four-wave", g4)):
            err = worst_rel(g, ref)
            print(f"{what} {name}: worst-frame error {err:.3e}")
            assert_parity(g, ref.float(), 1e-4, f"{what} {name} vs oracle")
            assert err <= 1e-4, f"{what} {name}: worst-frame error {err:.3e}"
        assert torch.equal(gw, wide.time_context_layers[layer](h)), f"{what}: repeat launch differs"
        h = gw


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("hid", (256, 512))
def test_wide_equals_four_wave(synth, hid, B, T):
    _compare(synth, hid, B, T, 512)


@pytest.mark.parametrize("hid", (384, 32))
def test_fallback_to_four_waves(synth, hid):
    """A padded width that is no multiple of 256: the default handle runs the four-wave kernel and the record says so."""
    _compare(synth, hid, 3, 22, 256)


@pytest.mark.parametrize("hid", (256, 512))
def test_ragged_batch(synth, hid):
    wide, four, sd, _ = _handles(hid)
    T = max(RAGGED)
    x = synth.make_mfcc(len(RAGGED), T, seed=7400 + hid)
    for i, n in enumerate(RAGGED):
        x[i, n:] = np.nan
    xg = torch.as_tensor(x).to(DEV)
    gw = wide.extract_x_vec(xg, lengths=RAGGED)
    for layer in WINO_LAYERS:
        _names(wide, layer, 512, f"width {hid} ragged")
    g4 = four.extract_x_vec(xg, lengths=RAGGED)
    for layer in WINO_LAYERS:
        _names(four, layer, 256, f"width {hid} ragged")
    one = [i for i, n in enumerate(RAGGED) if n - 14 < 2]          # 15 frames pool ONE frame: 0 / 0 in the reference too
    fin = [i for i, n in enumerate(RAGGED) if n - 14 >= 2]
    assert torch.isnan(gw[one]).all() and torch.isfinite(gw[fin]).all()
    assert torch.equal(gw[fin], g4[fin]), f"width {hid}: ragged x-vectors differ between the two tilings"
    with torch.no_grad():
        ref = torch.stack([oracle.extract_x_vec(torch.from_numpy(x[i:i + 1, :RAGGED[i]]), float_params(sd))[0] for i in fin])
    assert_parity(gw[fin], ref, 1e-4, f"width {hid}: ragged x-vectors vs oracle")
    assert torch.equal(gw[fin], wide.extract_x_vec(xg, lengths=RAGGED)[fin]), f"width {hid}: ragged repeat run differs"
    # layer 3's compact rows as the whole path leaves them in the workspace (activation buffer A; the pooled mode runs no segment
    # layer, which would reuse it; layer 2's rows are overwritten by layer 4, and a wrong bit in them changes layer 3's)
    rows = [workspace_rows(m, xg, RAGGED, "a") for m in (wide, four)]
    assert torch.isfinite(rows[0]).all(), f"width {hid}: a layer-3 row was not written, or padding was read"
    assert torch.equal(rows[0], rows[1]), f"width {hid}: ragged layer-3 rows differ between the two tilings"


@pytest.mark.parametrize("hid", (256, 512))
def test_graph_replay(synth, hid):
    wide, four, _, _ = _handles(hid)
    x = torch.as_tensor(synth.make_mfcc(5, 77, seed=7500 + hid)).to(DEV)
    want = wide.extract_x_vec(x).clone()
    assert wide.last_launches()[1][0] == 512 and wide.last_launches()[2][0] == 512, wide.last_launches()
    assert torch.equal(want, four.extract_x_vec(x))
    graphed = wide.graphed(x)
    for _ in range(2):
        assert torch.equal(graphed(x), want), f"width {hid}: graph replay differs from the plain launch"
    torch.cuda.synchronize()
