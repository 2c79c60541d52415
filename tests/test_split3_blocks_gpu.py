"""fp32 layers 4 and 5 as bf16_split3 at three blocks per CU (csrc/tdnn_split3.hip; the body is XV_S3_CHUNK of
csrc/tdnn_layer_impl.h): one staging set with a chunk of lead, six weight fragments reloaded in place, two rolling sets of three
activation fragments, the LDS buffers packed at 24 KiB, and a grid the planner sizes per kernel (csrc/xvec_api.hip,
persistent_grid).

Handles with XVEC_SPLIT3_MIN_ROWS=0 (the split form at every size) and XVEC_BLOCKS_PER_CU unset, 3, 2 and 1, at hidden widths
512, 72 and 32: 16, 4 and 2 K chunks per tile -- with two, the in-place weight reload wraps to chunk 0 on every other chunk.
  * test_small_shapes, test_small_shapes_pooling: B = 1, 2, 3 at T = 16, 21, 47 (2, 7 and 33 frames per utterance behind
    layer 3): one to four 32-row groups, one block each -- the block prologue, the tail tiles G < 4 with rows past the batch,
    the first-tile pooling pivot.  Widths 72 and 32 at B = 3.
  * test_default_grid: B = 64 at T = 300, 572 groups: 2-3 per block in layer 4 and 8-9 in layer 5 at three blocks per CU.
  * test_several_tiles_per_block: B = 40 at T = 300 with XVEC_BLOCKS_PER_CU=1, 358 groups: 5-6 per block in layer 4 and about
    17 in layer 5 (asserted from the grid rule) -- the weight and staging streams run across tile boundaries.
  * test_ragged_batch: lengths 200-1000 through the whole path, NaN in the padded frames.
What every case asserts: layer 4's stored output is the same bit for bit under all four settings (the products reach each
accumulator in one order whatever the grid) and at the fp32 bar against the fp64 oracle; layer 5's pooled statistics within
1e-5 of the direct form's (XVEC_SPLIT3=0) on the same input; the x-vectors at the fp32 bar against the oracle; a repeat run and
a graph replay bit for bit the first run; the forms, dispatch and operands the split form reports.

test_small_shapes_pooling is also what holds the pooling pivots of the two forms to one rule (process_tile: K cut to 8 bits in
every form).  A channel that is off in an utterance but on in the frame its block took the pivot K from contributes n equal
terms -K; with a 24-bit K pool_finalize forms a second moment of 0 or ~(3e-4 K)^2 from the rounded sums, by K's last bits
(tests/conftest.py, assert_parity_masked, describes the same), and at these shapes that put one or two standard deviations of
a batch's B x 1500 outside the element-wise part of the 1e-5 bound (atol 2.2e-6 = 1e-5 of the mean |value|) while the rows
agreed to 4e-7: 1.70e-5 in one form against exactly 0 in the other, [512-2-47], [512-3-16] and [32-3-16] with 24-bit pivots in
both forms, [512-2-16], [512-3-16], [72-3-21] and [32-3-16] with the cut in the split form alone."""
import ctypes

import numpy as np
import pytest
import torch

import xvector_oracle as oracle
from conftest import assert_parity, float_params
from tdnn_support import DEV, layer_input, make_model, oracle_layer, worst_rel

pytestmark = pytest.mark.gpu
WIDTHS = (512, 72, 32)
SETTINGS = (None, 3, 2, 1)          # XVEC_BLOCKS_PER_CU of a handle; None: unset
SMALL = [(512, B, T) for B in (1, 2, 3) for T in (16, 21, 47)] + [(hid, 3, T) for hid in (72, 32) for T in (16, 21, 47)]
_CACHE = {}


def _kw(hid):
    return {} if hid == 512 else dict(input_size=24, hidden_size=hid, num_classes=7, x_vector_size=16, batch_norm=True)


def _models(hid, sd42):
    """{setting: handle in the split form at every size} of a model of hidden width `hid`, its direct-form handle, its weights
    and their fp64 copy (built once per run; width 512: the seed-42 weights)."""
    if hid not in _CACHE:
        import xvector_amd as xa
        kw = _kw(hid)
        sd = sd42 if hid == 512 else {k: torch.from_numpy(np.asarray(v)) for k, v in xa.synth.make_state_dict(700 + hid, **kw).items()}
        ms = {}
        for s in SETTINGS:
            env = {"XVEC_SPLIT3_MIN_ROWS": "0"}
            if s is not None:
                env["XVEC_BLOCKS_PER_CU"] = str(s)
            ms[s] = make_model(sd, env, **kw)
        _CACHE[hid] = (ms, make_model(sd, {"XVEC_SPLIT3": "0"}, **kw), sd, oracle.cast_params(float_params(sd), torch.float64))
    return _CACHE[hid]


def _num_cu(m, total, B):
    from xvector_amd import hip
    lay = hip.WsLayout()
    hip.check(hip.lib.xvec_workspace_layout(m._engine(torch.device(DEV)).h, total, B, ctypes.byref(lay)))
    return lay.num_cu


def _assert_layer(m, layer):
    assert m.last_forms()[layer] == "bf16_split3" and m.last_dispatch()[layer] == "tile128", (m.last_forms(), m.last_dispatch())
    assert m.last_operands()[layer] == "bf16_split3", m.last_operands()


def _assert_path(m, hid):
    assert m.last_forms()[3:] == ["bf16_split3"] * 2 and m.last_operands()[3:] == ["bf16_split3"] * 2, m.last_forms()
    assert m.last_dispatch() == ["tile128"] * 5, m.last_dispatch()
    if hid == 512:
        assert m.last_forms() == ["direct", "winograd_f23", "winograd_f23", "bf16_split3", "bf16_split3"], m.last_forms()


def _layer4(synth, sd42, hid, B, T, seed):
    """Layer 4 of the batch: one result under every setting, at the fp32 bar; returns it."""
    ms, md, _, p64 = _models(hid, sd42)
    what = f"width {hid} B={B} T={T}"
    h = layer_input(md, synth, B, T, 3, seed)
    g4 = {}
    for s, m in ms.items():
        g4[s] = m.time_context_layers[3](h)
        _assert_layer(m, 3)
        assert torch.equal(g4[s], m.time_context_layers[3](h)), f"{what}, {s} blocks per CU: layer 4 repeat run differs"
    for s in SETTINGS[1:]:
        assert torch.equal(g4[s], g4[None]), f"{what}: layer 4 at XVEC_BLOCKS_PER_CU={s} differs from the default grid's"
    ref4 = oracle_layer(h.cpu(), p64, 3)
    print(f"{what}: layer 4 worst-frame error {worst_rel(g4[None], ref4):.3e}")
    assert_parity(g4[None], ref4.float(), 1e-4, f"{what}: layer 4 vs oracle")
    return g4[None]


def _pooling(sd42, hid, g4, what):
    """Layer 5 with the pooling epilogue on layer 4's rows, under every setting, against the direct form."""
    ms, md, _, _ = _models(hid, sd42)
    pd = md.pooled_last_layer(g4)
    assert md.last_forms()[4] == "direct"
    pooled = {s: m.pooled_last_layer(g4) for s, m in ms.items()}
    for s in ms:      # every figure before the first assertion
        print(f"{what}, {s} blocks per CU: pooled statistics vs direct {worst_rel(pooled[s], pd.double().cpu()):.3e}")
    for s, m in ms.items():
        assert_parity(pooled[s], pd, 1e-5, f"{what}, {s} blocks per CU: pooled statistics, split3 vs direct")
        assert torch.equal(pooled[s], m.pooled_last_layer(g4)), f"{what}, {s} blocks per CU: pooling repeat run differs"
        _assert_layer(m, 4)


def _whole_path(synth, sd42, hid, B, T, seed, settings):
    """x-vectors of the batch against the oracle (a few utterances of a large batch), repeat run, graph replay."""
    ms, _, sd, _ = _models(hid, sd42)
    x = synth.make_mfcc(B, T, seed=seed)
    idx = list(range(0, B, max(1, B // 8)))
    with torch.no_grad():
        ref = oracle.extract_x_vec(torch.from_numpy(x[idx]), float_params(sd))
    xg = torch.as_tensor(x).to(DEV)
    for s in settings:
        m, what = ms[s], f"width {hid} B={B} T={T}, {s} blocks per CU"
        e = m.extract_x_vec(xg)
        _assert_path(m, hid)
        print(f"{what}: x-vectors vs oracle {worst_rel(e[idx], ref.double()):.3e}")
        assert_parity(e[idx], ref, 1e-4, f"{what}: x-vectors vs oracle")
        assert torch.equal(m.extract_x_vec(xg), e), f"{what}: repeat run differs"
        out = m.graphed(xg)(xg).clone()
        torch.cuda.synchronize()
        assert torch.equal(out, e), f"{what}: graph replay differs from eager"


@pytest.mark.parametrize("hid,B,T", SMALL)
def test_small_shapes(synth, sd42, hid, B, T):
    _layer4(synth, sd42, hid, B, T, 7100 + 31 * B + T)
    _whole_path(synth, sd42, hid, B, T, 7100 + 31 * B + T, SETTINGS)


@pytest.mark.parametrize("hid,B,T", SMALL)
def test_small_shapes_pooling(synth, sd42, hid, B, T):
    """Layer 5's pooled statistics at the same shapes."""
    ms, md, _, _ = _models(hid, sd42)
    g4 = ms[None].time_context_layers[3](layer_input(md, synth, B, T, 3, 7100 + 31 * B + T))
    _pooling(sd42, hid, g4, f"width {hid} B={B} T={T}")


def test_default_grid(synth, sd42):
    B, T = 64, 300
    m = _models(512, sd42)[0][None]
    cus, groups = _num_cu(m, B * T, B), -(-B * (T - 14) // 32)
    if cus == 256:       # the grid rule (persistent_grid): three blocks per CU over 4 (layer 4) and 12 (layer 5) columns
        assert groups == 572 and 2 <= groups // (3 * cus // 4) and -(-groups // (3 * cus // 4)) <= 3
        assert 8 <= groups // (3 * cus // 12) and -(-groups // (3 * cus // 12)) <= 9
    _pooling(sd42, 512, _layer4(synth, sd42, 512, B, T, 7300), f"width 512 B={B} T={T}")
    _whole_path(synth, sd42, 512, B, T, 7300, (None,))


@pytest.mark.parametrize("hid", WIDTHS)
def test_several_tiles_per_block(synth, sd42, hid):
    B, T = 40, 300
    m = _models(hid, sd42)[0][1]
    cus, groups = _num_cu(m, B * T, B), -(-B * (T - 14) // 32)
    if cus == 256 and hid == 512:
        assert 5 <= groups // (cus // 4) and -(-groups // (cus // 4)) <= 6
        assert 16 <= groups // (cus // 12) and -(-groups // (cus // 12)) <= 18
    assert groups >= 5 * (cus // 12), "several four-group tiles per block in layer 5"
    _pooling(sd42, hid, _layer4(synth, sd42, hid, B, T, 7400 + hid), f"width {hid} B={B} T={T}")
    _whole_path(synth, sd42, hid, B, T, 7400 + hid, (1,))


def test_ragged_batch(synth, sd42):
    ms, md, sd, _ = _models(512, sd42)
    lens = [200, 1000, 333, 517, 764, 250, 901, 640]
    x = synth.make_mfcc(len(lens), max(lens), seed=7500)
    with torch.no_grad():
        ref = torch.stack([oracle.extract_x_vec(torch.from_numpy(x[i:i + 1, :n]), float_params(sd))[0] for i, n in enumerate(lens)])
    for i, n in enumerate(lens):
        x[i, n:] = np.nan
    xg = torch.as_tensor(x).to(DEV)
    gd = md.extract_x_vec(xg, lengths=lens)
    assert md.last_forms()[3:] == ["direct", "direct"]
    for s, m in ms.items():
        g = m.extract_x_vec(xg, lengths=lens)
        _assert_path(m, 512)
        print(f"ragged, {s} blocks per CU: vs oracle {worst_rel(g, ref.double()):.3e}, vs direct {worst_rel(g, gd.double().cpu()):.3e}")
        assert_parity(g, ref, 1e-4, f"ragged, {s} blocks per CU: x-vectors vs oracle")
        assert_parity(g, gd, 1e-5, f"ragged, {s} blocks per CU: split3 vs direct")
        assert torch.equal(m.extract_x_vec(xg, lengths=lens), g), f"ragged, {s} blocks per CU: repeat run differs"
