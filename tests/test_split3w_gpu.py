"""fp32 layer 5 (bf16_split3, pooling) on 384-channel tiles (csrc/tdnn_split3w.hip: twelve waves, one block per CU, two of the
three wave sets staging alternate chunks) against the four-wave kernel (csrc/tdnn_split3.hip), which computes every product in
the same order over the same row ranges: the pooled statistics must be the same BITS, and both must meet the fp64 oracle.

Handles over the same weights (split3w_support.make_model: tdnn_support's with the wide tile's two knobs set or cleared around
it): wide = XVEC_SPLIT3_MIN_ROWS=0 + XVEC_SPLIT3_WIDE_MIN_ROWS=0 (the wide tile at every size), narrow = the same +
XVEC_SPLIT3_WIDE=0.  Which kernel layer 5 went to is read from the launch record (last_launches: 768 threads = the wide kernel, 256 = the four-wave one); form, operands and kernel family read as before.

  widths   32, 256, 384, 512: K loops of 2, 8, 12 and 16 chunks (two: the weight reload and both staging streams wrap to the
           next tile on every chunk); N is 1500 padded to 1536 = 4 x 384 at every width
  batches  B = 1, T = 15       one row: fewer groups than blocks, one frame per utterance (the std is 0 / 0 = NaN, as the
                               reference's)
           B = 3, T = 21, 22   one 32-row group holding three utterances
           B = 8, T = 20       48 rows, two groups, masked partials
           B = 40, T = 300     358 groups over CUs / 4 blocks per column: 5-6 per block at 256 CUs, a full tile + 1 or 2
           B = 50, T = 300     447 groups, 6-7 per block: a full tile + 2 or 3
           ragged (15, 40, 16, 133) with NaN in the padding, through the whole path
  bounds   pooled statistics against the oracle as tests/test_batchnorm_checkpoint_gpu.py holds the same quantity: rows and
           means at 1e-4, the elements of the stds at 1e-3 from 64 frames on and 5e-2 below (nearly-off channels: conftest.py,
           nearly_off_channels); x-vectors at 1e-4
  replay   a repeated launch and a graph replay give the same bits
  fallback XVEC_BLOCKS_PER_CU = 1, 2, 3, XVEC_SPLIT3_WIDE=0 and a default threshold above the batch keep the four-wave kernel"""
import numpy as np
import pytest
import torch

import xvector_oracle as oracle
from conftest import assert_parity, float_params
from split3w_support import make_model
from tdnn_support import DEV, layer_input, oracle_layer, workspace_layout, worst_rel

pytestmark = pytest.mark.gpu
WIDTHS = (32, 256, 384, 512)
SHAPES = [(1, 15), (3, 21), (3, 22), (8, 20), (40, 300), (50, 300)]
RAGGED = [15, 40, 16, 133]
ALWAYS = {"XVEC_SPLIT3_MIN_ROWS": "0", "XVEC_SPLIT3_WIDE_MIN_ROWS": "0"}
_CACHE = {}
_REF = {}


def _kw(hid):
    return dict(input_size=24, hidden_size=hid, num_classes=7, x_vector_size=16, batch_norm=True)


def _handles(hid):
    """(wide handle, narrow handle, weights, fp64 parameters) of hidden width `hid`, once per run."""
    if hid not in _CACHE:
        import xvector_amd as xa
        kw = _kw(hid)
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in xa.synth.make_state_dict(2300 + hid, **kw).items()}
        wide = make_model(sd, ALWAYS, **kw)
        narrow = make_model(sd, dict(ALWAYS, XVEC_SPLIT3_WIDE="0"), **kw)
        _CACHE[hid] = (wide, narrow, sd, oracle.cast_params(float_params(sd), torch.float64))
    return _CACHE[hid]


def _record(m, threads, what):
    """Layer 5's launch record: the names the split form reports, `threads` per block; returns the blocks."""
    assert m.last_forms()[4] == "bf16_split3" and m.last_operands()[4] == "bf16_split3", (what, m.last_forms(), m.last_operands())
    assert m.last_dispatch()[4] == "tile128", (what, m.last_dispatch())
    thr, blocks = m.last_launches()[4]
    assert thr == threads and blocks >= 1, (what, m.last_launches())
    return blocks


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _case(synth, hid, B, T):
    """Layer 4's output of the batch and the oracle's pooled statistics of it, computed once and shared."""
    key = (hid, B, T)
    if key not in _REF:
        _, narrow, _, p64 = _handles(hid)
        g4 = layer_input(narrow, synth, B, T, 4, 8100 + 31 * B + T)
        _REF[key] = (g4, oracle.stat_pool(oracle_layer(g4.cpu(), p64, 4)))
    return _REF[key]


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("hid", WIDTHS)
def test_wide_equals_four_wave(synth, hid, B, T):
    wide, narrow, sd, _ = _handles(hid)
    what = f"width {hid} B={B} T={T}"
    g4, ref_p = _case(synth, hid, B, T)
    n, C = T - 14, ref_p.shape[1] // 2
    pw = wide.pooled_last_layer(g4)
    blocks = _record(wide, 768, what)
    cus = workspace_layout(wide, B * T, B).num_cu
    assert blocks % 4 == 0 and blocks <= max(4, cus // 4 * 4), (what, blocks, cus)      # one block per CU over four columns
    pn = narrow.pooled_last_layer(g4)
    assert _record(narrow, 256, what) % 12 == 0
    for name, p in (("wide", pw), ("four-wave", pn)):      # every figure before the first assertion
        print(f"{what} {name}: pooled means vs oracle {worst_rel(p[:, :C], ref_p[:, :C]):.3e}"
              + (f", pooled rows {worst_rel(p, ref_p):.3e}" if n >= 2 else ""))
    assert _same_bits(pw, pn), f"{what}: {int((pw.view(torch.int32) != pn.view(torch.int32)).sum())} pooled values differ between the two tilings"
    for name, p in (("wide", pw), ("four-wave", pn)):
        assert_parity(p[:, :C], ref_p[:, :C], 1e-4, f"{what} {name}: pooled means vs oracle")
        if n >= 2:
            assert_parity(p, ref_p, 1e-4, f"{what} {name}: pooled statistics vs oracle", elem_tol=1e-3 if n >= 64 else 5e-2)
        else:
            assert torch.isnan(p[:, C:]).all() and torch.isnan(ref_p[:, C:]).all(), f"{what} {name}: std of one frame"
    assert _same_bits(pw, wide.pooled_last_layer(g4)), f"{what}: repeat launch differs"
    # the whole path: x-vectors of a few utterances against the oracle, repeat run, graph replay
    x = synth.make_mfcc(B, T, seed=8100 + 31 * B + T)
    idx = list(range(0, B, max(1, B // 12)))
    xg = torch.as_tensor(x).to(DEV)
    ew = wide.extract_x_vec(xg)
    _record(wide, 768, what)
    en = narrow.extract_x_vec(xg)
    _record(narrow, 256, what)
    assert _same_bits(ew, en), f"{what}: x-vectors differ between the two tilings"
    if n >= 2:
        with torch.no_grad():
            ref = oracle.extract_x_vec(torch.from_numpy(x[idx]), float_params(sd))
        print(f"{what}: x-vectors vs oracle {worst_rel(ew[idx], ref.double()):.3e}")
        assert_parity(ew[idx], ref, 1e-4, f"{what}: x-vectors vs oracle")
    else:
        assert torch.isnan(ew).all(), f"{what}: x-vectors of one pooled frame"
    assert _same_bits(wide.extract_x_vec(xg), ew), f"{what}: repeat run differs"
    out = wide.graphed(xg)(xg).clone()
    torch.cuda.synchronize()
    assert _same_bits(out, ew), f"{what}: graph replay differs from the plain launch"


@pytest.mark.parametrize("hid", WIDTHS)
def test_ragged_batch(synth, hid):
    wide, narrow, sd, _ = _handles(hid)
    x = synth.make_mfcc(len(RAGGED), max(RAGGED), seed=8400 + hid)
    for i, n in enumerate(RAGGED):
        x[i, n:] = np.nan
    xg = torch.as_tensor(x).to(DEV)
    gw = wide.extract_x_vec(xg, lengths=RAGGED)
    _record(wide, 768, f"width {hid} ragged")
    gn = narrow.extract_x_vec(xg, lengths=RAGGED)
    _record(narrow, 256, f"width {hid} ragged")
    one = [i for i, n in enumerate(RAGGED) if n - 14 < 2]          # 15 frames pool ONE frame: 0 / 0 in the reference too
    fin = [i for i, n in enumerate(RAGGED) if n - 14 >= 2]
    assert torch.isnan(gw[one]).all() and torch.isfinite(gw[fin]).all()
    assert _same_bits(gw, gn), f"width {hid}: ragged x-vectors differ between the two tilings"
    assert _same_bits(wide.pooled(xg, lengths=RAGGED), narrow.pooled(xg, lengths=RAGGED)), f"width {hid}: ragged pooled statistics differ"
    with torch.no_grad():
        ref = torch.stack([oracle.extract_x_vec(torch.from_numpy(x[i:i + 1, :RAGGED[i]]), float_params(sd))[0] for i in fin])
    print(f"width {hid} ragged: x-vectors vs oracle {worst_rel(gw[fin], ref.double()):.3e}")
    assert_parity(gw[fin], ref, 1e-4, f"width {hid}: ragged x-vectors vs oracle")
    assert _same_bits(gw, wide.extract_x_vec(xg, lengths=RAGGED)), f"width {hid}: ragged repeat run differs"


@pytest.mark.parametrize("env", [dict(ALWAYS, XVEC_BLOCKS_PER_CU="1"), dict(ALWAYS, XVEC_BLOCKS_PER_CU="2"),
                                 dict(ALWAYS, XVEC_BLOCKS_PER_CU="3"), dict(ALWAYS, XVEC_SPLIT3_WIDE="0"),
                                 {"XVEC_SPLIT3_MIN_ROWS": "0"}],
                         ids=["blocks_per_cu_1", "blocks_per_cu_2", "blocks_per_cu_3", "wide_off", "below_default_threshold"])
def test_fallback_to_four_waves(synth, env):
    """Settings under which the planner keeps layer 5 on the four-wave kernel: the record says 256 threads, the bits stay."""
    hid, B, T = 256, 8, 20
    wide, _, sd, _ = _handles(hid)
    m = make_model(sd, env, **_kw(hid))
    g4, _ = _case(synth, hid, B, T)
    p = m.pooled_last_layer(g4)
    _record(m, 256, str(env))
    assert _same_bits(p, wide.pooled_last_layer(g4)), f"{env}: pooled statistics differ from the wide tile's"
    _record(wide, 768, str(env))
