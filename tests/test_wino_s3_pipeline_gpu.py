"""The pipelined K loop of the Winograd split3 kernel (csrc/tdnn_wino_s3.hip) at the smallest shapes where it can go wrong.

Hidden widths 32 and 64 give two and four 16-wide chunks per product (the kernel needs an even count), so the U look-ahead
wraps to chunk 0 in every second (every fourth) chunk.  Handles are created with XVEC_WINO_SPLIT3_MIN_ROWS=0, so the kernel
runs at these sizes (the operands label says so).

  * test_small_shapes: B = 1, 2, 3 at T = 15, 16, 21, 27 and B = 5 at T = 300.  At these widths a column has one block per
    32-pair group (the grid is min(2 x CUs, groups)), so every block here runs ONE tile of ONE pair group: the block prologue,
    the odd tail tile s3_tile<1>, pairs with one output, empty pair slots.
  * test_blocks_of_several_tiles: B = 288 at T = 300 with XVEC_BLOCKS_PER_CU=1: five or six 32-pair groups per block (asserted
    from the grid rule), i.e. two tiles of two pair groups and the odd tail, or three tiles of two -- s3_tile<2> with the
    barrier between its pair groups and the rolling fragment sets, the U stream's wrap across a tile boundary, the first
    fragments of the next tile read under the previous tile's last MFMAs and carried over the epilogue, the hand-over from a
    two-group tile to the tail, and at width 32 the row tables rewritten one tile ahead.
Every case of both, for layers 2 and 3: against the fp64 oracle at the project's 1e-4 bar; bit for bit against a second run and
against the same batch with its first utterance repeated at the end (the repeated utterance and every common one must come out
the same: a race in the LDS hand-over shows here); once more into an output buffer filled with NaN (every row is written).

  * test_ragged_batch: lengths 15, 16, 40, 299 with NaN in the padded frames, through the whole path (the only ragged entry).
    Layer 3's rows are read back from the workspace and must equal, bit for bit, what the per-layer entry gives for each
    utterance alone -- the same utterance at another batch position, in another row layout -- and those per-utterance
    layers 2 and 3 are checked against the fp64 oracle.  (Layer 2's ragged rows are overwritten by layer 4 before the call
    returns; a wrong bit in them changes layer 3's.)  Repeat run and NaN-filled workspace as above."""
import ctypes

import numpy as np
import pytest
import torch

import xvector_oracle as oracle
from conftest import assert_parity, float_params
from tdnn_support import DEV, make_model, oracle_layer, workspace_rows, worst_rel

pytestmark = pytest.mark.gpu
WINO_LAYERS = (1, 2)          # time_context_layers.1 / .2: contexts [-2, 0, 2] and [-3, 0, 3]
WIDTHS = (32, 64)
SHAPES = [(B, T) for B in (1, 2, 3) for T in (15, 16, 21, 27)] + [(5, 300)]
_CACHE = {}


def _kw(hid):
    return dict(input_size=24, hidden_size=hid, num_classes=7, x_vector_size=16, batch_norm=True)


def _handle(hid, blocks_per_cu=None):
    """Weights, fp64 parameters and the split3-everywhere handle of a model of hidden width `hid` (built once per run)."""
    env = {"XVEC_WINO_SPLIT3_MIN_ROWS": "0"}
    if blocks_per_cu is not None:
        env["XVEC_BLOCKS_PER_CU"] = str(blocks_per_cu)
        return (make_model(_handle(hid)[1], env, **_kw(hid)),) + _handle(hid)[1:]
    if hid not in _CACHE:
        import xvector_amd as xa
        kw = _kw(hid)
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in xa.synth.make_state_dict(900 + hid, **kw).items()}
        m = make_model(sd, env, **kw)
        _CACHE[hid] = (m, sd, oracle.cast_params(float_params(sd), torch.float64))
    return _CACHE[hid]


def _layer_into(m, index, x, y):
    """Layer `index` of `m` on x[B, T, C] into the caller's buffer y (the per-stage entry point of the library)."""
    from xvector_amd import hip
    from xvector_amd._device import stream
    eng = m._engine(torch.device(DEV))
    B, T, _ = x.shape
    ws, ws_bytes = eng.ensure_workspace(B * T, B)
    with torch.cuda.device(x.device):
        hip.check(hip.lib.xvec_tdnn_layer(eng.h, index, x.data_ptr(), B, T, hip.F32, y.data_ptr(), ws, ws_bytes, stream(x.device)))
    torch.cuda.synchronize()


def _check_layers(m, p64, synth, hid, B, T):
    h = m.time_context_layers[0](torch.as_tensor(synth.make_mfcc(B, T, seed=9700 + 31 * B + T)).to(DEV))
    for layer in WINO_LAYERS:
        what = f"width {hid} layer {layer} B={B} T={T}"
        g = m.time_context_layers[layer](h)
        assert m.last_forms()[layer] == "winograd_f23" and m.last_operands()[layer] == "bf16_split3", (what, m.last_operands())
        ref = oracle_layer(h.cpu(), p64, layer)
        err = worst_rel(g, ref)
        print(f"{what}: worst-frame error {err:.3e}")
        assert_parity(g, ref.float(), 1e-4, f"{what} vs oracle")
        assert err <= 1e-4, f"{what}: worst-frame error {err:.3e}"
        assert torch.equal(g, m.time_context_layers[layer](h)), f"{what}: repeat run differs"
        # the first utterance once more at the end of the batch
        hp = torch.cat([h, h[:1]])
        gp = m.time_context_layers[layer](hp)
        assert m.last_operands()[layer] == "bf16_split3"
        assert torch.equal(gp[:B], g), f"{what}: rows depend on the batch size"
        assert torch.equal(gp[B], g[0]), f"{what}: rows depend on the batch position"
        # every output row is written
        y = torch.full_like(g, float("nan"))
        _layer_into(m, layer, h.contiguous(), y)
        assert m.last_operands()[layer] == "bf16_split3"
        assert torch.equal(y, g), f"{what}: {int(torch.isnan(y).sum())} NaN left in a pre-filled output buffer"
        h = g


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("hid", WIDTHS)
def test_small_shapes(synth, hid, B, T):
    m, _, p64 = _handle(hid)
    _check_layers(m, p64, synth, hid, B, T)


def _layout(m, total, B):
    from xvector_amd import hip
    lay = hip.WsLayout()
    hip.check(hip.lib.xvec_workspace_layout(m._engine(torch.device(DEV)).h, total, B, ctypes.byref(lay)))
    return lay


def _pairs(t_out, d):
    """Winograd F(2,3) pairs of an utterance with t_out output frames at dilation d (csrc/tdnn_common.h, wino_pair_count)."""
    return d * (t_out // (2 * d)) + min(t_out % (2 * d), d)


@pytest.mark.parametrize("hid", WIDTHS)
def test_blocks_of_several_tiles(synth, hid):
    B, T = 288, 300
    m, _, p64 = _handle(hid, blocks_per_cu=1)
    # the grid rule (csrc/xvec_api.hip, persistent_grid; one 128-channel column at these widths): min(CUs x blocks per CU,
    # groups) blocks, the 32-pair groups dealt out in contiguous ranges whose sizes differ by at most one
    blocks = _layout(m, B * T, B).num_cu
    for t_out, d in ((T - 8, 2), (T - 14, 3)):
        for b in (B, B + 1):
            groups = -(-b * _pairs(t_out, d) // 32)
            assert 5 <= groups // blocks and -(-groups // blocks) <= 6, (groups, blocks)
    _check_layers(m, p64, synth, hid, B, T)


@pytest.mark.parametrize("hid", WIDTHS)
def test_ragged_batch(synth, hid):
    m, sd, p64 = _handle(hid)
    lens = [15, 16, 40, 299]
    T = max(lens)
    x = synth.make_mfcc(len(lens), T, seed=9800 + hid)
    # each utterance alone through the per-layer entry: layers 2 and 3 against the oracle, layer 3 kept
    alone = []
    for i, n in enumerate(lens):
        h = m.time_context_layers[0](torch.as_tensor(x[i:i + 1, :n]).to(DEV))
        for layer in WINO_LAYERS:
            g = m.time_context_layers[layer](h)
            assert m.last_operands()[layer] == "bf16_split3"
            err = worst_rel(g, oracle_layer(h.cpu(), p64, layer))
            print(f"width {hid} layer {layer} utterance of {n} frames: worst-frame error {err:.3e}")
            assert err <= 1e-4, f"width {hid} layer {layer} utterance of {n} frames: worst-frame error {err:.3e}"
            h = g
        alone.append(h[0])
    for i, n in enumerate(lens):
        x[i, n:] = np.nan
    xg = torch.as_tensor(x).to(DEV)
    off = np.concatenate([[0], np.cumsum([n - 14 for n in lens])])       # compact rows of layer 3's output

    def layer3_rows():
        """Layer 3's rows of the ragged batch as the whole path left them in the workspace (tdnn_support.workspace_rows)."""
        y = workspace_rows(m, xg, lens, "a")
        assert m.last_forms()[1:3] == ["winograd_f23"] * 2 and m.last_operands()[1:3] == ["bf16_split3"] * 2, m.last_operands()
        assert y.shape[0] == int(off[-1])
        return y

    y = layer3_rows()
    assert torch.isfinite(y).all(), "ragged: a layer-3 row was not written, or a row that no layer wrote was read"
    for i, n in enumerate(lens):
        assert torch.equal(y[off[i]:off[i + 1]], alone[i]), f"ragged: layer 3 of the utterance of {n} frames differs from the utterance alone"
    assert torch.equal(y, layer3_rows()), "ragged: repeat run differs"
    # the whole path: 15 frames pool ONE frame, whose standard deviation (torch.std, unbiased) is 0 / 0 in the reference too
    g = m.extract_x_vec(xg, lengths=lens)
    with torch.no_grad():
        ref = torch.stack([oracle.extract_x_vec(torch.from_numpy(x[i:i + 1, :n]), float_params(sd))[0] for i, n in enumerate(lens)])
    fin = [i for i, n in enumerate(lens) if n - 14 >= 2]
    one = [i for i, n in enumerate(lens) if n - 14 < 2]
    assert torch.isnan(ref[one]).all() and torch.isnan(g[one]).all()
    assert torch.isfinite(g[fin]).all()
    assert_parity(g[fin], ref[fin], 1e-4, f"width {hid}: ragged x-vectors vs oracle")
