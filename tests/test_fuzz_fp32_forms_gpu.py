"""Seeded ragged and fixed-length batches through every fp32 kernel form of the frame-level layers, row by row.

Four handles on the seed-42 weights (width 512), each under the knobs that pin one set of forms:
  D    XVEC_WINOGRAD=0, XVEC_SPLIT3=0                          every layer the direct 128x128 kernel, fp32 operands
  W    XVEC_WINO_SPLIT3=0, XVEC_SPLIT3=0                       layers 2-3 fp32 Winograd F(2,3) (csrc/tdnn_wino.hip)
  S4   XVEC_WINO_SPLIT3_MIN_ROWS=0, XVEC_SPLIT3_MIN_ROWS=0,    layers 2-3 Winograd on bf16_split3 operands, four waves
       XVEC_BLOCKS_PER_CU=2                                    (tdnn_wino_s3.hip); layers 4-5 bf16_split3 at two blocks per CU
  S8   XVEC_WINO_SPLIT3_MIN_ROWS=0, XVEC_SPLIT3_MIN_ROWS=0     the same on eight waves and 256-channel tiles (tdnn_wino_s3w.hip);
                                                               layers 4-5 bf16_split3 at three blocks per CU (tdnn_split3.hip)
After EVERY library call the launch record is held to the handle's forms, operands, kernel family and block size, and its block
count to the grid that tests/fp32_forms_ref.py -- the host restatement of the planner's and the kernels' geometry -- gives for
the device's CU count: that ties the restatement, and with it the classes K1..K10 that tests/test_fuzz_fp32_forms.py shows the
default case list to reach, to what ran.

The cases come from fp32_forms_ref.cases (FUZZ_N / FUZZ_SEED: a longer walk by hand; FUZZ_LOG=file appends one JSON line per
case -- profiles/fp32_forms_fuzz.txt is the summary of such walks): tiny batches, many short utterances (a tile of 64 Winograd
pairs holds a dozen of them; the deep ones make a block walk several tiles) and mid-sized ones, two thirds ragged with NaN in
every padded frame, an utterance of 15 frames (one pooled frame: NaN std here and in the reference) and one of 16.

Per case and handle:
  * every row written: layer 3's and layer 4's compact rows, read back from a workspace pre-filled with 0xFF bytes
    (tdnn_support.workspace_rows), are all finite; fixed-length cases also run layers 2-4 through the per-layer entry into a
    NaN-filled output.  (In the workspace the finite check alone is weak -- a skipped row holds layer 1's or layer 2's values,
    and a NaN read is 0 behind the ReLU; the build without the j0 clamp of profiles/fp32_forms_fuzz.txt passed it and was
    caught by the next check, which therefore covers EVERY row;)
  * every row of every utterance against the fp64 oracle chained per utterance on the un-padded slice, at the project's bar:
    worst norm-wise frame error <= 1e-4 and assert_parity(..., 1e-4);
  * the same bits where the kernels promise them: S8's layer-3 and layer-4 rows equal S4's, and a repeat run equals the first
    on the rows and on the pooled statistics;
  * position independence: utterances run alone (B = 1) through time_context_layers[0..3] of the same handle -- first, last,
    shortest, longest, three drawn from the seed and every utterance that starts in a Winograd tile classified K3 (first pair
    in a hole) or K4a (three starts or more) -- give, bit for bit, their layer-3 and layer-4 rows of the batch;
  * pooled statistics and x-vectors of every utterance against the oracle at the bars of test_random_shapes_fp32_vs_oracle
    (means 1e-4; stds 1e-4 norm-wise, element-wise 1e-3 from 64 frames on and 5e-2 below; x-vectors 1e-4 / 1e-3), NaN exactly
    where the oracle has NaN.

The plan this file was written to assumed that the many-short family makes a four-wave block run several tiles under a cap of
12 000 layer-1 rows.  It does not at 256 CUs: see DEEP_ROW_CAP in fp32_forms_ref.py, which is what every second case of that
family runs under instead."""
import json
import os

import numpy as np
import pytest
import torch

import fp32_forms_ref as ref
import xvector_oracle as oracle
from conftest import assert_parity
from tdnn_support import DEV, make_model, p64, workspace_layout, workspace_rows, worst_rel  # noqa: F401 (p64: a fixture)

pytestmark = pytest.mark.gpu
KNOBS = {"D": {"XVEC_WINOGRAD": "0", "XVEC_SPLIT3": "0"},
         "W": {"XVEC_WINO_SPLIT3": "0", "XVEC_SPLIT3": "0"},
         "S4": {"XVEC_WINO_SPLIT3_MIN_ROWS": "0", "XVEC_SPLIT3_MIN_ROWS": "0", "XVEC_BLOCKS_PER_CU": "2"},
         "S8": {"XVEC_WINO_SPLIT3_MIN_ROWS": "0", "XVEC_SPLIT3_MIN_ROWS": "0"}}
CASES = ref.cases(int(os.environ.get("FUZZ_N", ref.DEFAULT_N)), int(os.environ.get("FUZZ_SEED", ref.DEFAULT_SEED)))
HIDDEN = 512


@pytest.fixture(scope="module")
def handles(sd42):
    return {f: make_model(sd42, KNOBS[f]) for f in ref.FORMS}


@pytest.fixture(scope="module")
def num_cu(handles):
    return workspace_layout(handles["D"], 15, 1).num_cu


def _check_record(m, form, lengths, fixed, num_cu, layers, what):
    """The launch record of `layers` after a call on the batch `lengths`: names, block size, and the restatement's grid."""
    forms, ops, thr = ref.expected_record(form)
    got_f, got_o, got_d, got_l = m.last_forms(), m.last_operands(), m.last_dispatch(), m.last_launches()
    for l in layers:
        grid = ref.layer_grid(form, l, lengths, num_cu, HIDDEN, fixed)
        assert (got_f[l], got_o[l], got_d[l]) == (forms[l], ops[l], "tile128"), (what, form, l, got_f, got_o, got_d)
        assert got_l[l] == (thr[l], grid.blocks), f"{what} {form} layer index {l}: launched {got_l[l]}, restated {(thr[l], grid)}"


def _oracle(x, lengths, p64):
    """fp64 oracle per utterance on the un-padded slice (utterances of one length share a call): layer-3 rows, layer-4 rows,
    pooled statistics [B, 3000] and x-vectors [B, 512]."""
    lengths = np.asarray(lengths)
    B = len(lengths)
    r3, r4, pooled, xv = [None] * B, [None] * B, [None] * B, [None] * B
    with torch.no_grad():
        for n in sorted(set(lengths.tolist())):
            idx = np.flatnonzero(lengths == n)
            for lo in range(0, len(idx), 32):
                ii = idx[lo:lo + 32]
                h = torch.from_numpy(x[ii, :n]).double()
                for l in range(5):
                    h = oracle.tdnn_layer(h, p64, f"time_context_layers.{l}.", oracle.CONTEXTS[l], True)
                    if l == 2:
                        h3 = h
                    if l == 3:
                        h4 = h
                pl = oracle.stat_pool(h)
                xs = pl @ p64["segment_layer6.weight"].t() + p64["segment_layer6.bias"]
                for k, i in enumerate(ii):
                    r3[i], r4[i], pooled[i], xv[i] = h3[k], h4[k], pl[k], xs[k]
    return torch.cat(r3), torch.cat(r4), torch.stack(pooled), torch.stack(xv)


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


def _alone_set(case, marked, rng):
    lengths, B = case.lengths, len(case.lengths)
    base = {0, B - 1, int(np.argmin(lengths)), int(np.argmax(lengths))} | {int(v) for v in rng.integers(0, B, 3)}
    return sorted(base | set(marked))


def _stats_vs_oracle(got_p, got_x, ref_p, ref_x, lengths, what):
    n = torch.as_tensor(lengths)
    assert torch.equal(torch.isnan(got_p), torch.isnan(ref_p)), f"{what}: pooled NaN pattern differs from the oracle's"
    assert torch.equal(torch.isnan(got_x), torch.isnan(ref_x)), f"{what}: x-vector NaN pattern differs from the oracle's"
    assert bool((torch.isnan(ref_p[:, 1500:]).all(dim=1) == (n == 15)).all()) and not torch.isnan(ref_p[:, :1500]).any()
    assert_parity(got_p[:, :1500], ref_p[:, :1500], 1e-4, f"{what} means")
    for sel, et in (((n >= 64), 1e-3), ((n < 64) & (n > 15), 5e-2)):
        if sel.any():
            assert_parity(got_p[sel, 1500:], ref_p[sel, 1500:], 1e-4, f"{what} stds ({'>=' if et == 1e-3 else '<'} 64 frames)", elem_tol=et)
    if (n > 15).any():
        assert_parity(got_x[n > 15], ref_x[n > 15], 1e-4, f"{what} x-vectors", elem_tol=1e-3)


@pytest.mark.filterwarnings("ignore:std\\(\\)")          # the oracle's torch.std of the one pooled frame of a 15-frame utterance
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[f"{i}-{c.family}-{'fixed' if c.fixed else 'ragged'}-B{len(c.lengths)}"
                                                        for i, c in enumerate(CASES)])
def test_case(handles, p64, synth, num_cu, ci):
    case = CASES[ci]
    lengths, B, T = case.lengths, len(case.lengths), max(case.lengths)
    arg = None if case.fixed else lengths
    what = f"case {ci} ({case.family}, {'fixed' if case.fixed else 'ragged'}, B={B}, T={T})"
    x = synth.make_mfcc(B, T, seed=case.seed % 100000)
    ref3, ref4, ref_p, ref_x = _oracle(x, lengths, p64)
    for i, n in enumerate(lengths):
        x[i, n:] = np.nan                                             # (a fixed-length batch has no padded frame)
    xg = torch.as_tensor(x).to(DEV)
    off = np.concatenate([[0], np.cumsum(np.asarray(lengths) - 14)])
    rows, errs, log = {}, {}, {"case": ci, "family": case.family, "fixed": case.fixed, "B": B, "T": T,
                               "rows_l1": int(sum(lengths) - 4 * B), "num_cu": num_cu, "classes": {}, "errors": {}, "alone": {}}
    for form in ref.FORMS:
        m = handles[form]
        counts, marked = ref.classify(lengths, num_cu, form, HIDDEN, case.fixed)
        log["classes"][form] = {k: int(v) for k, v in counts.items() if v}
        # every row written, twice the same bits
        y3, y4 = workspace_rows(m, xg, arg, "ab")
        _check_record(m, form, lengths, case.fixed, num_cu, range(5), what)
        assert torch.isfinite(y3).all(), f"{what} {form}: a layer-3 row was not written, or padding was read"
        assert torch.isfinite(y4).all(), f"{what} {form}: a layer-4 row was not written, or padding was read"
        got_p = m.pooled(xg, lengths=arg)
        _check_record(m, form, lengths, case.fixed, num_cu, range(5), what)
        z3, z4 = workspace_rows(m, xg, arg, "ab")
        assert torch.equal(y3, z3) and torch.equal(y4, z4), f"{what} {form}: the rows of a repeat run differ"
        assert torch.equal(got_p.view(torch.int32), m.pooled(xg, lengths=arg).view(torch.int32)), f"{what} {form}: pooled repeat run differs"
        got_x = m.extract_x_vec(xg, lengths=arg)
        _check_record(m, form, lengths, case.fixed, num_cu, range(5), what)
        rows[form] = (y3, y4)
        # every row against the oracle
        for name, y, r in (("layer 3", y3, ref3), ("layer 4", y4, ref4)):
            err = errs[(form, name)] = worst_rel(y, r)
            print(f"{what} {form} {name}: worst-frame error {err:.3e} over {y.shape[0]} rows")
            assert err <= 1e-4, f"{what} {form} {name}: worst-frame error {err:.3e}"
            assert_parity(y, r, 1e-4, f"{what} {form} {name} vs oracle")
        log["errors"][form] = {"layer3": errs[(form, "layer 3")], "layer4": errs[(form, "layer 4")]}
        _stats_vs_oracle(got_p.cpu().double(), got_x.cpu().double(), ref_p, ref_x, lengths, f"{what} {form}")
        # fixed-length: layers 2-4 through the per-layer entry into a NaN-filled output
        if case.fixed:
            h = m.time_context_layers[0](xg)
            _check_record(m, form, lengths, True, num_cu, [0], what)
            for l in (1, 2, 3):
                y = torch.full((B, T - ref.CUM[l], HIDDEN), float("nan"), device=DEV)
                _layer_into(m, l, h.contiguous(), y)
                _check_record(m, form, lengths, True, num_cu, [l], what)
                assert torch.isfinite(y).all(), f"{what} {form}: layer index {l} left {int(torch.isnan(y).sum())} NaN in a pre-filled output"
                if l >= 2:
                    assert torch.equal(y.reshape(-1, HIDDEN), (y3, y4)[l - 2]), f"{what} {form}: layer index {l} alone differs from the whole path"
                h = y
        # position independence: an utterance alone gives the bits it has in the batch
        alone = _alone_set(case, marked, np.random.default_rng(case.seed))
        log["alone"][form] = len(alone)
        for u in alone:
            n = lengths[u]
            h = xg[u:u + 1, :n]
            for l in range(4):
                h = m.time_context_layers[l](h)
                _check_record(m, form, [n], True, num_cu, [l], f"{what} utterance {u} alone")
                if l >= 2:
                    assert torch.equal(h[0], (y3, y4)[l - 2][off[u]:off[u + 1]]), \
                        f"{what} {form}: layer {l + 1} of utterance {u} ({n} frames, rows {off[u]}..{off[u + 1]}) differs from the utterance alone"
    # the same bits on both Winograd split3 tilings and on both split3 grids
    assert torch.equal(rows["S8"][0], rows["S4"][0]), f"{what}: layer-3 rows differ between the eight-wave and the four-wave kernel"
    assert torch.equal(rows["S8"][1], rows["S4"][1]), f"{what}: layer-4 rows differ between the split form's two grids"
    if os.environ.get("FUZZ_LOG"):
        with open(os.environ["FUZZ_LOG"], "a") as f:
            f.write(json.dumps(log) + "\n")
