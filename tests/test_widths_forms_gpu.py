"""Every TDNN kernel form at model widths other than 24 / 512 (the reference's user configuration: input_size, hidden_size,
x_vector_size, num_classes and batch_norm are constructor arguments), against the fp64 oracle and against each other.

  A. seven architectures x three forced fp32 handles (split / fp32 Winograd / direct) at small shapes: every element of every
     layer, layer 5's fused pooling, the split form's error against the direct form's, the whole path, determinism;
  B. five of them at a large batch with the default dispatch, in fp32, bf16 and bf16x3: the forms and kernel families the
     planner picks (tdnn_split3, tdnn_wino_s3, tdnn_pp16, tdnn_first) against the other family / the fp32 Winograd handle;
  C. the planner's switch-over to the split operands, exactly at 64 output rows per CU, per layer;
  D. exact scaling: with batch_norm=False the path is positively homogeneous, and scaling the input and every bias by 2^k must
     scale every layer's frames, the pooled statistics and the x-vector by exactly 2^k in every kernel family.
"""
import ctypes

import numpy as np
import pytest
import torch

import xvector_oracle as oracle
from conftest import assert_parity, assert_parity_masked, float_params
from tdnn_support import DEV, make_model, oracle_layer, worst_rel

pytestmark = pytest.mark.gpu

# (input_size, hidden_size, batch_norm, x_vector_size, num_classes)
ARCHS = {
    "W0": (24, 512, True, 512, 1211),   # the baseline: the split layer 4-5 tails nobody ran
    "W1": (13, 512, True, 200, 37),     # layer-1 kpt 80 (cin_pad 16 x 5 taps) in the streaming kernels
    "W2": (20, 400, False, 128, 11),    # n_pad 512 with 112 padded columns; tdnn_first with padded outputs; K tail 400 -> 448
    "W3": (40, 256, True, 256, 50),     # tdnn_first not applicable (kpt 200 > 126: bf16 layer 1 on tile128); pp16 at one column
    "W4": (24, 136, True, 64, 5),       # n_pad 256 with 120 padded columns; K tail 136 -> 192 (split k-steps cut mid-chunk)
    "W5": (23, 768, False, 512, 100),   # three 256-columns in pp16; odd input (cin_pad 24); tdnn_first not applicable (n_pad 768)
    "W6": (24, 72, True, 16, 3),        # one 128-column tile; kpt_pad 128
}
SEEDS = {name: 700 + i for i, name in enumerate(ARCHS)}

SPLIT_FORMS = ["direct", "winograd_f23", "winograd_f23", "bf16_split3", "bf16_split3"]
SPLIT_OPERANDS = ["fp32"] + ["bf16_split3"] * 4
WINO_FORMS = ["direct", "winograd_f23", "winograd_f23", "direct", "direct"]
FP32_ENVS = {"split": {"XVEC_SPLIT3_MIN_ROWS": "0", "XVEC_WINO_SPLIT3_MIN_ROWS": "0"},
             "wino": {"XVEC_SPLIT3": "0", "XVEC_WINO_SPLIT3": "0"},
             "direct": {"XVEC_WINOGRAD": "0", "XVEC_SPLIT3": "0"}}


def _sd(arch, batch_norm=None, seed=None):
    import xvector_amd as xa
    cin, hid, bn, xv, nc = ARCHS[arch]
    bn = bn if batch_norm is None else batch_norm
    sd = xa.synth.make_state_dict(SEEDS[arch] if seed is None else seed, input_size=cin, hidden_size=hid, num_classes=nc,
                                  x_vector_size=xv, batch_norm=bn)
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _model(arch, sd, precision="fp32", env=None, batch_norm=None):
    """A model of `arch` whose handle is created now, under `env` (the knobs are read once per handle in xvec_create)."""
    cin, hid, bn, xv, nc = ARCHS[arch]
    return make_model(sd, env, precision, input_size=cin, hidden_size=hid, num_classes=nc, x_vector_size=xv,
                      batch_norm=bn if batch_norm is None else batch_norm)


_ARCH_CACHE = {}


def _arch(name):
    """Weights, fp64 parameters and the three forced fp32 handles of an architecture (built once per module run)."""
    if name not in _ARCH_CACHE:
        sd = _sd(name)
        _ARCH_CACHE[name] = {"sd": sd, "p64": oracle.cast_params(float_params(sd), torch.float64), "bn": ARCHS[name][2],
                             **{k: _model(name, sd, env=e) for k, e in FP32_ENVS.items()}}
    return _ARCH_CACHE[name]


def _mfcc(arch, B, T, seed):
    import xvector_amd as xa
    return xa.synth.make_mfcc(B, T, input_size=ARCHS[arch][0], seed=seed)


def _num_cu(m):
    from xvector_amd import hip
    lay = hip.WsLayout()
    hip.check(hip.lib.xvec_workspace_layout(m._engine(torch.device(DEV)).h, 1000, 1, ctypes.byref(lay)))
    return lay.num_cu


def _oracle_pooled_xvec(x, lens, p64, bn, idx):
    """Per utterance on the un-padded slice: pooled statistics and layer-6 x-vectors of utterances `idx`."""
    pooled = []
    with torch.no_grad():
        for j in idx:
            xj = torch.as_tensor(x[j:j + 1, :lens[j]]).double()
            pooled.append(oracle.stat_pool(oracle.time_context_layers(xj, p64, bn)))
    pooled = torch.cat(pooled)
    return pooled, pooled @ p64["segment_layer6.weight"].t() + p64["segment_layer6.bias"]     # main.py:81-94, layer 6


def _assert_forms_agree(got, ref, lens, what, pooled=False):
    """Two fp32 forms of the whole path (or of layer 5 + pooling) against each other, per utterance of `lens` frames.

    Utterances with at least 16 pooled frames at 1e-5.  Of their stds, those under 1 % of the mean non-zero std on both
    sides are listed instead of bounded (assert_parity_masked): a channel that is on in a frame or two with a pre-activation
    within fp32 rounding of zero, whose std is that rounding (measured: 0 against 2e-7, 1.6e-7 against 3.1e-7 where the bound
    is 8e-8 in the models without BatchNorm, W2 and W5, whose layer-5 outputs are small; at most 1.2e-2 of the elements).
    Shorter utterances, whose stds hang on a few frames (std = |a - b| / sqrt 2 of two; measured over 11: 3.4034e-4 against
    3.4045e-4), at the fp32 bar, 1e-4; every utterance is also checked against the oracle."""
    n = torch.as_tensor([int(v) - 14 for v in lens])
    got, ref = got.double().cpu(), ref.double().cpu()
    longs, shorts = n >= 16, n < 16
    if shorts.any():
        assert_parity(got[shorts], ref[shorts], 1e-4, f"{what} (< 16 pooled frames)", elem_tol=1e-3)
    if not longs.any():
        return
    g, r = got[longs], ref[longs]
    if not pooled:
        assert_parity(g, r, 1e-5, what)
        return
    C = r.shape[1] // 2
    big = torch.maximum(g[:, C:], r[:, C:])
    exclude = torch.zeros_like(r, dtype=torch.bool)
    exclude[:, C:] = (big > 0) & (big < 1e-2 * r[:, C:][r[:, C:] > 0].mean())
    assert_parity_masked(g, r, 1e-5, what, 1e-5, exclude, max_excluded=MAX_ILL_STDS)


# ---------------------------------------------------------------------------------------------------------------------------
# A. forced fp32 forms, small shapes, every element

SHAPES = [(1, 15), (3, 16), (7, 25), (5, 61), (2, 300), (1, 3000), (16, 200)]
MID = (16, 200)          # ~3 000 rows per layer: the error-ratio shape
MAX_ILL_STDS = 2e-2


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("arch", list(ARCHS))
def test_every_layer_every_form(arch, B, T):
    a = _arch(arch)
    ms, mw, md, p64, bn = a["split"], a["wino"], a["direct"], a["p64"], a["bn"]
    h = torch.as_tensor(_mfcc(arch, B, T, seed=SEEDS[arch] * 100 + B * 7 + T)).to(DEV)
    for layer in range(5):
        ref = oracle_layer(h.cpu(), p64, layer, bn)
        gs = ms.time_context_layers[layer](h)
        assert ms.last_forms()[layer] == SPLIT_FORMS[layer] and ms.last_operands()[layer] == SPLIT_OPERANDS[layer], \
            (arch, layer, ms.last_forms(), ms.last_operands())
        assert ms.last_dispatch()[layer] == "tile128"
        gw = mw.time_context_layers[layer](h)
        assert mw.last_forms()[layer] == WINO_FORMS[layer] and mw.last_operands()[layer] == "fp32"
        gd = md.time_context_layers[layer](h)
        assert md.last_forms()[layer] == "direct" and md.last_operands()[layer] == "fp32"
        what = f"{arch} layer {layer} B={B} T={T}"
        for g, name in ((gs, "split"), (gw, "fp32 winograd"), (gd, "direct")):
            assert_parity(g, ref.float(), 1e-4, f"{what}: {name} vs oracle")
        assert_parity(gs, gd, 1e-5, f"{what}: split vs direct")
        if (B, T) == MID and layer > 0:
            # the check that sees a split that drops its lo piece (~2^-17 per operand: under the 1e-4 bar, over this ratio)
            es, ed = worst_rel(gs, ref), worst_rel(gd, ref)
            print(f"{arch} layer {layer}: worst-frame error split {es:.3e}, direct {ed:.3e} ({es / ed:.2f}x)")
            assert es <= 1.5 * ed, f"{what}: split {es:.3e} vs direct {ed:.3e}"
        if layer == 4:
            # the fused pooling epilogue on the same input, against stat_pool of the oracle's frames
            ref_p = oracle.stat_pool(ref)
            n = T - 14
            for m, name, form in ((ms, "split", "bf16_split3"), (mw, "fp32 winograd", "direct"), (md, "direct", "direct")):
                pooled = m.pooled_last_layer(h)
                assert m.last_forms()[4] == form
                C = pooled.shape[1] // 2
                assert_parity(pooled[:, :C], ref_p[:, :C], 1e-4, f"{what}: {name} pooled means")
                if n >= 2:           # (one frame: no std; two frames: std = |a - b| / sqrt 2, element-wise ill-conditioned)
                    assert_parity(pooled, ref_p, 1e-4, f"{what}: {name} pooled", elem_tol=1e-3 if n >= 64 else 5e-2)
                if name == "split":
                    p_split = pooled
                elif name == "direct":
                    assert_parity(p_split[:, :C], pooled[:, :C], 1e-5, f"{what}: pooled means split vs direct")
                    if n >= 2:
                        _assert_forms_agree(p_split, pooled, [T] * B, f"{what}: pooled split vs direct", pooled=True)
        assert torch.equal(gs, ms.time_context_layers[layer](h)), f"{what}: repeat run differs"
        h = gd


@pytest.mark.parametrize("arch", list(ARCHS))
def test_whole_path_split_handle(arch):
    """extract_x_vec (layers 6 and 7), forward and a NaN-padded ragged batch on the split handle against the oracle per
    utterance and against the direct handle."""
    a = _arch(arch)
    ms, md, p64, bn = a["split"], a["direct"], a["p64"], a["bn"]
    for B, T in ((3, 16), (5, 61), (2, 300), (1, 3000)):
        x = _mfcc(arch, B, T, seed=SEEDS[arch] * 1000 + B + T)
        xg = torch.as_tensor(x).to(DEV)
        xt = torch.as_tensor(x).double()
        what = f"{arch} B={B} T={T}"
        with torch.no_grad():
            ref6 = oracle.extract_x_vec(xt, p64, 6, bn)
            ref7 = oracle.extract_x_vec(xt, p64, 7, bn)
            refl = oracle.forward(xt, p64, bn)
        got = {}
        for layer, ref in ((6, ref6), (7, ref7)):
            for m in (ms, md):
                m.x_vec_extract_layer = layer
            try:
                gs = ms.extract_x_vec(xg)
                assert ms.last_forms() == SPLIT_FORMS and ms.last_operands() == SPLIT_OPERANDS
                gd = md.extract_x_vec(xg)
            finally:
                for m in (ms, md):
                    m.x_vec_extract_layer = 6
            assert torch.isfinite(gs).all()
            assert_parity(gs, ref, 1e-4, f"{what}: x-vector layer {layer} vs oracle", elem_tol=1e-3)
            _assert_forms_agree(gs, gd, [T] * B, f"{what}: x-vector layer {layer} split vs direct")
            got[layer] = gs
        gl = ms(xg)
        assert ms.last_forms() == SPLIT_FORMS and ms.last_operands() == SPLIT_OPERANDS
        assert torch.isfinite(gl).all()
        assert_parity(gl, refl, 1e-4, f"{what}: logits vs oracle", elem_tol=1e-3)
        _assert_forms_agree(gl, md(xg), [T] * B, f"{what}: logits split vs direct")
        assert torch.equal(got[6], ms.extract_x_vec(xg)), f"{what}: repeat run differs"
    # ragged, NaN in every padded frame, lengths from 16 to T
    lens = [16, 300, 17, 61, 120, 29, 255, 16, 200, 64, 31]
    T = max(lens)
    x = _mfcc(arch, len(lens), T, seed=SEEDS[arch] * 1000 + 7)
    for i, n in enumerate(lens):
        x[i, n:] = np.nan
    xg = torch.as_tensor(x).to(DEV)
    gs = ms.extract_x_vec(xg, lengths=lens)
    assert ms.last_forms() == SPLIT_FORMS and ms.last_operands() == SPLIT_OPERANDS
    assert torch.isfinite(gs).all()
    _, ref = _oracle_pooled_xvec(x, lens, p64, bn, range(len(lens)))
    assert_parity(gs, ref, 1e-4, f"{arch} ragged x-vectors vs oracle", elem_tol=1e-3)
    _assert_forms_agree(gs, md.extract_x_vec(xg, lengths=lens), lens, f"{arch} ragged split vs direct")
    assert torch.equal(gs, ms.extract_x_vec(xg, lengths=lens)), f"{arch} ragged: repeat run differs"


# ---------------------------------------------------------------------------------------------------------------------------
# B. large batch, default dispatch, fp32 / bf16 / bf16x3

LARGE = ["W1", "W2", "W3", "W4", "W5"]
# tdnn_first[3]_applicable: 512 padded output channels (W4: n_pad 256, W5: 768) and layer-1 kpt <= 126 (W3: 200)
FIRST_APPLICABLE = {"W1": True, "W2": True, "W3": False, "W4": False, "W5": False}


def _large_inputs(arch):
    """B = 128, T = 300, and a ragged batch of similar size (NaN padding, lengths 16 .. T)."""
    B, T = 128, 300
    x = _mfcc(arch, B, T, seed=SEEDS[arch] * 10 + 1)
    rng = np.random.default_rng(SEEDS[arch])
    lens = rng.integers(200, T + 1, 140).tolist()   # (W3's layers 3-5: 1.8 units of 64 rows on each of 256 CUs = 29.5 k rows)
    lens[3], lens[77] = 16, T
    xr = _mfcc(arch, len(lens), T, seed=SEEDS[arch] * 10 + 2)
    for i, n in enumerate(lens):
        xr[i, n:] = np.nan
    return [(x, [T] * B, None), (xr, lens, lens)]


@pytest.mark.parametrize("arch", LARGE)
def test_large_batch_fp32_default(arch):
    a = _arch(arch)
    m = _model(arch, a["sd"])                       # no knobs
    mw, p64, bn = a["wino"], a["p64"], a["bn"]
    for x, lens, lengths in _large_inputs(arch):
        xg = torch.as_tensor(x).to(DEV)
        what = f"{arch} fp32 B={x.shape[0]} ragged={lengths is not None}"
        pooled = m.pooled(xg, lengths=lengths)
        assert m.last_forms() == SPLIT_FORMS and m.last_operands() == SPLIT_OPERANDS, (m.last_forms(), m.last_operands())
        assert m.last_dispatch() == ["tile128"] * 5
        xv = m.extract_x_vec(xg, lengths=lengths)
        assert torch.isfinite(xv).all()
        pw = mw.pooled(xg, lengths=lengths)
        assert mw.last_forms() == WINO_FORMS and mw.last_operands() == ["fp32"] * 5
        _assert_forms_agree(pooled, pw, lens, f"{what}: pooled split vs fp32 winograd", pooled=True)
        _assert_forms_agree(xv, mw.extract_x_vec(xg, lengths=lengths), lens, f"{what}: x-vectors split vs fp32 winograd")
        idx = sorted({0, 41, 77, 3, x.shape[0] - 1})
        ref_p, ref_x = _oracle_pooled_xvec(x, lens, p64, bn, idx)
        C = ref_p.shape[1] // 2
        for k, j in enumerate(idx):
            n = lens[j] - 14
            assert_parity(pooled[j:j + 1, :C], ref_p[k:k + 1, :C], 1e-4, f"{what}: means utt {j}")
            assert_parity(pooled[j:j + 1, C:], ref_p[k:k + 1, C:], 1e-4, f"{what}: stds utt {j}",
                          elem_tol=1e-3 if n >= 64 else 5e-2)
            assert_parity(xv[j:j + 1], ref_x[k:k + 1], 1e-4, f"{what}: x-vector utt {j}", elem_tol=1e-3)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("arch", LARGE)
def test_large_batch_bf16_families(arch, precision):
    a = _arch(arch)
    p64, bn = a["p64"], a["bn"]
    m_pp = _model(arch, a["sd"], precision)
    m_old = _model(arch, a["sd"], precision, env={"XVEC_PP": "0"})
    first = "first" if FIRST_APPLICABLE[arch] else "tile128"
    tight = 2e-3 if precision == "bf16" else 2e-5
    bar, elem = (1e-2, 4e-2) if precision == "bf16" else (1e-4, 1e-3)
    for x, lens, lengths in _large_inputs(arch):
        xg = torch.as_tensor(x).to(DEV)
        B = x.shape[0]
        what = f"{arch} {precision} B={B} ragged={lengths is not None}"
        got = m_pp.pooled(xg, lengths=lengths)
        assert m_pp.last_dispatch() == [first, "pp", "pp", "pp", "pp"], (what, m_pp.last_dispatch())
        assert torch.equal(got, m_pp.pooled(xg, lengths=lengths)), f"{what}: repeat run differs"
        old = m_old.pooled(xg, lengths=lengths)
        assert m_old.last_dispatch() == ["tile128"] * 5
        short = torch.zeros_like(got, dtype=torch.bool)
        if lengths is not None:
            short[torch.as_tensor([n - 14 < 4 for n in lens])] = True
        assert_parity_masked(got, old, tight, f"{what}: pooled pp vs 128x128", 2e-2 if precision == "bf16" else 10 * tight,
                             short, max_excluded=1.5 / B if lengths is not None else 0.0)
        xv = m_pp.extract_x_vec(xg, lengths=lengths)
        assert m_pp.last_dispatch() == [first, "pp", "pp", "pp", "pp"]
        assert_parity(xv, m_old.extract_x_vec(xg, lengths=lengths), tight, f"{what}: x-vectors pp vs 128x128",
                      elem_tol=10 * tight)
        idx = sorted({0, 41, 77, B - 1})
        ref_p, ref_x = _oracle_pooled_xvec(x, lens, p64, bn, idx)
        C = ref_p.shape[1] // 2
        for k, j in enumerate(idx):
            assert_parity(got[j:j + 1, :C], ref_p[k:k + 1, :C], bar, f"{what}: means utt {j} vs oracle", elem_tol=elem)
            assert_parity(xv[j:j + 1], ref_x[k:k + 1], bar, f"{what}: x-vector utt {j} vs oracle", elem_tol=elem)
            assert_parity(got[j:j + 1], ref_p[k:k + 1], bar, f"{what}: pooled utt {j} vs oracle", elem_tol=elem)


# ---------------------------------------------------------------------------------------------------------------------------
# C. the planner's switch-over

def _lens_with_rows(B, cum, rows, T=300):
    """B lengths <= T whose output rows sum(len - cum) are exactly `rows`."""
    total = rows + B * cum
    base, extra = divmod(total, B)
    lens = [base + (1 if i < extra else 0) for i in range(B)]
    assert max(lens) <= T and min(lens) > 14 and sum(n - cum for n in lens) == rows
    return lens


def test_planner_switch_over_exact():
    a = _arch("W0")
    m = _model("W0", a["sd"])                       # the default handle
    num_cu = _num_cu(m)
    assert num_cu == torch.cuda.get_device_properties(0).multi_processor_count
    R = 64 * num_cu
    p64, bn = a["p64"], a["bn"]
    T = 300
    B = -(-R // 280)                                 # lengths around 280 frames
    x = _mfcc("W0", B + 1, T, seed=4242)
    # pair 1: layers 3-5 at R - 1 / R output rows (layer 2, 6 B rows more, past R in both)
    # pair 2: layer 2 at R - 1 / R output rows (layers 3-5, 6 B rows fewer, below R in both)
    for cum, flips in ((14, (2, 3, 4)), (8, (1,))):
        lo = _lens_with_rows(B, cum, R - 1, T)
        hi = list(lo)
        j = next(i for i, n in enumerate(hi) if n < T)
        hi[j] += 1                                   # one frame more: R rows
        outs, seen = [], []
        for lens in (lo, hi):
            rows = [sum(n - c for n in lens) for c in (4, 8, 14, 14, 14)]
            xv = m.extract_x_vec(torch.as_tensor(x[:B]).to(DEV), lengths=lens)
            ops, forms = m.last_operands(), m.last_forms()
            for layer in range(1, 5):
                split = rows[layer] >= R
                assert ops[layer] == ("bf16_split3" if split else "fp32"), (cum, layer, rows[layer], R, ops)
                assert forms[layer] == ("winograd_f23" if layer < 3 else "bf16_split3" if split else "direct"), (layer, forms)
            assert ops[0] == "fp32" and forms[0] == "direct"
            outs.append(xv)
            seen.append((ops, forms))
        (ops_lo, forms_lo), (ops_hi, forms_hi) = seen
        if cum == 14:
            assert ops_lo[1:] == ["bf16_split3"] + ["fp32"] * 3 and ops_hi[1:] == ["bf16_split3"] * 4
            assert forms_lo[3:] == ["direct"] * 2 and forms_hi[3:] == ["bf16_split3"] * 2
        else:
            assert ops_lo[1:] == ["fp32"] * 4 and ops_hi[1:] == ["bf16_split3"] + ["fp32"] * 3
            assert forms_lo == forms_hi == WINO_FORMS
        r_lo = [sum(n - c for n in lo) for c in (4, 8, 14, 14, 14)]
        r_hi = [sum(n - c for n in hi) for c in (4, 8, 14, 14, 14)]
        assert [l for l in range(1, 5) if (r_lo[l] >= R) != (r_hi[l] >= R)] == list(flips)
        same = [i for i in range(B) if i != j]
        assert_parity(outs[0][same], outs[1][same], 1e-5, f"switch-over cum={cum}: common utterances")
        idx = sorted({0, j, B // 2, B - 1})
        for lens, xv in ((lo, outs[0]), (hi, outs[1])):
            _, ref = _oracle_pooled_xvec(x, lens, p64, bn, idx)
            assert_parity(xv[idx], ref, 1e-4, f"switch-over cum={cum} vs oracle", elem_tol=1e-3)


# ---------------------------------------------------------------------------------------------------------------------------
# D. exact scaling across exponents

KS = (-30, -12, 12, 30)


def _scaled(sd, k):
    s = 2.0 ** k
    return {n: (v * s if n.endswith(".bias") and (n.startswith("time_context_layers.") or n.startswith("segment_layer6"))
                else v) for n, v in sd.items()}


def _scale_family(arch, handles, x):
    """Run every handle on x and 2^k x with the biases scaled by 2^k; frames of every layer (each handle's own chain),
    pooled statistics and layer-6 x-vectors must scale bit for bit."""
    sd = _sd(arch, batch_norm=False)
    xg = torch.as_tensor(x).to(DEV)
    for name, (m, check) in handles.items():
        def run(xs, sdk):
            m.load_state_dict(sdk)                   # repacks the handle's weights (same handle, same knobs)
            frames, h = [], xs
            for i in range(5):
                h = m.time_context_layers[i](h)
                frames.append(h)
            pooled = m.pooled(xs)
            check(m)
            return frames, pooled, m.extract_x_vec(xs)
        f0, p0, x0 = run(xg, sd)
        assert torch.isfinite(p0).all() and torch.isfinite(x0).all()
        for k in KS:
            s = 2.0 ** k
            fk, pk, xk = run(xg * s, _scaled(sd, k))
            for i, (a_, b_) in enumerate(zip(fk, f0)):
                assert torch.equal(a_, b_ * s), f"{arch} {name} k={k}: layer {i} frames not scaled exactly " \
                    f"({int((a_ != b_ * s).sum())} elements differ)"
            assert torch.equal(pk, p0 * s), f"{arch} {name} k={k}: pooled statistics not scaled exactly " \
                f"({int((pk[:, :pk.shape[1] // 2] != p0[:, :pk.shape[1] // 2] * s).sum())} means, " \
                f"{int((pk[:, pk.shape[1] // 2:] != p0[:, pk.shape[1] // 2:] * s).sum())} stds differ)"
            assert torch.equal(xk, x0 * s), f"{arch} {name} k={k}: x-vectors not scaled exactly"
        m.load_state_dict(sd)


def _expect(forms=None, operands=None, dispatch=None):
    def check(m):
        if forms is not None:
            assert m.last_forms() == forms, m.last_forms()
        if operands is not None:
            assert m.last_operands() == operands, m.last_operands()
        if dispatch is not None:
            assert m.last_dispatch() == dispatch, m.last_dispatch()
    return check


SCALE_ARCHS = ["W2", "W0"]          # W2: BN off by construction; W0: the 512-wide model, built with batch_norm=False


@pytest.mark.parametrize("arch", SCALE_ARCHS)
def test_exact_scaling_fp32_forms_small(arch):
    sd = _sd(arch, batch_norm=False)
    hs = {k: (_model(arch, sd, env=e, batch_norm=False), c) for (k, e), c in zip(FP32_ENVS.items(), (
        _expect(SPLIT_FORMS, SPLIT_OPERANDS), _expect(WINO_FORMS, ["fp32"] * 5), _expect(["direct"] * 5, ["fp32"] * 5)))}
    _scale_family(arch, hs, _mfcc(arch, 5, 61, seed=61))


@pytest.mark.parametrize("arch", SCALE_ARCHS)
def test_exact_scaling_large_batch(arch):
    sd = _sd(arch, batch_norm=False)
    first = "first" if arch in ("W0", "W2") else "tile128"
    hs = {"fp32": (_model(arch, sd, batch_norm=False), _expect(SPLIT_FORMS, SPLIT_OPERANDS, ["tile128"] * 5))}
    for p in ("bf16", "bf16x3"):
        hs[p] = (_model(arch, sd, p, batch_norm=False), _expect(dispatch=[first] + ["pp"] * 4))
        hs[p + " XVEC_PP=0"] = (_model(arch, sd, p, env={"XVEC_PP": "0"}, batch_norm=False), _expect(dispatch=["tile128"] * 5))
    _scale_family(arch, hs, _mfcc(arch, 128, 300, seed=128))
