"""CPU-only checks of speaker identification (include/xvec_ident.h): `group_models` against np.unique and the boolean masks of
the package's mean_stat_per_model, the reference's fp64 open-set loop against its longdouble form (and the library's algorithm,
restated in numpy, against both), the header's constants against the module's, and the C ABI's argument errors (each returns
before the library touches a device)."""

import numpy as np
import pytest

import ident_ref
from hipcc_support import header_constants

P = 0x1000          # a pointer that is never followed: every call here fails its argument checks first


# ---------------------------------------------------------------- group_models

@pytest.mark.parametrize("names", [
    ["b", "a", "b", "c", "a", "b"],                                 # unsorted, interleaved
    ["spk3", "spk3", "spk1", "spk2", "spk2", "spk2", "spk1"],
    ["only"] * 5,                                                   # a single model
    ["z"],
    [7, 3, 7, 7, 1, 3],                                             # integer ids
    ["id10", "id9", "id10", "id1"],                                 # sorted as strings, as np.unique sorts them
])
def test_group_models_is_np_unique_and_the_boolean_masks(names):
    from xvector_amd.identify import group_models
    arr = np.asarray(names)
    unique, order, start = group_models(names)
    assert np.array_equal(unique, np.unique(arr))
    assert order.dtype == np.int32 and start.dtype == np.int64
    assert sorted(order.tolist()) == list(range(len(names)))        # a permutation
    assert start[0] == 0 and start[-1] == len(names) and (np.diff(start) >= 1).all() and start.shape == (len(unique) + 1,)
    for c, model in enumerate(unique):
        mine = order[start[c]:start[c + 1]]
        assert np.array_equal(mine, np.nonzero(arr == model)[0])    # the mask's rows, in the order they were given (stable)


def test_group_models_refuses_what_has_no_models():
    from xvector_amd.identify import group_models
    with pytest.raises(ValueError):
        group_models([])
    with pytest.raises(ValueError):
        group_models([["a", "b"]])


def test_reference_model_means_are_the_masked_means():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((7, 5))
    names = np.array(["b", "a", "b", "c", "a", "b", "c"])
    models, means = ident_ref.model_means(x, names)
    assert models.tolist() == ["a", "b", "c"]
    assert np.allclose(means[1], (x[0] + x[2] + x[5]) / 3, rtol=0, atol=1e-15)
    ld = ident_ref.model_means(x, names, ident_ref.LD)[1]
    assert (np.abs(means.astype(ident_ref.LD) - ld) <= ident_ref.model_mean_bound(x, names)).all()


# ---------------------------------------------------------------- the open-set references

def _benign(N, T, seed):
    return np.random.default_rng(seed).normal(-20.0, 15.0, (N, T))


@pytest.mark.parametrize("N,T", [(2, 5), (3, 7), (33, 4), (64, 9), (130, 3)])
@pytest.mark.parametrize("p", [0.1, 0.5, 1.0])
def test_fp64_loop_equals_its_longdouble_form_on_benign_scores(N, T, p):
    s = _benign(N, T, N * 100 + T)
    loop = ident_ref.open_set_loop(s, p)
    out, L, W = ident_ref.open_set_longdouble(s, p)
    # the loop sums N terms left to right and takes exp at the scores' own scale: N u relative on the sum, |S| u per exponent
    bound = ident_ref.U * ((2 * N + 8 + np.abs(s).max(axis=0)[None, :]) + 2 * np.abs(L.astype(np.float64))
                           + np.abs(loop) + np.abs(s))
    assert (np.abs(loop.astype(ident_ref.LD) - out).astype(np.float64) <= bound).all()


@pytest.mark.parametrize("kind", ["plain", "dominated", "equal_maxima", "all_plus_900", "all_minus_900", "minus_inf_row"])
@pytest.mark.parametrize("p", [0.1, 1.0])
def test_the_algorithm_in_numpy_is_inside_the_bound_and_total_minus_own_is_not(kind, p):
    N, T = 64, 6
    s = _benign(N, T, 11)
    if kind == "dominated":
        s[np.arange(T) * 7 % N, np.arange(T)] = 80.0
    elif kind == "equal_maxima":
        s[5], s[40] = 12.5, 12.5
    elif kind == "all_plus_900":
        s[:] = 900.0
    elif kind == "all_minus_900":
        s[:] = -900.0
    elif kind == "minus_inf_row":
        s[9] = -np.inf
    out, L, W = ident_ref.open_set_longdouble(s, p)
    got = ident_ref.open_set_algorithm(s, p)
    fin = np.isfinite(out.astype(np.float64))
    bound = ident_ref.open_set_bound(s, out, L, W)
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(ident_ref.LD) - out).astype(np.float64)
    assert (err[fin] <= bound[fin]).all(), float((err[fin] / bound[fin]).max())
    assert np.array_equal(np.isneginf(got), np.isneginf(out.astype(np.float64)))
    if kind == "dominated":
        with np.errstate(all="ignore"):
            short = np.abs(ident_ref.total_minus_own(s, p).astype(ident_ref.LD) - out).astype(np.float64)
        assert not (short[fin] <= bound[fin]).all()


def test_reference_topk_orders_ties_zeros_and_nans():
    nan = float("nan")
    s = np.array([[1.0, nan, -0.0, nan],
                  [3.0, 2.0, 0.0, nan],
                  [3.0, nan, -1.0, nan],
                  [-np.inf, 2.0, 0.0, nan]])
    idx, val = ident_ref.topk(s, 3)
    assert idx[:, 0].tolist() == [1, 2, 0] and idx[:, 1].tolist() == [1, 3, -1]
    assert idx[:, 2].tolist() == [0, 1, 3] and idx[:, 3].tolist() == [-1, -1, -1]
    assert np.signbit(val[0, 2]) and np.isnan(val[2, 1]) and np.isnan(val[:, 3]).all()
    assert ident_ref.decide(idx, val, 2.0).tolist() == [1, 1, -1, -1]


# ---------------------------------------------------------------- the header, the module and the C ABI without a device

def test_module_restates_the_header_constants_and_refuses_the_cpu():
    import torch
    from xvector_amd import hip, identify
    consts = header_constants("xvec_ident.h", "XVEC_IDENT_")
    assert consts == {"X_F32": hip.IDENT_X_F32, "X_F64": hip.IDENT_X_F64, "COLS": identify.COLS,
                      "SLICE_ROWS": identify.SLICE_ROWS, "BLOCK_ROWS": identify.BLOCK_ROWS,
                      "TOPK_BLOCK_ROWS": identify.TOPK_BLOCK_ROWS, "APPLY_ROWS": identify.APPLY_ROWS,
                      "APPLY_COLS": identify.APPLY_COLS, "MAX_K": identify.MAX_K}
    assert identify.BLOCK_ROWS == 4 * identify.SLICE_ROWS and identify.TOPK_BLOCK_ROWS % identify.BLOCK_ROWS == 0
    s = torch.zeros(3, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="HIP device only"):
        identify.open_set_scores(s, 0.5)
    with pytest.raises(RuntimeError, match="HIP device only"):
        identify.identify(s, 1)
    with pytest.raises(RuntimeError, match="HIP device only"):
        identify.enroll(np.zeros((4, 8)), ["a", "b", "a", "b"], device="cpu")
    import xvector_amd
    assert xvector_amd.SpeakerIdentifier is identify.SpeakerIdentifier and xvector_amd.enroll is identify.enroll


def _open_set(lib, S=P, ld=8, N=4, T=8, p=0.5, out=P + 0x10000, ld_out=8, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.xvec_ident_workspace_bytes(N, T, 0)
    return lib.xvec_open_set_scores(S, ld, N, T, p, out, ld_out, ws, ws_bytes, None)


def _topk(lib, S=P, ld=8, N=4, T=8, k=2, thr=0.0, idx=P, val=P, dec=None, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.xvec_ident_workspace_bytes(N, T, max(0, min(k, 16)))
    return lib.xvec_identify_topk(S, ld, N, T, k, thr, idx, val, dec, ws, ws_bytes, None)


def test_c_abi_argument_errors_return_before_any_device_call():
    """A workspace that is too small answers ERR_WORKSPACE, the code host_support.h gives that error in every back end; every
    other bad argument ERR_ARG."""
    from xvector_amd import hip
    lib, err = hip.lib, lambda: hip.lib.xvec_ident_last_error().decode()
    big_n = 3 * 128 + 1
    need = lib.xvec_ident_workspace_bytes(big_n, 8, 0)
    assert need >= (1 + 4) * 8 * 20 and need % 256 == 0      # the statistics and four blocks' partials of 8 columns
    cases = [
        (dict(N=1), hip.ERR_ARG, "N = 1: open-set scores need at least two models"),
        (dict(N=0), hip.ERR_ARG, "N = 0: open-set scores need at least two models"),
        (dict(T=0, ld=0, ld_out=0), hip.ERR_ARG, "T = 0: need at least one test column"),
        (dict(p=0.0), hip.ERR_ARG, "p_known = 0 must lie in (0, 1]"),
        (dict(p=-0.25), hip.ERR_ARG, "p_known = -0.25 must lie in (0, 1]"),
        (dict(p=1.5), hip.ERR_ARG, "p_known = 1.5 must lie in (0, 1]"),
        (dict(p=float("nan")), hip.ERR_ARG, "p_known = nan must lie in (0, 1]"),
        (dict(ld=7), hip.ERR_ARG, "ld = 7 and ld_out = 8 must be at least T = 8"),
        (dict(ld_out=7), hip.ERR_ARG, "ld = 8 and ld_out = 7 must be at least T = 8"),
        (dict(S=None), hip.ERR_ARG, "null pointer: S / out"),
        (dict(out=None), hip.ERR_ARG, "null pointer: S / out"),
        (dict(out=P, ld_out=9), hip.ERR_ARG, "in place (out == S) needs ld_out == ld (got 9 and 8)"),
        (dict(ws=None), hip.ERR_ARG, "null pointer: workspace"),
        (dict(N=big_n, ws_bytes=need - 1), hip.ERR_WORKSPACE, f"workspace too small: {need - 1} < {need} bytes"),
        (dict(N=2 ** 31, ws_bytes=1 << 40), hip.ERR_TOO_LARGE, f"score matrix [{2 ** 31}, 8]: both sizes must be at most 2^31 - 1"),
    ]
    for kwargs, code, text in cases:
        assert _open_set(lib, **kwargs) == code, kwargs
        assert err() == text, kwargs

    big_n = 2 * 512 + 1
    need = lib.xvec_ident_workspace_bytes(big_n, 8, 16)
    assert need >= 3 * 16 * 8 * 12 and need % 256 == 0
    cases = [
        (dict(N=0), hip.ERR_ARG, "score matrix [0, 8]: need at least one model and one test column"),
        (dict(T=0, ld=0), hip.ERR_ARG, "score matrix [4, 0]: need at least one model and one test column"),
        (dict(k=0), hip.ERR_ARG, "k = 0 must lie in 1 .. 16"),
        (dict(k=17), hip.ERR_ARG, "k = 17 must lie in 1 .. 16"),
        (dict(k=-1), hip.ERR_ARG, "k = -1 must lie in 1 .. 16"),
        (dict(ld=7), hip.ERR_ARG, "ld = 7 is smaller than T = 8"),
        (dict(S=None), hip.ERR_ARG, "null pointer: S / idx / val"),
        (dict(idx=None), hip.ERR_ARG, "null pointer: S / idx / val"),
        (dict(val=None), hip.ERR_ARG, "null pointer: S / idx / val"),
        (dict(ws=None), hip.ERR_ARG, "null pointer: workspace"),
        (dict(N=big_n, k=16, ws_bytes=need - 1), hip.ERR_WORKSPACE, f"workspace too small: {need - 1} < {need} bytes"),
        (dict(T=2 ** 31, ld=2 ** 31, ws_bytes=1 << 40), hip.ERR_TOO_LARGE, f"score matrix [4, {2 ** 31}]: both sizes must be at most 2^31 - 1"),
    ]
    for kwargs, code, text in cases:
        assert _topk(lib, **kwargs) == code, kwargs
        assert err() == text, kwargs
    for N, T, k in ((0, 8, 1), (8, 0, 1), (2 ** 31, 8, 1), (8, 8, -1), (8, 8, 17)):
        assert lib.xvec_ident_workspace_bytes(N, T, k) == 0, (N, T, k)
    assert lib.xvec_ident_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1, 16) > 0


def test_model_mean_argument_errors_return_before_any_device_call():
    import ctypes
    from xvector_amd import hip
    lib, err = hip.lib, lambda: hip.lib.xvec_ident_last_error().decode()
    start = lambda *v: (ctypes.c_int64 * len(v))(*v)
    good = dict(x=P, dt=hip.IDENT_X_F64, n=5, dim=4, ld=4, order=P, start=start(0, 2, 5), m=2, out=P, ws=P, ws_bytes=256)
    call = lambda **kw: lib.xvec_model_mean(*[{**good, **kw}[a] for a in
                                              ("x", "dt", "n", "dim", "ld", "order", "start", "m", "out", "ws", "ws_bytes")], None)
    assert lib.xvec_model_mean_workspace_bytes(2) == 256 and lib.xvec_model_mean_workspace_bytes(0) == 0
    cases = [
        (dict(n=0), hip.ERR_ARG, "need at least one enrolment vector (n = 0)"),
        (dict(n=2 ** 31), hip.ERR_TOO_LARGE, f"n = {2 ** 31}: row indices are int32"),
        (dict(dim=0), hip.ERR_ARG, "dim = 0 and n_models = 2 must be >= 1"),
        (dict(m=6, start=start(0, 1, 2, 3, 4, 5, 5)), hip.ERR_ARG, "more models (6) than vectors (5)"),
        (dict(ld=3), hip.ERR_ARG, "ld = 3 is smaller than dim = 4"),
        (dict(dt=7), hip.ERR_ARG, "x_dtype 7 unknown"),
        (dict(x=None), hip.ERR_ARG, "null pointer"),
        (dict(order=None), hip.ERR_ARG, "null pointer"),
        (dict(out=None), hip.ERR_ARG, "null pointer"),
        (dict(start=start(1, 2, 5)), hip.ERR_ARG, "class_start must run from 0 to n = 5 (got 1 .. 5)"),
        (dict(start=start(0, 2, 4)), hip.ERR_ARG, "class_start must run from 0 to n = 5 (got 0 .. 4)"),
        (dict(start=start(0, 0, 5)), hip.ERR_ARG, "model 0 is empty or model_start decreases: every model needs a row"),
        (dict(start=start(0, 5, 5)), hip.ERR_ARG, "model 1 is empty or model_start decreases: every model needs a row"),
        (dict(ws_bytes=255), hip.ERR_WORKSPACE, "workspace too small: 255 < 256 bytes"),
    ]
    for kwargs, code, text in cases:
        assert call(**kwargs) == code, kwargs
        assert err() == text, kwargs


def test_ident_error_channel_is_its_own():
    from xvector_amd import hip
    lib = hip.lib
    assert lib.xvec_snorm_row_stats(P, 8, 4, 8, -5, None, P, P, P, P, P, 4096, None) == hip.ERR_ARG
    assert _topk(lib, k=99) == hip.ERR_ARG
    assert lib.xvec_ident_last_error().decode() == "k = 99 must lie in 1 .. 16"
    assert lib.xvec_snorm_last_error().decode() == "top_k = -5 must not be negative (0 = every valid cell)"


def test_fast_plda_scoring_points_to_the_open_set_call():
    from xvector_amd import scoring

    class Stat:
        modelset = segset = np.array(["a", "b"])
        stat1 = np.zeros((2, 4))

    with pytest.raises(NotImplementedError, match="open_set_scores"):
        scoring.fast_PLDA_scoring(Stat(), Stat(), None, np.zeros(4), np.eye(4), np.eye(4), p_known=0.1)
