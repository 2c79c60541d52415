"""VBx on the device (csrc/vbx.hip, include/xvec_vbx.h) against tests/vbx_ref.py, through the C ABI.

Parity.  With epsilon = -inf and a fixed number of iterations, gamma, pi and every ELBO slot are held against the log-domain
restatement run in np.longdouble.  The bar is measured per case, not fixed: 8 x the larger of the two fp64 restatements' own
distances to that run (absolute for gamma and pi, relative for the ELBO) -- the margin covers the device's tiled order of the
sums over T and D, a reordering of terms of one magnitude.  Labels and speaker counts must be EQUAL (tests/test_vbx.py holds
that no frame of these cases is a near tie), and so must the iteration count under the stop rule (and that no ELBO increment
of those cases is near epsilon).  Every case prints its distances; XVEC_VBX_ERRORS_LOG=<file> appends them to a file
(profiles/vbx_errors.txt is such a log of one full run).

Exactness.  A recording's result is a pure function of its own inputs: bit-identical from run to run, alone or inside a batch,
whatever the row strides, the base alignment and the workspace held before."""
import ctypes
import os

import numpy as np
import pytest
import torch

import score_support as ss
import vbx_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
MARGIN = 8.0
BATCH = [5, 64, 1, 65, 300, 37, 1]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _i64(v):
    return (ctypes.c_int64 * len(v))(*[int(x) for x in v])


def _starts(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _strided(a, ld, odd):
    """A device copy of the host matrix `a` with row stride `ld`, NaN in every cell outside it, its base an odd multiple of 8
    bytes with `odd`: (the view, the buffer that owns it)."""
    n, m = a.shape
    buf = torch.full((n * ld + 2,), NAN, dtype=torch.float64, device=DEV)
    at = 1 if odd and buf.data_ptr() % 16 == 0 else 0
    view = buf[at:at + n * ld].view(n, ld)[:, :m]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
    if odd:
        assert view.data_ptr() % 16 == 8
    return view, buf


def _run(X, phi, gamma0, pi0, rec_start, max_iter, epsilon=-INF, loop_prob=0.99, Fa=0.3, Fb=17.0, ldx=None, ldg=None, odd=False,
         ws=None, outputs=True, fill_ws=None):
    """xvec_vbx_run on host inputs (gamma0 [N, S], pi0 [n_rec, S]): a dict of numpy arrays, and the device X / phi before and
    after as `untouched`."""
    from xvector_amd import hip
    X, gamma0 = np.asarray(X, dtype=np.float64), np.asarray(gamma0, dtype=np.float64)
    N, D = X.shape
    S = gamma0.shape[1]
    n_rec = len(rec_start) - 1
    pi0 = np.asarray(pi0, dtype=np.float64).reshape(n_rec, S)
    xd, xbuf = _strided(X, D if ldx is None else ldx, odd)
    gd, gbuf = _strided(gamma0, S if ldg is None else ldg, odd)
    x_before = xbuf.clone()
    phid = torch.from_numpy(np.ascontiguousarray(phi, dtype=np.float64)).to(DEV)
    phi_before = phid.clone()
    pid = torch.from_numpy(np.ascontiguousarray(pi0)).to(DEV)
    elbo = torch.full((n_rec, max_iter), 7.5, dtype=torch.float64, device=DEV)
    iters = torch.full((n_rec,), -7, dtype=torch.int32, device=DEV)
    labels = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    count = torch.full((n_rec,), -7, dtype=torch.int32, device=DEV)
    rs = _i64(rec_start)
    need = int(hip.lib.xvec_vbx_workspace_bytes(rs, n_rec, D, S))
    assert need > 0 and need % 256 == 0
    if ws is None:
        wst = torch.empty(need, dtype=torch.uint8, device=DEV)
        if fill_ws is not None:
            wst.fill_(fill_ws)
        ws = wst.data_ptr()
    opts = hip.VbxOptions(loop_prob, Fa, Fb, epsilon, max_iter, 0)
    rc = hip.lib.xvec_vbx_run(xd.data_ptr(), xd.stride(0), D, phid.data_ptr(), rs, n_rec, S, ctypes.byref(opts), gd.data_ptr(),
                              gd.stride(0), pid.data_ptr(), elbo.data_ptr(), iters.data_ptr(), labels.data_ptr() if outputs else None,
                              count.data_ptr() if outputs else None, ws, need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_vbx_last_error()
    torch.cuda.synchronize()
    untouched = bool(torch.equal(xbuf.view(torch.int64), x_before.view(torch.int64))) and bool(torch.equal(phid, phi_before))
    gflat = gbuf.cpu().numpy()
    outside = np.ones(gflat.shape[0], dtype=bool)
    off = (gd.data_ptr() - gbuf.data_ptr()) // 8
    ld = gd.stride(0)
    for t in range(N):
        outside[off + t * ld:off + t * ld + S] = False
    return dict(gamma=gd.cpu().numpy().copy(), pi=pid.cpu().numpy(), elbo=elbo.cpu().numpy(), iters=iters.cpu().numpy(),
                labels=labels.cpu().numpy(), n_speakers=count.cpu().numpy(), untouched=untouched,
                around_is_nan=bool(np.isnan(gflat[outside]).all()))


def _same(a, b, what, keys=("gamma", "pi", "elbo")):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)
    for k in ("iters", "labels", "n_speakers"):
        assert np.array_equal(a[k], b[k]), (what, k)


def _same_floats(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("gamma", "pi", "elbo"))


def _log(line):
    print(line)
    if os.environ.get("XVEC_VBX_ERRORS_LOG"):
        with open(os.environ["XVEC_VBX_ERRORS_LOG"], "a") as f:
            f.write(line + "\n")


def _assert_parity(got, refs, what):
    """`got` (one recording) against the longdouble run refs["ld"], at MARGIN x the fp64 restatements' own distances."""
    ld = refs["ld"]
    d_log, d_scaled = vbx_ref.distances(refs["log"], ld), vbx_ref.distances(refs["scaled"], ld)
    d_got = vbx_ref.distances((got["gamma"], got["pi"][0], got["elbo"][0]), ld)
    bars = [MARGIN * max(a, b) for a, b in zip(d_log, d_scaled)]
    _log(f"[vbx] {what}: device gamma {d_got[0]:.2e} pi {d_got[1]:.2e} elbo {d_got[2]:.2e} | log-domain fp64 {d_log[0]:.2e} "
         f"{d_log[1]:.2e} {d_log[2]:.2e} | scaled fp64 {d_scaled[0]:.2e} {d_scaled[1]:.2e} {d_scaled[2]:.2e} | ratio to the bar "
         + " ".join("%.2f" % (g / b) if b > 0 else ("0" if g == 0 else "inf") for g, b in zip(d_got, bars)))
    assert np.isfinite(got["gamma"]).all() and np.isfinite(got["pi"]).all()
    for name, g, b in zip(("gamma", "pi", "elbo"), d_got, bars):
        assert g <= b, f"{what}: {name} is {g:.3e} from the longdouble run, the bar is {b:.3e}"
    want_labels, want_count = vbx_ref.labels_of(np.asarray(ld[0], dtype=np.float64))
    assert np.array_equal(got["labels"], want_labels), (what, "labels")
    assert got["n_speakers"].tolist() == [want_count], (what, got["n_speakers"], want_count)


# ---------------------------------------------------------------- parity at the kernel's boundaries

@pytest.mark.parametrize("name", list(vbx_ref.CASES))
def test_parity_with_the_longdouble_run(name):
    T, D, S, _, _, _, n_iter = vbx_ref.CASES[name]
    X, phi, gamma0, pi0 = vbx_ref.case_data(name)
    got = _run(X, phi, gamma0, pi0, [0, T], n_iter)
    assert got["untouched"] and got["iters"].tolist() == [n_iter] and not np.isnan(got["elbo"]).any()
    _assert_parity(got, vbx_ref.case_refs(name), f"{name} (T = {T}, D = {D}, S = {S}, {n_iter} iterations)")
    if T <= 1024:
        _same(_run(X, phi, gamma0, pi0, [0, T], n_iter, fill_ws=0xFF), got, f"{name}: second run, NaN in the workspace")


@pytest.mark.parametrize("name", vbx_ref.STOP_CASES)
def test_stop_rule_runs_the_reference_s_iterations(name):
    T = vbx_ref.CASES[name][0]
    X, phi, gamma0, pi0 = vbx_ref.case_data(name)
    ref = vbx_ref.case_refs(name, epsilon=1e-4, max_iter=40)["ld"]
    got = _run(X, phi, gamma0, pi0, [0, T], 40, epsilon=1e-4)
    print(f"[vbx] {name}: stopped after {got['iters'][0]} iterations (reference: {ref[3]})")
    assert 2 <= ref[3] < 40 and got["iters"].tolist() == [ref[3]]
    assert not np.isnan(got["elbo"][0, :ref[3]]).any() and np.isnan(got["elbo"][0, ref[3]:]).all()
    want_labels, want_count = vbx_ref.labels_of(np.asarray(ref[0], dtype=np.float64))
    assert np.array_equal(got["labels"], want_labels) and got["n_speakers"].tolist() == [want_count]


@pytest.mark.parametrize("loop_prob", [0.0, 0.5, 0.9999])
def test_extreme_loop_probabilities(loop_prob):
    X, phi, gamma0, pi0 = vbx_ref.case_data("issue65")
    kw = dict(loop_prob=loop_prob, Fa=0.3, Fb=17.0, max_iter=10, epsilon=-INF)
    refs = {"ld": vbx_ref.vbx_log(X, phi, gamma0, pi0, dtype=np.longdouble, **kw), "log": vbx_ref.vbx_log(X, phi, gamma0, pi0, **kw),
            "scaled": vbx_ref.vbx_scaled(X, phi, gamma0, pi0, **kw)}
    got = _run(X, phi, gamma0, pi0, [0, 65], 10, loop_prob=loop_prob)
    _assert_parity(got, refs, f"loop_prob = {loop_prob}")


def test_saturated_emissions_are_finite_and_match():
    X, phi, gamma0, pi0 = vbx_ref.case_data("issue65")
    X = 6.0 * X
    kw = dict(loop_prob=0.99, Fa=30.0, Fb=30.0, max_iter=10, epsilon=-INF)
    refs = {"ld": vbx_ref.vbx_log(X, phi, gamma0, pi0, dtype=np.longdouble, **kw), "log": vbx_ref.vbx_log(X, phi, gamma0, pi0, **kw),
            "scaled": vbx_ref.vbx_scaled(X, phi, gamma0, pi0, **kw)}
    g = np.asarray(refs["ld"][0], dtype=np.float64)
    assert (np.abs(g.max(axis=1) - 1.0) < 1e-12).all()          # the reference's gamma is saturated
    got = _run(X, phi, gamma0, pi0, [0, 65], 10, Fa=30.0, Fb=30.0)
    assert np.isfinite(got["elbo"]).all()
    _assert_parity(got, refs, "Fa = Fb = 30, X scaled by 6")


def test_dead_speakers_on_entry_stay_dead():
    X, phi, gamma0, _ = vbx_ref.case_data("issue65")
    pi0 = np.array([0.4, 0.0, 0.3, 0.0, 0.2, 0.1])
    kw = dict(loop_prob=0.99, Fa=0.3, Fb=17.0, max_iter=10, epsilon=-INF)
    with np.errstate(invalid="ignore", divide="ignore"):
        refs = {"ld": vbx_ref.vbx_log(X, phi, gamma0, pi0, dtype=np.longdouble, **kw), "log": vbx_ref.vbx_log(X, phi, gamma0, pi0, **kw),
                "scaled": vbx_ref.vbx_scaled(X, phi, gamma0, pi0, **kw)}
    got = _run(X, phi, gamma0, pi0, [0, 65], 10)
    assert (_bits(got["gamma"][:, [1, 3]]) == 0).all() and (_bits(got["pi"][0, [1, 3]]) == 0).all()
    assert not np.isin(np.argmax(got["gamma"], axis=1), [1, 3]).any()
    _assert_parity(got, refs, "pi = 0 for speakers 1 and 3 on entry")


def test_surplus_speakers_lose_their_prior_and_take_no_label():
    T, D, K, S = 300, 16, 3, 12
    X, phi, spk = vbx_ref.planted(T, D, K, seed=77, sep=2.0)
    gamma0, pi0 = vbx_ref.init_gamma(vbx_ref.noisy_labels(spk, S, 77), S, 5.0)
    ref = vbx_ref.vbx_scaled(X, phi, gamma0, pi0, max_iter=40, epsilon=-INF, **vbx_ref.OPTS)
    got = _run(X, phi, gamma0, pi0, [0, T], 40)
    raw = np.argmax(got["gamma"], axis=1)
    used = np.unique(raw)
    assert got["n_speakers"].tolist() == [len(used)] == [K] and np.array_equal(used, np.unique(np.argmax(ref[0], axis=1)))
    surplus = np.setdiff1d(np.arange(S), used)
    print(f"[vbx] surplus speakers: largest pi {got['pi'][0, surplus].max():.2e}")
    assert got["pi"][0, surplus].max() < 1e-6 and abs(got["pi"][0, used].sum() - 1.0) < 1e-6
    assert np.array_equal(got["labels"], vbx_ref.labels_of(ref[0])[0])


# ---------------------------------------------------------------- exactness

def _batch(seed0=500, D=12, S=5):
    rs = _starts(BATCH)
    parts = []
    for r, n in enumerate(BATCH):
        X, phi_r, spk = vbx_ref.planted(n, D, 3, seed0 + r, sep=1.5)
        parts.append((X, vbx_ref.init_gamma(vbx_ref.noisy_labels(spk, S, seed0 + r), S, 5.0)[0]))
    phi = vbx_ref.planted(4, D, 1, seed0)[1]
    X = np.concatenate([p[0] for p in parts])
    gamma0 = np.concatenate([p[1] for p in parts])
    pi0 = np.full((len(BATCH), S), 1.0 / S)
    return rs, X, phi, gamma0, pi0


def test_a_recording_alone_equals_itself_inside_a_strided_batch():
    rs, X, phi, gamma0, pi0 = _batch()
    D, S = X.shape[1], gamma0.shape[1]
    plain = _run(X, phi, gamma0, pi0, rs, 6, epsilon=1e-4)
    odd = _run(X, phi, gamma0, pi0, rs, 6, epsilon=1e-4, ldx=D + 3, ldg=S + 2, odd=True, fill_ws=0xFF)
    assert odd["untouched"] and odd["around_is_nan"]
    _same(odd, plain, "strides, an odd base, NaN around the blocks and in the workspace")
    for r in range(len(BATCH)):
        lo, hi = int(rs[r]), int(rs[r + 1])
        alone = _run(X[lo:hi], phi, gamma0[lo:hi], pi0[r:r + 1], [0, hi - lo], 6, epsilon=1e-4)
        for k, sl in (("gamma", slice(lo, hi)), ("labels", slice(lo, hi)), ("pi", slice(r, r + 1)), ("elbo", slice(r, r + 1)),
                      ("iters", slice(r, r + 1)), ("n_speakers", slice(r, r + 1))):
            a, b = alone[k], plain[k][sl]
            assert np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), (r, k)
    only = _run(X, phi, gamma0, pi0, rs, 6, epsilon=1e-4, outputs=False)             # without labels and n_speakers
    assert _same_floats(only, plain) and np.array_equal(only["iters"], plain["iters"]) and (only["labels"] == -7).all()


def test_inside_a_workspace_window_of_the_reported_size():
    from xvector_amd import hip
    rs, X, phi, gamma0, pi0 = _batch()
    need = int(hip.lib.xvec_vbx_workspace_bytes(_i64(rs), len(BATCH), X.shape[1], gamma0.shape[1]))
    big, off = ss.window(need, DEV)                  # the window holds 0xFF bytes (NaN as float64): nothing is read unwritten
    got = _run(X, phi, gamma0, pi0, rs, 4, ws=big.data_ptr() + off)
    assert ss.guards_intact(big, off, need)
    plain = _run(X, phi, gamma0, pi0, rs, 4)
    assert _same_floats(got, plain) and np.array_equal(got["labels"], plain["labels"])


def test_a_nan_poisons_its_own_recording_only():
    rs, X, phi, gamma0, pi0 = _batch()
    clean = _run(X, phi, gamma0, pi0, rs, 4)
    bad = X.copy()
    r = 4
    bad[int(rs[r]) + 17, 3] = NAN
    got = _run(bad, phi, gamma0, pi0, rs, 4)
    lo, hi = int(rs[r]), int(rs[r + 1])
    assert np.isnan(got["gamma"][lo:hi]).all() and np.isnan(got["pi"][r]).all() and np.isnan(got["elbo"][r]).all()
    assert (got["labels"][lo:hi] == -1).all() and got["iters"][r] == 0 and got["n_speakers"][r] == 0
    keep = np.ones(len(X), dtype=bool)
    keep[lo:hi] = False
    recs = np.arange(len(BATCH)) != r
    assert np.array_equal(_bits(got["gamma"][keep]), _bits(clean["gamma"][keep])) and np.array_equal(got["labels"][keep], clean["labels"][keep])
    for k in ("pi", "elbo"):
        assert np.array_equal(_bits(got[k][recs]), _bits(clean[k][recs])), k
    assert np.array_equal(got["iters"][recs], clean["iters"][recs]) and np.array_equal(got["n_speakers"][recs], clean["n_speakers"][recs])
    inf_gamma = gamma0.copy()
    inf_gamma[0, 0] = INF                                        # ... and so does an infinity in gamma
    got = _run(X, phi, inf_gamma, pi0, rs, 4)
    assert np.isnan(got["gamma"][:int(rs[1])]).all() and (got["labels"][:int(rs[1])] == -1).all()
    assert np.array_equal(_bits(got["gamma"][int(rs[1]):]), _bits(clean["gamma"][int(rs[1]):]))


# ---------------------------------------------------------------- the initial assignment

@pytest.mark.parametrize("S,smoothing", [(1, 5.0), (5, 5.0), (64, 7.25), (10, 0.0)])
def test_init_matches_numpy_bit_for_bit(S, smoothing):
    from xvector_amd import hip
    counts = [3, 300, 1]
    rs = _starts(counts)
    N = int(rs[-1])
    rng = np.random.default_rng(S)
    labels = rng.integers(0, S, N).astype(np.int32)
    labels[[0, 5, 17, N - 1]] = [-1, S, 2 ** 31 - 1, -2 ** 31]      # outside 0 .. S - 1: the uniform row
    want_g, want_pi = vbx_ref.init_gamma(labels, S, smoothing)
    ldg = S + 3
    gd, gbuf = _strided(np.zeros((N, S)), ldg, odd=True)
    gd.fill_(7.5)
    pid = torch.full((len(counts), S), 7.5, dtype=torch.float64, device=DEV)
    rc = hip.lib.xvec_vbx_init(torch.from_numpy(labels).to(DEV).data_ptr(), _i64(rs), len(counts), S, smoothing, gd.data_ptr(), ldg,
                               pid.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_vbx_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(gd.cpu().numpy()), _bits(want_g))
    assert np.array_equal(_bits(pid.cpu().numpy()), _bits(np.tile(want_pi, (len(counts), 1))))
    assert int(torch.isnan(gbuf).sum()) == gbuf.numel() - N * S         # nothing outside the rows was written
    assert np.allclose(want_g.sum(axis=1), 1.0, rtol=0, atol=1e-15 * S)


# ---------------------------------------------------------------- the module and the chain

def test_vbx_module_call_equals_the_pieces():
    from xvector_amd import vbx as vbx_mod
    counts = [40, 64, 65, 130, 33, 70, 90, 257]
    rs = _starts(counts)
    D, S = 16, 6
    phi = vbx_ref.planted(4, D, 1, 900)[1]
    parts = [vbx_ref.planted(n, D, 3, 900 + r, sep=1.5) for r, n in enumerate(counts)]
    X = np.concatenate([p[0] for p in parts])
    ahc = np.concatenate([vbx_ref.noisy_labels(p[2], S, 900 + r) for r, p in enumerate(parts)])
    res = vbx_mod.vbx(torch.from_numpy(X).to(DEV), rs, phi, init_labels=torch.from_numpy(ahc).to(DEV), n_speakers=S, max_iter=8)
    assert res.labels.dtype == torch.int32 and res.gamma.shape == (len(X), S) and res.elbo.shape == (len(counts), 8) and res.labels.is_cuda
    gamma0, pi_row = vbx_ref.init_gamma(ahc, S, 5.0)
    by_hand = _run(X, phi, gamma0, np.tile(pi_row, (len(counts), 1)), rs, 8, epsilon=1e-4)
    got = dict(gamma=res.gamma.cpu().numpy(), pi=res.pi.cpu().numpy(), elbo=res.elbo.cpu().numpy(), iters=res.iters.cpu().numpy(),
               labels=res.labels.cpu().numpy(), n_speakers=res.n_speakers.cpu().numpy())
    _same(got, by_hand, "vbx() against xvec_vbx_init + xvec_vbx_run by hand")
    again = vbx_mod.vbx(torch.from_numpy(X).to(DEV), rs, phi, gamma=torch.from_numpy(gamma0).to(DEV), max_iter=8)
    assert torch.equal(again.labels, res.labels) and torch.equal(again.gamma, res.gamma)
    for r, n in enumerate(counts):                   # and the reference's labels, recording by recording
        lo, hi = int(rs[r]), int(rs[r + 1])
        ref = vbx_ref.vbx_scaled(X[lo:hi], phi, gamma0[lo:hi], pi_row, max_iter=8, epsilon=1e-4, **vbx_ref.OPTS)
        assert got["iters"][r] == ref[3] and np.array_equal(got["labels"][lo:hi], vbx_ref.labels_of(ref[0])[0]), r
    with pytest.raises(ValueError, match="init_labels or gamma"):
        vbx_mod.vbx(torch.from_numpy(X).to(DEV), rs, phi)
    with pytest.raises(ValueError, match="rec_start must rise"):
        vbx_mod.vbx(torch.from_numpy(X).to(DEV), rs[:-1], phi, init_labels=ahc, n_speakers=S)


def test_diarizer_with_resegment_equals_the_chain_by_hand(synth):
    import xvector_amd as xa
    from xvector_amd import diarize, vbx as vbx_mod
    from xvector_amd.scoring import cosine_scores
    cin, hid, xv, nc = 24, 72, 16, 3
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in
          synth.make_state_dict(706, input_size=cin, hidden_size=hid, num_classes=nc, x_vector_size=xv).items()}
    model = xa.XVectorModel(input_size=cin, hidden_size=hid, num_classes=nc, x_vector_size=xv)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    rng = np.random.default_rng(5)
    lengths = [960, 700, 400]
    x = synth.make_mfcc(3, max(lengths), seed=8)
    shift = rng.standard_normal(cin).astype(np.float32) * 1.5
    who = (np.arange(max(lengths)) // 120) % 2
    x += np.where(who[None, :, None] == 0, shift, -shift)
    xd = torch.from_numpy(x).to(DEV)
    win, hop = 60, 30
    vecs, windows = model.extract_windows(xd, win, hop, lengths=lengths)
    v64 = vecs.double()
    # a PLDA-shaped model of the windows' own statistics: the between-speaker part along the direction that separates the two
    host = v64.cpu().numpy()
    mean = host.mean(axis=0)
    Sigma = np.cov((host - mean).T) + 1e-3 * np.eye(xv)
    F = np.linalg.cholesky(Sigma)[:, :4] * 2.0
    vm = vbx_mod.VbxModel.from_plda(mean, F, Sigma)
    opts = vbx_mod.Vbx(vm, n_speakers=4, max_iter=10)
    plain = diarize.Diarizer(model, "cosine", win=win, hop=hop, max_score_rows=40, threshold=0.5, device=DEV)
    res_plain = plain.diarize(xd, lengths=lengths)
    d = diarize.Diarizer(model, "cosine", win=win, hop=hop, max_score_rows=40, threshold=0.5, device=DEV, resegment=opts)
    assert d.max_speakers == 4 and plain.max_speakers is None
    res = d.diarize(xd, lengths=lengths)
    counts = [int((windows[:, 0] == u).sum()) for u in range(3)]
    rs = _starts(counts)
    for a, b in d.calls(rs):
        lo, hi = int(rs[a]), int(rs[b])
        sub = rs[a:b + 1] - lo
        S = cosine_scores(v64[lo:hi], device=DEV)
        cl = diarize.cluster(S, sub, threshold=0.5, max_speakers=4)
        y = vm.project(v64[lo:hi], device=DEV)
        by_hand = vbx_mod.vbx(y, sub, vm.phi, init_labels=cl.labels, n_speakers=4, max_iter=10)
        assert np.array_equal(res.labels[lo:hi], by_hand.labels.cpu().numpy())
        assert np.array_equal(res.n_clusters[a:b], by_hand.n_speakers.cpu().numpy())
        assert (res.n_clusters[a:b] <= 4).all() and (res.labels[lo:hi] >= 0).all()
        # resegment = None: the clustering's labels, as before
        assert np.array_equal(res_plain.labels[lo:hi], diarize.cluster(S, sub, threshold=0.5).labels.cpu().numpy())
    assert np.array_equal(res.turns, diarize.turns(windows, res.labels))
