"""The GMM-UBM unit on the device (csrc/gmm.hip through xvector_amd.gmm) against the numpy oracle tests/gmm_ref.py and the
scikit-learn fixture tests/golden/g13_gmm.npz, at shapes (N, C, D) on either side of the tiles of 64 frames and 64 components,
with K = 2 D below, at and past a chunk of 16, each with the slices of the global statistics forced to 1, 2 and 7.

TOLERANCES ARE MEASURED, NOT CHOSEN.  For every quantity the bar is MARGIN = 8 times the largest distance, on that test's own
inputs, between gmm_ref in fp64 and gmm_ref in np.longdouble: what fp64 arithmetic in numpy's order loses.  The margin covers
the device's different but equally bounded order (the MFMA's K order, the chunks of 64 frames, the slice tree).  Integer counts,
exact zeros and the selection rules are compared exactly.  With XVEC_GMM_ERRORS_LOG set, each comparison appends its measured
distance and the device's share of the bar to that file (profiles/gmm_errors.txt)."""
import functools
import os

import numpy as np
import pytest
import torch

import gmm_ref as gr
from conftest import ROOT
from test_evaluate_gpu import DEV

pytestmark = pytest.mark.gpu

MARGIN = 8
SHAPES = [(1, 1, 1), (65, 3, 1), (257, 63, 13), (300, 65, 24), (1000, 130, 36)]
SLICES = [1, 2, 7]
LD = np.longdouble


def _log(name, got_err, bar):
    path = os.environ.get("XVEC_GMM_ERRORS_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(f"{name:<58} fp64-vs-longdouble {bar / MARGIN:.3e}  bar {bar:.3e}  device {got_err:.3e}  share {got_err / bar if bar else 0:.3f}\n")


def close(name, got, ref64, refld, target=None):
    """`got` (device, fp64) within MARGIN x |ref64 - refld|_max of the longdouble oracle (or of `target`, a recorded fp64 result)."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref64, refld = np.asarray(ref64), np.asarray(refld)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    if got.size == 0:
        return
    bar = MARGIN * float(np.abs(ref64.astype(LD) - refld).max())
    err = float(np.abs(got.astype(LD) - (refld if target is None else np.asarray(target))).max())
    _log(name, err, bar)
    print(f"{name}: device {err:.3e} bar {bar:.3e}")
    assert np.isfinite(got).all(), name
    assert err <= bar, (name, err, bar)


@functools.lru_cache(maxsize=None)
def case(N, C, D, seed=0):
    """Planted data and a model near it: x [N, D], w, mu, v (numpy fp64, read-only)."""
    rng = np.random.default_rng(1000 * N + 10 * C + D + seed)
    centres = rng.normal(0.0, 2.0, (C, D))
    x = centres[rng.integers(0, C, N)] + rng.normal(0.0, 1.0, (N, D))
    w = rng.uniform(0.5, 1.5, C)
    w /= w.sum()
    mu = centres + rng.normal(0.0, 0.3, (C, D))
    v = rng.uniform(0.6, 1.6, (C, D))
    for a in (x, w, mu, v):
        a.setflags(write=False)
    return x, w, mu, v


@functools.lru_cache(maxsize=None)
def ref_loglik(N, C, D):
    x, w, mu, v = case(N, C, D)
    return gr.loglik(x, w, mu, v), gr.loglik(x, w, mu, v, dtype=LD)


@functools.lru_cache(maxsize=None)
def ref_global(N, C, D):
    x, w, mu, v = case(N, C, D)
    return gr.accumulate(x, w, mu, v), gr.accumulate(x, w, mu, v, dtype=LD)


def utts_of(N):
    """Four utterances that cut N frames at N / 3 and 2 N / 3, an empty one among them."""
    a, b = N // 3, (2 * N) // 3
    return np.array([0, a, a, b], np.int64), np.array([a, 0, b - a, N - b], np.int64)


def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def model(w, mu, v):
    from xvector_amd import gmm
    return gmm.DiagGmm(w, mu, v, device=DEV)


# ---------------------------------------------------------------- every call at every shape

@pytest.mark.parametrize("N,C,D", SHAPES)
def test_loglik_and_posteriors(N, C, D):
    x, w, mu, v = case(N, C, D)
    r64, rld = ref_loglik(N, C, D)
    m = model(w, mu, v)
    lse, llsum, cnt = m.log_likelihood(_t(x))
    close(f"loglik lse {N, C, D}", lse, r64["lse"], rld["lse"])
    close(f"loglik utt_llsum {N, C, D}", llsum, r64["utt_llsum"], rld["utt_llsum"])
    assert cnt.cpu().tolist() == r64["utt_frames"].tolist() == [N]
    gam = m.posteriors(_t(x))
    close(f"posteriors {N, C, D}", gam, r64["gamma"], rld["gamma"])
    P, g = m.prepared()
    P64, g64 = gr.prepare(w, mu, v)
    Pld, gld = gr.prepare(w, mu, v, LD)
    close(f"prepare g {N, C, D}", g, g64, gld)
    assert np.array_equal(P.cpu().numpy(), P64)              # one correctly rounded division each


@pytest.mark.parametrize("n_slices", SLICES)
@pytest.mark.parametrize("N,C,D", SHAPES)
def test_global_statistics(N, C, D, n_slices):
    from xvector_amd import gmm
    x, w, mu, v = case(N, C, D)
    r64, rld = ref_global(N, C, D)
    assert gmm.plan(N, C, D, n_slices=n_slices)["slices"] == n_slices
    n, f, s, llsum, cnt, n_bad = model(w, mu, v).estep(_t(x), n_slices=n_slices)
    for name, got in (("n", n), ("f", f), ("s", s)):
        close(f"estep {name} {N, C, D} slices {n_slices}", got, r64[name], rld[name])
    close(f"estep llsum {N, C, D} slices {n_slices}", llsum, [r64["llsum"]], [rld["llsum"]])
    assert (int(cnt.item()), int(n_bad.item())) == (N, 0)


@pytest.mark.parametrize("N,C,D", SHAPES)
def test_per_utterance_statistics_and_their_sum(N, C, D):
    x, w, mu, v = case(N, C, D)
    first, count = utts_of(N)
    r64 = gr.accumulate(x, w, mu, v, first, count, per_utt=True)
    rld = gr.accumulate(x, w, mu, v, first, count, per_utt=True, dtype=LD)
    m = model(w, mu, v)
    st = m.stats(_t(x), (first, count))
    close(f"stats n {N, C, D}", st.n, r64["n"], rld["n"])
    close(f"stats f {N, C, D}", st.f, r64["f"], rld["f"])
    close(f"stats llsum {N, C, D}", st.llsum, r64["llsum"], rld["llsum"])
    assert st.n_frames.cpu().tolist() == count.tolist() and st.n_bad == 0
    empty = np.flatnonzero(count == 0)
    assert len(empty) >= 1 or N < 3
    for u in empty:                                             # exact zeros, not small numbers
        assert not st.n[u].any() and not st.f[u].any() and float(st.llsum[u]) == 0.0
    # the global statistics are the per-utterance ones summed on the host: both lie within their bars of the same numbers,
    # so they differ by at most the global bar plus the utterances' bars added up
    g64, gld = ref_global(N, C, D)
    n, f, _, _, _, _ = m.estep(_t(x))
    for name, glob, per in (("n", n, st.n), ("f", f, st.f)):
        bar = MARGIN * (np.abs(g64[name].astype(LD) - gld[name]).max() + len(count) * np.abs(r64[name].astype(LD) - rld[name]).max())
        err = np.abs(glob.cpu().numpy() - per.cpu().numpy().sum(axis=0)).max()
        _log(f"global - sum of utterances {name} {N, C, D}", float(err), float(bar))
        assert err <= bar, (name, err, bar)


@pytest.mark.parametrize("N,C,D", SHAPES)
def test_mstep(N, C, D):
    x, w, mu, v = case(N, C, D)
    st = ref_global(N, C, D)[0]
    n, f, s = (np.asarray(st[k], np.float64) for k in ("n", "f", "s"))
    for opts in (dict(), dict(var_floor=0.9), dict(min_count=float(np.median(n)) if C > 1 else 0.0, reg_covar=1e-3)):
        m = model(w, mu, v)
        m.mstep(_t(n), _t(f), _t(s), torch.tensor([N], dtype=torch.int64, device=DEV), **opts)
        r64 = gr.mstep(n, f, s, N, mu, v, **opts)
        rld = gr.mstep(n, f, s, N, mu, v, dtype=LD, **opts)
        for name, got, a, b in zip(("w", "mu", "v"), (m.weights, m.means, m.variances), r64, rld):
            close(f"mstep {name} {N, C, D} {sorted(opts)}", got, a, b)
        if "min_count" in opts and C > 1:
            kept = n < opts["min_count"]
            assert kept.any() and np.array_equal(m.means.cpu().numpy()[kept], mu[kept]) and np.array_equal(m.variances.cpu().numpy()[kept], v[kept])
        if "var_floor" in opts:
            assert float(m.variances.min()) >= 0.9


@pytest.mark.parametrize("N,C,D", SHAPES)
def test_map_and_linear_scores(N, C, D):
    """Relevance MAP with its selection rule for n = 0, and linear scoring with its exact zeros, against the oracle."""
    from xvector_amd import gmm
    x, w, mu, v = case(N, C, D)
    first, count = utts_of(N)
    r = gr.accumulate(x, w, mu, v, first, count, per_utt=True)
    n, f = np.asarray(r["n"], np.float64), np.asarray(r["f"], np.float64)
    m = model(w, mu, v)
    stats = gmm.GmmStats(_t(n), _t(f))
    hat = gmm.map_adapt(m, stats, relevance=16.0)
    h64, hld = gr.map_means(n, f, mu, 16.0), gr.map_means(n, f, mu, 16.0, LD)
    close(f"map_means {N, C, D}", hat, h64, hld)
    zero = n == 0                                                # (the empty utterance: every component)
    assert zero.any() and np.array_equal(hat.cpu().numpy()[zero], np.broadcast_to(mu, hat.shape)[zero])
    S = gmm.linear_scores(m, _t(h64), stats)
    empty = np.flatnonzero(count == 0)
    assert not S[:, empty].any()                                 # a test utterance without frames scores exactly 0
    close(f"linear_scores {N, C, D}", S, gr.linear_scores(h64, n, f, mu, v), gr.linear_scores(h64, n, f, mu, v, LD))


def test_map_and_linear_scores_by_hand_on_the_device():
    """The two-component case of tests/test_gmm.py through gmm_map_kernel and the three score kernels: every value is a dyadic
    rational that fp64 holds, so the device's results are the hand-computed ones exactly."""
    from xvector_amd import gmm
    mu = np.array([[0.0, 2.0], [4.0, -2.0]])
    v = np.array([[1.0, 4.0], [2.0, 0.5]])
    n = np.array([[16.0, 0.0], [48.0, 16.0]])
    f = np.array([[[16.0, 48.0], [0.0, 0.0]], [[96.0, 0.0], [32.0, -64.0]]])
    m = model([0.5, 0.5], mu, v)
    hat = gmm.map_adapt(m, gmm.GmmStats(_t(n), _t(f)), relevance=16.0)
    assert hat.cpu().tolist() == [[[0.5, 2.5], [4.0, -2.0]], [[1.5, 0.5], [3.0, -3.0]]] == gr.map_means(n, f, mu, 16.0).tolist()
    tn, tf = np.array([[2.0, 2.0], [0.0, 0.0]]), np.array([[[2.0, 6.0], [6.0, -2.0]], [[0.0, 0.0], [0.0, 0.0]]])
    S = gmm.linear_scores(m, hat, gmm.GmmStats(_t(tn), _t(tf)))
    assert S.cpu().tolist() == [[0.3125, 0.0], [-0.1875, 0.0]]
    # what the binding refuses before the library reads a pointer
    for bad in (lambda: gmm.map_adapt(m, gmm.GmmStats(_t(n, torch.float32), _t(f))), lambda: gmm.map_adapt(m, gmm.GmmStats(_t(n).cpu(), _t(f))),
                lambda: gmm.map_adapt(m, gmm.GmmStats(_t(n), _t(f[:, :1]))), lambda: gmm.linear_scores(m, hat[:, :, :1], gmm.GmmStats(_t(tn), _t(tf))),
                lambda: gmm.linear_scores(m, hat.to(torch.float32), gmm.GmmStats(_t(tn), _t(tf))),
                lambda: gmm.linear_scores(m, hat, gmm.GmmStats(_t(tn[:1]), _t(tf)))):
        with pytest.raises(ValueError, match="expected a float64 tensor"):
            bad()


# ---------------------------------------------------------------- inputs

def test_fp32_equals_its_widened_copy_and_strides_do_not_matter():
    N, C, D = 300, 65, 24
    x, w, mu, v = case(N, C, D)
    x32 = _t(x, torch.float32)
    wide = x32.to(torch.float64)
    m = model(w, mu, v)
    a, b = m.estep(x32, n_slices=2), m.estep(wide, n_slices=2)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert torch.equal(m.log_likelihood(x32)[0], m.log_likelihood(wide)[0])
    pad = torch.full((N, D + 5), float("nan"), dtype=torch.float64, device=DEV)
    pad[:, :D] = wide
    c = m.estep(pad[:, :D], n_slices=2)
    assert pad[:, :D].stride(0) == D + 5 and all(torch.equal(p, q) for p, q in zip(b, c))
    first, count = utts_of(N)
    sa, sb = m.stats(x32, (first, count)), m.stats(pad[:, :D], (first, count))
    assert torch.equal(sa.n, sb.n) and torch.equal(sa.f, sb.f) and torch.equal(sa.llsum, sb.llsum)
    # and the fp32 run is the oracle's on the widened values
    r64, rld = gr.accumulate(wide.cpu().numpy(), w, mu, v), gr.accumulate(wide.cpu().numpy(), w, mu, v, dtype=LD)
    close("estep f (fp32 input)", a[1], r64["f"], rld["f"])


def test_utterance_lists_and_padding():
    from xvector_amd import gmm
    B, T, D, C = 5, 70, 13, 63
    _, w, mu, v = case(257, C, D)
    rng = np.random.default_rng(5)
    xb = rng.normal(0.0, 2.0, (B, T, D))
    lengths = np.array([70, 0, 1, 33, 64])
    poison = xb.copy()
    for b, n in enumerate(lengths):
        poison[b, n:] = [np.nan, np.inf, -np.inf][b % 3]
    xp = _t(poison)
    feats, utt = gmm.frames_of(xp, lengths)
    assert feats.data_ptr() == xp.data_ptr() and feats.shape == (B * T, D)             # no copy
    m = model(w, mu, v)
    st = m.stats(feats, utt)
    packed = np.concatenate([xb[b, :n] for b, n in enumerate(lengths)])
    pf, pc = np.concatenate([[0], np.cumsum(lengths)[:-1]]), lengths
    sp = m.stats(_t(packed), (pf, pc))
    assert st.n_bad == 0 and torch.equal(st.n, sp.n) and torch.equal(st.f, sp.f) and torch.equal(st.llsum, sp.llsum)   # padding is never read
    assert st.n_frames.cpu().tolist() == lengths.tolist()
    r64 = gr.accumulate(packed, w, mu, v, pf, pc, per_utt=True)
    rld = gr.accumulate(packed, w, mu, v, pf, pc, per_utt=True, dtype=LD)
    close("padded stats n", st.n, r64["n"], rld["n"])
    close("padded stats f", st.f, r64["f"], rld["f"])
    assert not st.n[1].any() and not st.f[1].any()
    g = m.estep(feats, utt, n_slices=2)
    gp = m.estep(_t(packed), (pf, pc), n_slices=2)
    assert all(torch.equal(a, b) for a, b in zip(g, gp)) and int(g[5].item()) == 0
    # overlapping ranges (sliding windows): a shared row is two frames
    of, oc = np.array([0, 10, 20, 5]), np.array([30, 30, 13, 1])
    so = m.stats(_t(packed), (of, oc))
    o64 = gr.accumulate(packed, w, mu, v, of, oc, per_utt=True)
    old = gr.accumulate(packed, w, mu, v, of, oc, per_utt=True, dtype=LD)
    close("overlapping stats n", so.n, o64["n"], old["n"])
    close("overlapping stats f", so.f, o64["f"], old["f"])
    lse = m.log_likelihood(_t(packed), (of, oc))[0]
    assert lse.shape[0] == 74 and torch.equal(lse[10:30], lse[30:50])      # rows 10 .. 29 as frames of two utterances


def test_zero_weight_far_component_far_frame_and_nan_frame():
    N, C, D = 257, 63, 13
    x, w, mu, v = case(N, C, D)
    w, mu, x = w.copy(), mu.copy(), x.copy()
    w[7] = 0.0
    w /= w.sum()
    mu[11] = 1e4                                                 # so far away that its posterior underflows
    x[100] = 60.0                                                # far from every component: exp(ll) underflows, lse must not
    m = model(w, mu, v)
    gam = m.posteriors(_t(x)).cpu().numpy()
    lse = m.log_likelihood(_t(x))[0].cpu().numpy()
    assert np.isfinite(gam).all() and not gam[:, 7].any() and not gam[:, 11].any()
    assert np.isfinite(lse).all() and lse[100] < -700.0
    r64, rld = gr.loglik(x, w, mu, v), gr.loglik(x, w, mu, v, dtype=LD)
    close("far frame lse", lse, r64["lse"], rld["lse"])
    close("posteriors with a zero weight", gam, r64["gamma"], rld["gamma"])
    close("posteriors sum to 1", gam.sum(axis=1), r64["gamma"].sum(axis=1), rld["gamma"].sum(axis=1))
    n = m.estep(_t(x))[0].cpu().numpy()
    assert n[7] == 0.0 and n[11] == 0.0 and np.isfinite(n).all()
    # a NaN frame and an Inf frame: counted once each, left out of everything
    bad = x.copy()
    bad[5, 3] = np.nan
    bad[200, 0] = np.inf
    first, count = utts_of(N)
    got = m.estep(_t(bad), n_slices=2)
    a64, ald = gr.accumulate(bad, w, mu, v), gr.accumulate(bad, w, mu, v, dtype=LD)
    assert (int(got[4].item()), int(got[5].item())) == (N - 2, 2) == (a64["n_frames"], a64["n_bad"])
    for name, t in zip(("n", "f", "s"), got[:3]):
        close(f"estep {name} with bad frames", t, a64[name], ald[name])
    close("estep llsum with bad frames", got[3], [a64["llsum"]], [ald["llsum"]])
    st = m.stats(_t(bad), (first, count))
    p64 = gr.accumulate(bad, w, mu, v, first, count, per_utt=True)
    assert st.n_bad == 2 and st.n_frames.cpu().tolist() == p64["n_frames"].tolist() and int(st.n_frames.sum()) == N - 2
    assert torch.isfinite(st.n).all() and torch.isfinite(st.f).all()
    pg = m.posteriors(_t(bad)).cpu().numpy()
    assert not pg[5].any() and not pg[200].any() and np.isfinite(pg).all()


def test_two_calls_are_bit_identical_whatever_the_workspace_held():
    from xvector_amd import gmm, hip
    N, C, D = 1000, 130, 36
    x, w, mu, v = case(N, C, D)
    m, xt = model(w, mu, v), _t(x)
    first, count = utts_of(N)
    for per_utt, slices in ((False, 7), (True, 0)):
        need = hip.lib.xvec_gmm_accumulate_workspace_bytes(N, len(first) if per_utt else 1, C, D, int(per_utt), slices)
        runs = []
        for fill in (0x00, 0xFF, None):
            ws = torch.randint(0, 256, (need,), dtype=torch.uint8, device=DEV) if fill is None else \
                torch.full((need,), fill, dtype=torch.uint8, device=DEV)
            if per_utt:
                st = m.stats(xt, (first, count), workspace=ws)
                runs.append((st.n, st.f, st.llsum, st.n_frames))
            else:
                runs.append(m.estep(xt, n_slices=slices, workspace=ws))
        for other in runs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(runs[0], other))
    assert gmm.plan(N, C, D, n_slices=7)["slice_frames"] == 192


# ---------------------------------------------------------------- EM

@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "g13_gmm.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("n_slices", SLICES)
def test_em_against_the_scikit_learn_fixture(golden, n_slices):
    from xvector_amd import gmm
    z = golden
    x, w0, mu0, v0 = z["x"], z["w0"], z["mu0"], z["v0"]
    m = model(w0, mu0, v0)
    lse = m.log_likelihood(_t(x))[0]
    r64, rld = gr.loglik(x, w0, mu0, v0), gr.loglik(x, w0, mu0, v0, dtype=LD)
    close("fixture score_samples", lse, r64["lse"], rld["lse"], target=z["score_samples"])
    close("fixture predict_proba", m.posteriors(_t(x)), r64["gamma"], rld["gamma"], target=z["predict_proba"])
    for k in (1, 10):
        m = gmm.fit_ubm(_t(x), 5, n_iter=k, tol=0.0, init=(w0, mu0, v0), n_slices=n_slices)
        e64, eld = gr.em(x, w0, mu0, v0, k), gr.em(x, w0, mu0, v0, k, dtype=LD)
        assert m.n_iter_ == k and len(m.lower_bounds) == k
        for name, got, a, b in zip(("w", "mu", "v"), (m.weights, m.means, m.variances), e64, eld):
            close(f"em {k} iterations {name} slices {n_slices}", got, a, b, target=z[f"{name}{k}"])      # against scikit-learn's numbers
        close(f"em {k} iterations lower bound slices {n_slices}", m.lower_bounds, e64[3], eld[3])
        recorded = np.append(eld[3][:-1], z[f"lb{k}"])          # scikit-learn's own last lower bound, under the bar of the k bounds
        close(f"em {k} iterations lower bound, the last against the fixture's, slices {n_slices}", m.lower_bounds, e64[3], eld[3], target=recorded)
        assert (np.diff(m.lower_bounds) >= -1e-12).all()


def test_em_stops_on_the_device_where_the_restatement_stops(golden):
    from xvector_amd import gmm
    z = golden
    x, w0, mu0, v0 = z["x"], z["w0"], z["mu0"], z["v0"]
    full = gr.em(x, w0, mu0, v0, 40)[3]
    steps = np.abs(np.diff(full))
    # a tolerance in the middle (in log) of the two successive steps of the lower bound that lie furthest apart: fp64 noise
    # cannot move the stop
    k = max(range(3, 9), key=lambda i: steps[i - 1] / steps[i])
    assert steps[k - 1] > 1.05 * steps[k] > 1e-9
    tol = float(np.sqrt(steps[k] * steps[k - 1]))
    want = gr.em(x, w0, mu0, v0, 40, tol=tol)
    assert want[4] == k + 2
    m = gmm.fit_ubm(_t(x), 5, n_iter=40, tol=tol, init=(w0, mu0, v0))
    assert m.n_iter_ == want[4] and len(m.lower_bounds) == want[4]
    eld = gr.em(x, w0, mu0, v0, 40, tol=tol, dtype=LD)
    close("em stopped: means", m.means, want[1], eld[1])
    one = gmm.fit_ubm(_t(x), 5, n_iter=3, tol=np.inf, init=(w0, mu0, v0))      # |change| = inf is not < inf: the first test never stops
    assert one.n_iter_ == 2


def test_em_that_stops_early_keeps_the_bad_frames_count_and_leaves_them_out(golden):
    """A NaN and an Inf frame in the fixture's data and a tolerance that stops EM long before max_iter: n_bad is that of the
    last iteration run (the spare iterations behind the stop must not touch it), and the model is the one of the data without
    the two frames."""
    from xvector_amd import gmm
    z = golden
    x, w0, mu0, v0 = z["x"], z["w0"], z["mu0"], z["v0"]
    bad = x.copy()
    bad[4, 2], bad[200, 0] = np.nan, np.inf
    clean = np.delete(x, [4, 200], axis=0)
    steps = np.abs(np.diff(gr.em(clean, w0, mu0, v0, 40)[3]))
    k = max(range(3, 9), key=lambda i: steps[i - 1] / steps[i])
    assert steps[k - 1] > 1.05 * steps[k] > 1e-9
    tol = float(np.sqrt(steps[k] * steps[k - 1]))
    e64, eld = gr.em(clean, w0, mu0, v0, 40, tol=tol), gr.em(clean, w0, mu0, v0, 40, tol=tol, dtype=LD)
    assert e64[4] == k + 2 < 40
    m = gmm.fit_ubm(_t(bad), 5, n_iter=40, tol=tol, init=(w0, mu0, v0))
    assert (m.n_iter_, m.n_bad) == (e64[4], 2)
    for name, got, a, b in zip(("w", "mu", "v"), (m.weights, m.means, m.variances), e64, eld):
        close(f"em stopped early, two bad frames: {name}", got, a, b)
    close("em stopped early, two bad frames: lower bounds", m.lower_bounds, e64[3], eld[3])
    full = gmm.fit_ubm(_t(bad), 5, n_iter=3, tol=0.0, init=(w0, mu0, v0))        # and when it runs to the end
    assert (full.n_iter_, full.n_bad) == (3, 2)


def test_fit_ubm_from_frames_never_takes_a_bad_frame_as_a_mean():
    from xvector_amd import gmm
    x = case(257, 63, 13)[0].copy()
    x[::2, 0] = np.nan                                           # every second frame is bad: any draw of 100 of 257 rows would hit one
    m = gmm.fit_ubm(_t(x), 100, n_iter=2, tol=0.0, seed=0)
    assert m.n_bad == 129 and m.n_iter_ == 2
    assert all(torch.isfinite(t).all() for t in (m.weights, m.means, m.variances)) and np.isfinite(m.lower_bounds).all()
    with pytest.raises(ValueError, match="distinct finite frames"):
        gmm.fit_ubm(_t(x), 129, n_iter=1)


def test_fit_ubm_from_frames_raises_the_lower_bound():
    from xvector_amd import gmm
    x, _, _, _ = case(1000, 130, 36)
    a = gmm.fit_ubm(_t(x, torch.float32), 16, n_iter=6, tol=0.0, seed=3)
    b = gmm.fit_ubm(_t(x, torch.float32), 16, n_iter=6, tol=0.0, seed=3)
    assert a.n_iter_ == 6 and (np.diff(a.lower_bounds) >= -1e-12).all() and a.lower_bounds[-1] > a.lower_bounds[0]
    assert torch.equal(a.means, b.means) and abs(float(a.weights.sum()) - 1.0) < 1e-12 and float(a.variances.min()) > 0


# ---------------------------------------------------------------- scores

def test_scores_feed_evaluate_trials_and_follow_the_exact_llr():
    import xvector_amd as xa
    from xvector_amd import gmm
    rng = np.random.default_rng(11)
    C, D, S, per = 8, 6, 6, 4                                    # six speakers, four utterances each, two to enrol
    centres = rng.normal(0.0, 3.0, (C, D))
    shift = rng.normal(0.0, 1.0, (S, C, D))
    utts, spk = [], []
    for s in range(S):
        for _ in range(per):
            comp = rng.integers(0, C, 80)
            utts.append(centres[comp] + shift[s, comp] + rng.normal(0.0, 1.0, (80, D)))
            spk.append(s)
    x = np.concatenate(utts)
    first, count = np.arange(len(utts)) * 80, np.full(len(utts), 80)
    ubm = gmm.fit_ubm(_t(x), C, utt=(first, count), n_iter=8, tol=0.0, seed=1)
    st = ubm.stats(_t(x), (first, count))
    enrol_rows = [u for u in range(len(utts)) if u % per < 2]
    test_rows = [u for u in range(len(utts)) if u % per >= 2]
    n_e = torch.stack([st.n[[u for u in enrol_rows if spk[u] == s]].sum(0) for s in range(S)])
    f_e = torch.stack([st.f[[u for u in enrol_rows if spk[u] == s]].sum(0) for s in range(S)])
    models = gmm.map_adapt(ubm, gmm.GmmStats(n_e, f_e), relevance=16.0)
    test = gmm.GmmStats(st.n[test_rows].contiguous(), st.f[test_rows].contiguous())
    scores = gmm.linear_scores(ubm, models, test)
    assert scores.shape == (S, len(test_rows)) and scores.dtype == torch.float64 and scores.is_cuda
    w, mu, v = (t.cpu().numpy() for t in (ubm.weights, ubm.means, ubm.variances))
    args = (models.cpu().numpy(), test.n.cpu().numpy(), test.f.cpu().numpy(), mu, v)
    close("linear_scores (verifier)", scores, gr.linear_scores(*args), gr.linear_scores(*args, dtype=LD))
    rows, cols = np.meshgrid(np.arange(S), np.arange(len(test_rows)), indexing="ij")
    tgt = np.array([[spk[u] == s for u in test_rows] for s in range(S)])
    res = xa.evaluate_trials(scores, xa.TrialList(rows.ravel(), cols.ravel(), tgt.ravel().astype(int)))
    assert 0.0 <= res.eer <= 0.25                                # planted speakers: the baseline separates them
    exact = gmm.llr_scores(ubm, models, _t(x), (first[test_rows], count[test_rows]))
    l64 = gr.llr(x, w, mu, v, models.cpu().numpy(), first[test_rows], count[test_rows])
    lld = gr.llr(x, w, mu, v, models.cpu().numpy(), first[test_rows], count[test_rows], dtype=LD)
    close("llr_scores", exact, l64, lld)
    assert np.corrcoef(exact.cpu().numpy().ravel(), scores.cpu().numpy().ravel())[0, 1] > 0.8
