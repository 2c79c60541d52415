"""Speaker identification on the device (csrc/ident.hip, identify.py) against tests/ident_ref.py.

Model means.  Per element inside (n_c + 2) u sum |x| / n_c of the longdouble mean (n_c - 1 roundings of a sum in any order, one
of the division, one spare); two runs give the same bits.

Open-set scores.  Every finite cell inside
    u [(N + 8 + W_j) + 2 |L_ij| + |out_ij| + |S_ij|],      u = 2^-53, W_j = max_k |S_kj - m1_j|, L the subtracted logarithm,
of the longdouble reference (ident_ref.open_set_bound).  Derivation: the sum over k != i has N - 1 positive terms, so any order
of adding them, the merges' "+ 1" and rescaling products included, costs at most N u relative; every term is exp of a rounded
difference S - m1 (or a chain of such differences that telescopes to it), |x| u relative for an argument x with |x| <= W_j;
exp and log are correctly rounded to 1 ulp on the device (the HIP math library's documented figure for both in double
precision), which with the product p A, the quotient by N - 1, the (1 - p) term and the sum under the logarithm is the 8;
L = m1 + log(.) rounds twice at the scale of L; the final subtraction rounds at the scale of out, and S - m1 at the scale of
S.  The bound was fixed before the kernel ran; on the MI355X the largest error / bound of every N is printed, 0.55 at worst
(N = 3) in the first run, 0.23 at N = 385.  A column's bits
must not depend on T, ld, the base alignment or the other columns, and out = S in place must equal out of place.

Top-k.  Indices and scores EQUAL the stable-argsort reference."""
import numpy as np
import pytest
import torch

import ident_ref
import plda_oracle as po
import score_support as ss
from ident_ref import LD, U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
SLICE, BLOCK, TOPK_BLOCK, MAX_K = 32, 128, 512, 16          # tests/test_ident.py ties xvector_amd.identify's copies to the header


def _dev(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------- model means

COUNTS = [1, 2, 3, 4, 5, 9, 1, 5]          # rows per model: 1, 2, the walk's unroll of 4 and its neighbours, two trips + 1


def _enrolment(D, seed):
    """Vectors of len(COUNTS) models in interleaved order, names that do not sort in the order of first appearance."""
    rng = np.random.default_rng(seed)
    names = np.concatenate([[f"spk{(7 * c) % 10}_{c}"] * n for c, n in enumerate(COUNTS)])
    names = names[rng.permutation(names.shape[0])]
    x = rng.standard_normal((names.shape[0], D)) * 3 + rng.standard_normal(D)
    return x, names


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 512])
def test_model_means_inside_the_bound_and_bit_identical(D, dtype):
    from xvector_amd import identify
    x, names = _enrolment(D, D)
    x = x.astype(dtype)
    models, ref = ident_ref.model_means(x, names, LD)
    bound = ident_ref.model_mean_bound(x, names)
    got = identify.enroll(x, names, device=DEV)
    assert got.names.tolist() == models.tolist() and sorted(got.counts.tolist()) == sorted(COUNTS)
    assert got.vectors.shape == (len(COUNTS), D) and got.vectors.dtype == torch.float64
    g = got.vectors.cpu().numpy()
    err = np.abs(g.astype(LD) - ref).astype(np.float64)
    with np.errstate(all="ignore"):
        worst = float(np.max(err / bound, initial=0.0, where=bound > 0))
    print(f"[ident] model means D = {D}, {np.dtype(dtype).name}: largest error / bound {worst:.3f}")
    assert (err <= bound).all(), worst
    assert _same_bits(identify.enroll(x, names, device=DEV).vectors.cpu().numpy(), g)         # run to run
    # the same rows with a row stride (ld = D + 3) are read where they are and give the same bits
    wide = torch.full((x.shape[0], D + 3), 9.5, dtype=torch.float32 if dtype == np.float32 else torch.float64, device=DEV)
    wide[:, :D] = _dev(x, dtype)
    assert _same_bits(identify.enroll(wide[:, :D], names, device=DEV).vectors.cpu().numpy(), g)


# ---------------------------------------------------------------- open-set scores

KINDS = ["plain", "dominated", "equal_maxima", "all_plus_900", "all_minus_900", "minus_inf_row", "nan_cell"]
T_FULL = 257
T_SUB = [1, 63, 64, 65]


def _max_rows(N):
    """Rows the maximum is put at, column after column: the first row, the last row, one row of every slice."""
    return sorted({0, N - 1} | {min(s0 + (s0 // SLICE) % SLICE, N - 1) for s0 in range(0, N, SLICE)})


def _scores(N, kind, seed):
    rng = np.random.default_rng(seed)
    s = rng.normal(-20.0, 15.0, (N, T_FULL))
    at = np.array(_max_rows(N))[np.arange(T_FULL) % len(_max_rows(N))]
    cols = np.arange(T_FULL)
    if kind == "plain":
        s[at, cols] = s.max(axis=0) + 3.0
    elif kind == "dominated":
        s[at, cols] = s.max(axis=0) + 80.0
    elif kind == "equal_maxima":
        top = s.max(axis=0) + 1.0
        s[at, cols] = top
        s[(at + max(1, N // 2)) % N, cols] = top
    elif kind == "all_plus_900":
        s[:] = 900.0
    elif kind == "all_minus_900":
        s[:] = -900.0
    elif kind == "minus_inf_row":
        s[N // 2] = -INF
        s[at[:5], cols[:5]] = -INF                      # and where the maximum would have been
    elif kind == "nan_cell":
        s[at[::3], cols[::3]] = NAN                     # every third column has one
    return s


def _check_open_set(got, host, p, what, worst):
    out, L, W = ident_ref.open_set_longdouble(host, p)
    ref64 = out.astype(np.float64)
    fin = np.isfinite(ref64)
    assert np.array_equal(np.isnan(got), np.isnan(ref64)), what
    assert np.array_equal(got[~fin], ref64[~fin], equal_nan=True), what       # -inf cells stay -inf
    bound = ident_ref.open_set_bound(host, out, L, W)
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(LD) - out).astype(np.float64)
    ratio = float((err[fin] / bound[fin]).max()) if fin.any() else 0.0
    worst[0] = max(worst[0], ratio)
    assert (err[fin] <= bound[fin]).all(), (what, ratio)
    return out, bound, fin


@pytest.mark.parametrize("N", [2, 3, SLICE - 1, SLICE, SLICE + 1, 3 * SLICE + 1, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 1])
def test_open_set_scores_inside_the_bound_and_a_column_depends_on_itself_alone(N):
    from xvector_amd import identify
    worst = [0.0]
    for kind in KINDS:
        host = _scores(N, kind, 100 * N + len(kind))
        dev = _dev(host)
        for p in (0.1, 0.5, 1.0):
            what = f"N = {N}, {kind}, p = {p}"
            full = identify.open_set_scores(dev, p).cpu().numpy()
            out, bound, fin = _check_open_set(full, host, p, what, worst)
            if kind == "nan_cell":
                assert np.isnan(full[:, ::3]).all() and not np.isnan(full[:, 1::3]).any(), what
            if kind == "minus_inf_row":
                assert np.isneginf(full[N // 2]).all() if N > 2 else True, what
            if kind == "dominated":                     # the shortcut "column total minus own term" misses this bound
                with np.errstate(all="ignore"):
                    short = np.abs(ident_ref.total_minus_own(host, p).astype(LD) - out).astype(np.float64)
                assert not (short[fin] <= bound[fin]).all(), what
            inplace = dev.clone()
            assert identify.open_set_scores(inplace, p, out=inplace) is inplace
            assert _same_bits(inplace.cpu().numpy(), full), what
            # fewer columns, ld > T, a base that is 8 but not 16 bytes aligned, other values around: the same bits per column
            for T in T_SUB:
                buf = torch.full((N * (T + 5) + 2,), 3.25, dtype=torch.float64, device=DEV)
                off = 1 if buf.data_ptr() % 16 == 0 else 0
                sub = buf[off:off + N * (T + 5)].view(N, T + 5)
                assert sub.data_ptr() % 16 == 8
                c0 = T_FULL - T if T > 1 else 7         # not the leading columns: another lane, another tile
                sub[:, :T] = dev[:, c0:c0 + T]
                got = identify.open_set_scores(sub[:, :T], p)
                assert _same_bits(got.cpu().numpy(), full[:, c0:c0 + T]), (what, T)
                assert (sub[:, T:] == 3.25).all()
    print(f"[ident] open-set N = {N}: largest error / bound {worst[0]:.3f}")


def test_open_set_scores_inside_a_workspace_window_of_the_reported_size():
    from xvector_amd import hip, identify
    N, T, p = 3 * BLOCK + 1, 70, 0.3
    host = _scores(N, "dominated", 5)[:, :T]
    dev = _dev(host)
    want = identify.open_set_scores(dev, p).cpu().numpy()
    need = int(hip.lib.xvec_ident_workspace_bytes(N, T, 0))
    assert need >= (1 + 4) * T * 20
    big, off = ss.window(need, DEV)
    out = torch.empty((N, T), dtype=torch.float64, device=DEV)
    rc = hip.lib.xvec_open_set_scores(dev.data_ptr(), T, N, T, p, out.data_ptr(), T, big.data_ptr() + off, need,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_ident_last_error()
    torch.cuda.synchronize()
    assert ss.guards_intact(big, off, need)
    assert _same_bits(out.cpu().numpy(), want)


# ---------------------------------------------------------------- top-k

def _topk_scores(N, T, seed):
    """Small integers (many ties) with NaN cells, an all-NaN column, -inf, zeros of both signs, and columns whose best values
    are equal cells on both sides of every slice, wave and block edge."""
    rng = np.random.default_rng(seed)
    s = rng.integers(-4, 5, (N, T)).astype(np.float64)
    s[rng.random((N, T)) < 0.1] = NAN
    s[rng.random((N, T)) < 0.05] = -INF
    s[:, 1] = NAN                                        # nothing to select
    s[:, 2] = np.where(rng.random(N) < 0.5, -0.0, 0.0)   # the two zeros tie: row order
    s[:, 3] = NAN
    s[N // 2, 3] = -INF                                  # one selectable cell, and it is -inf
    col = 4
    for edge in (SLICE, BLOCK, TOPK_BLOCK, 2 * TOPK_BLOCK):
        if edge < N and col < T:
            s[:, col] = rng.integers(-4, 5, N)
            s[[edge - 1, edge], col] = 7.0               # the best two are equal and lie on both sides of the edge
            if edge + 1 < N:
                s[edge + 1, col] = 7.0
            col += 1
    s[:, T - 1] = 2.5                                    # every cell equal: 0, 1, 2, ...
    return s


@pytest.mark.parametrize("N", [1, 3, SLICE - 1, SLICE, SLICE + 1, BLOCK, BLOCK + 1, TOPK_BLOCK - 1, TOPK_BLOCK, TOPK_BLOCK + 1,
                               3 * TOPK_BLOCK + 1])
def test_topk_equals_the_stable_argsort(N):
    from xvector_amd import identify
    T = 130
    host = _topk_scores(N, T, N)
    dev = _dev(host)
    for k in (1, 2, 4, 5, MAX_K):                        # lists of 1, 4 and 16 places, and k > N for the small N
        idx, val = ident_ref.topk(host, k)
        thr = float(val[0, 0]) if np.isfinite(val[0, 0]) else 0.0          # exactly the best score of column 0
        got = identify.identify(dev, k, threshold=thr)
        gi, gv = got.idx.cpu().numpy(), got.scores.cpu().numpy()
        assert gi.dtype == np.int32 and gi.shape == (k, T)
        assert np.array_equal(gi, idx), (N, k)
        assert np.array_equal(np.isnan(gv), np.isnan(val)) and np.array_equal(_bits(gv)[~np.isnan(val)], _bits(val)[~np.isnan(val)])
        want = ident_ref.decide(idx, val, thr)
        assert np.array_equal(got.decision.cpu().numpy(), want), (N, k)
        if idx[0, 0] >= 0 and np.isfinite(val[0, 0]):
            assert want[0] == idx[0, 0]                  # a score equal to the threshold is accepted
        assert (gi[:, 1] == -1).all() and np.isnan(gv[:, 1]).all() and want[1] == -1
        assert gi[0, 3] == N // 2 and gv[0, 3] == -INF and (gi[1:, 3] == -1).all()
        assert np.array_equal(gi[:, T - 1], np.where(np.arange(k) < N, np.arange(k), -1))
        assert identify.identify(dev, k).decision is None
    # ld > T, a base that is 8 but not 16 bytes aligned: the same result
    buf = torch.full((N * (T + 3) + 2,), -1.5, dtype=torch.float64, device=DEV)
    off = 1 if buf.data_ptr() % 16 == 0 else 0
    sub = buf[off:off + N * (T + 3)].view(N, T + 3)
    sub[:, :T] = dev
    a, b = identify.identify(sub[:, :T], 5), identify.identify(dev, 5)
    assert torch.equal(a.idx, b.idx) and torch.equal(a.scores.nan_to_num(nan=-7.0), b.scores.nan_to_num(nan=-7.0))


def test_topk_inside_a_workspace_window_of_the_reported_size():
    from xvector_amd import hip
    N, T, k = 3 * TOPK_BLOCK + 1, 70, MAX_K
    host = _topk_scores(N, T, 9)
    dev = _dev(host)
    need = int(hip.lib.xvec_ident_workspace_bytes(N, T, k))
    assert need >= 4 * MAX_K * T * 12
    big, off = ss.window(need, DEV)
    idx = torch.empty((k, T), dtype=torch.int32, device=DEV)
    val = torch.empty((k, T), dtype=torch.float64, device=DEV)
    dec = torch.empty(T, dtype=torch.int32, device=DEV)
    rc = hip.lib.xvec_identify_topk(dev.data_ptr(), T, N, T, k, 1.0, idx.data_ptr(), val.data_ptr(), dec.data_ptr(),
                                    big.data_ptr() + off, need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_ident_last_error()
    torch.cuda.synchronize()
    assert ss.guards_intact(big, off, need)
    ri, rv = ident_ref.topk(host, k)
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(val.cpu().numpy(), rv, equal_nan=True)
    assert np.array_equal(dec.cpu().numpy(), ident_ref.decide(ri, rv, 1.0))


# ---------------------------------------------------------------- the chain

def _population(seed=17):
    """40 speakers, 3 to 5 enrolment vectors each in shuffled order, 200 test vectors of known speakers; D = 64, rank 20."""
    dim, rank = 64, 20
    mean, F, Sigma = po.make_plda(dim, rank, seed=seed)
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((40, rank)) @ F.T * 2.0 + mean
    counts = rng.integers(3, 6, 40)
    names = np.concatenate([[f"id{(13 * c) % 40:03d}"] * n for c, n in enumerate(counts)])
    who = np.concatenate([[c] * n for c, n in enumerate(counts)])
    perm = rng.permutation(names.shape[0])
    names, who = names[perm], who[perm]
    enrol = centres[who] + rng.standard_normal((names.shape[0], dim)) * 0.5
    t_who = rng.integers(0, 40, 200)
    test = centres[t_who] + rng.standard_normal((200, dim)) * 0.5
    t_names = np.array([f"id{(13 * c) % 40:03d}" for c in t_who])
    return (mean, F, Sigma), enrol, names, test, t_names


@pytest.fixture(scope="module")
def population():
    return _population()


@pytest.mark.parametrize("kind", ["plda", "cosine", "plda_snorm"])
def test_speaker_identifier_equals_its_pieces(kind, population):
    from xvector_amd import identify, snorm
    from xvector_amd.scoring import PldaScorer, cosine_scores
    (mean, F, Sigma), enrol, names, test, t_names = population
    k, p, thr = 5, 0.2, -1.0
    models = identify.enroll(enrol, names, device=DEV)
    ref_names, ref_means = ident_ref.model_means(enrol, names, LD)
    assert models.names.tolist() == ref_names.tolist() and len(ref_names) == 40
    mv = models.vectors.cpu().numpy()
    assert (np.abs(mv.astype(LD) - ref_means).astype(np.float64) <= ident_ref.model_mean_bound(enrol, names)).all()
    normalizer = None
    if kind == "cosine":
        scorer = "cosine"
        raw = cosine_scores(models.vectors, test, device=DEV)
        oracle = po.cosine_scoring(mv, test)
    else:
        scorer = PldaScorer(mean, F, Sigma, device=DEV)
        raw = scorer.score(models.vectors, test)
        oracle = po.fast_plda_scoring(mv, test, mean, F, Sigma)
    assert np.abs(raw.cpu().numpy() - oracle).max() / np.abs(oracle).max() < 1e-9
    if kind == "plda_snorm":
        cohort = np.random.default_rng(3).standard_normal((150, 64)) @ np.linalg.cholesky(F @ F.T + Sigma).T + mean
        normalizer = snorm.ScoreNormalizer(scorer, cohort, top_k=40, device=DEV)
        raw = normalizer.normalize(raw, models.vectors, _dev(test), mode="s")
    # the pieces, each against its host reference on the device's own input
    host = raw.cpu().numpy()
    opened = identify.open_set_scores(raw, p)
    _check_open_set(opened.cpu().numpy(), host, p, kind, [0.0])
    ri, rv = ident_ref.topk(opened.cpu().numpy(), k)
    ident = identify.SpeakerIdentifier(scorer, models, normalizer=normalizer, device=DEV)
    res = ident.identify(test, k=k, p_known=p, threshold=thr)
    assert np.array_equal(res.idx.cpu().numpy(), ri) and _same_bits(res.scores.cpu().numpy(), rv)
    assert np.array_equal(res.decision.cpu().numpy(), ident_ref.decide(ri, rv, thr))
    # closed set: the raw (or normalised) scores, no threshold
    closed = ident.identify(test, k=k)
    ci, cv = ident_ref.topk(host, k)
    assert closed.decision is None and np.array_equal(closed.idx.cpu().numpy(), ci) and _same_bits(closed.scores.cpu().numpy(), cv)
    # the hit rates against the known speakers
    truth = np.searchsorted(models.names, t_names)
    r1, rk = identify.identification_rate(closed.idx, truth)
    assert r1 == pytest.approx(float((ci[0] == truth).mean())) and rk == pytest.approx(float((ci == truth[None, :]).any(0).mean()))
    assert rk >= r1 > 0.5                                # the speakers are separable: most segments find their model
    assert identify.identification_rate(closed.idx.cpu().numpy(), truth) == (r1, rk)


class _Stat:      # the fields of StatObject_SB the path reads (plda_classifier.py:71-79)
    def __init__(self, ids, x):
        self.modelset = np.array(ids, dtype="|O")
        self.segset = np.array(ids, dtype="|O")
        self.stat1 = x


def test_fast_plda_scoring_averages_several_sessions_per_model(population, tmp_path):
    from xvector_amd import evaluate as ev, scoring
    (mean, F, Sigma), enrol, names, test, t_names = population
    seg_ids = [f"seg{j:04d}" for j in range(test.shape[0])]
    sc = scoring.fast_PLDA_scoring(_Stat(names.tolist(), enrol), _Stat(seg_ids, test), None, mean, F, Sigma, p_known=0.0)
    ref_names, ref_means = ident_ref.model_means(enrol, names)
    assert list(sc.modelset) == ref_names.tolist() == sorted(set(names.tolist())) and list(sc.segset) == seg_ids
    ref = po.fast_plda_scoring(ref_means, test, mean, F, Sigma)
    assert sc.scoremat.shape == (40, 200) and sc.scoremat.dtype == np.float64
    assert np.abs(sc.scoremat - ref).max() / np.abs(ref).max() < 1e-9
    # an ndx picks and orders models by their (unique) names
    ndx = scoring._Ndx(models=ref_names[[5, 2, 30]], testsegs=np.array(seg_ids[10:20]))
    part = scoring.fast_PLDA_scoring(_Stat(names.tolist(), enrol), _Stat(seg_ids, test), ndx, mean, F, Sigma)
    assert list(part.modelset) == ref_names[[5, 2, 30]].tolist()
    assert np.abs(part.scoremat - ref[[5, 2, 30], 10:20]).max() / np.abs(ref).max() < 1e-9
    # the model names go where the utterance ids went: a trial list over models and segments
    path = str(tmp_path / "trials.txt")
    with open(path, "w") as f:
        for j in range(0, 200, 7):
            f.write(f"1 {t_names[j]} {seg_ids[j]}\n0 {ref_names[(j + 1) % 40]} {seg_ids[j]}\n")
    trials = ev.TrialList.from_file(path, sc.modelset, sc.segset)
    assert len(trials) == 2 * len(range(0, 200, 7))
