"""Score normalisation on the device (csrc/snorm.hip, snorm.py) against tests/snorm_ref.py (np.longdouble).

Selection.  n_used and kth must EQUAL the reference (kth bit for bit, +0.0 for a zero of either sign) at every row length
around the kernel's own boundaries: the 512 threads of a block (one trip of a thread's loop or two), the two LDS images of the
resident regime (4096 and 16384 cells) and the switch to streamed rows beyond 16384.
Mean and std.  Per row, inside the bound snorm_ref.mean_bound / std_bound derive from the kernel's summation order: with
R = min(k - 1, ceil(C / 512) - 1 + 6 + 7 + 2) roundings on the way to a sum (never more than a plain left-to-right sum has),
  |mean - ref| <= 1.01 (R + 1) u sum |x| / k,        |std - ref| / ref <= 1.01 ((R + 4) / 2 + 1) u + (k u |mean| / std)^2.
A selection of k equal values has std exactly 0 (the kernel takes the value as the mean).  Every case prints its largest
error / bound.
Apply.  Three roundings lie on each term's path (difference, quotient; the weight 0.5 is exact) and one on their sum:
|out - ref| <= 3.03 u (|a| + |b|), a and b the two terms."""
import numpy as np
import pytest
import torch

import score_support as ss
import snorm_ref
from conftest import load_golden
from snorm_ref import U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
THREADS, SMALL, LARGE = 512, 4096, 16384            # tests/test_snorm.py ties xvector_amd.snorm's copies to the header
SIZES = [2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, THREADS - 1, THREADS, THREADS + 1, SMALL - 1, SMALL, SMALL + 1,
         LARGE - 1, LARGE, LARGE + 1]


def _dev(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _rows(C, n=300, seed=0):
    """Row 0 and rows 8 .. n - 1 from a seeded normal distribution; rows 1 .. 7 the special ones."""
    rng = np.random.default_rng(1000 + C + seed)
    s = rng.standard_normal((n, C))
    s[1] = 0.75                                                          # all equal
    s[2] = np.where(rng.random(C) < 0.5, 2.0, -1.0)                      # two distinct values: the cut falls inside a run of ties
    s[2, 0], s[2, -1] = 2.0, -1.0
    s[3] = np.sort(s[3])                                                 # ascending
    s[4] = np.sort(s[4])[::-1]                                           # descending
    s[5] = -np.abs(s[5]) - 0.5                                           # every value negative
    s[6, 0], s[6, C // 2] = INF, -INF                                    # +-inf are ordinary values
    s[7] = np.where(rng.random(C) < 0.5, -0.0, 0.0)                      # -0.0 mixed with +0.0, some negative values below them
    s[7, ::5] = -rng.random(s[7, ::5].size) - 0.1
    s[7, -1] = -0.0
    return s


def _stats(scores, top_k=0, skip=None):
    from xvector_amd import snorm
    st = snorm.cohort_stats(scores, top_k, skip)
    return tuple(t.cpu().numpy() for t in st)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _check(got, ref, C, what, worst=None):
    """got = (mean, std, kth, n_used) of the device, ref a snorm_ref.RowRef of the same rows."""
    mean, std, kth, n_used = got
    assert np.array_equal(n_used, ref.n_used), what
    few = ref.n_used < 2
    assert np.isnan(mean[few]).all() and np.isnan(std[few]).all() and np.isnan(kth[few]).all(), what
    rk = ref.kth.astype(np.float64)
    assert np.array_equal(kth[~few], rk[~few]) and not np.signbit(kth[~few][kth[~few] == 0]).any(), what
    rm, rs = ref.mean.astype(np.float64), ref.std.astype(np.float64)
    fin = ~few & np.isfinite(rm) & np.isfinite(rs)
    odd = ~few & ~fin                                   # an infinity in the selection: the same infinity or NaN as IEEE gives
    assert np.array_equal(mean[odd], rm[odd], equal_nan=True) and np.array_equal(std[odd], rs[odd], equal_nan=True), what
    em = np.abs(mean[fin].astype(snorm_ref.LD) - ref.mean[fin]).astype(np.float64)
    bm = snorm_ref.mean_bound(ref, C)[fin]
    flat = fin & (rs == 0)
    assert (std[flat] == 0).all(), what                 # k equal values
    sp = fin & (rs > 0)
    es = (np.abs(std[sp].astype(snorm_ref.LD) - ref.std[sp]) / ref.std[sp]).astype(np.float64)
    bs = snorm_ref.std_bound(ref, C)[sp]
    with np.errstate(all="ignore"):
        wm = float(np.max(em / bm, initial=0.0, where=bm > 0))
        ws = float(np.max(es / bs, initial=0.0))
    if worst is not None:
        worst[0], worst[1] = max(worst[0], wm), max(worst[1], ws)
    assert (em <= bm).all(), (what, wm)
    assert (es <= bs).all(), (what, ws)


# ---------------------------------------------------------------- selection, mean and std

@pytest.mark.parametrize("C", SIZES)
def test_selection_is_exact_and_the_sums_are_inside_their_bound(C):
    host = _rows(C)
    dev = _dev(host)
    rows = snorm_ref.sorted_valid(host)
    worst = [0.0, 0.0]
    for top_k in sorted({0, 2, 3, max(C - 1, 1), C, C + 5}):
        ref = snorm_ref.row_stats(host, top_k, rows=rows)
        assert (ref.n_used == (C if top_k == 0 else min(top_k, C))).all()
        full = _stats(dev, top_k)
        _check(full, ref, C, f"C = {C}, top_k = {top_k}, n = 300", worst)
        for n in (1, 5):
            part = _stats(dev[:n], top_k)
            for g, f in zip(part, full):                # the same rows: the same bits
                assert _same_bits(g, f[:n]) if g.dtype == np.float64 else np.array_equal(g, f[:n]), (C, top_k, n)
    print(f"[snorm] C = {C}: largest mean error / bound {worst[0]:.3f}, std {worst[1]:.3f}")


@pytest.mark.parametrize("top_k", [0, 200])
def test_ill_conditioned_rows(top_k):
    C = 1025
    host = 1e6 + np.random.default_rng(5).standard_normal((64, C))
    ref = snorm_ref.row_stats(host, top_k)
    worst = [0.0, 0.0]
    got = _stats(_dev(host), top_k)
    _check(got, ref, C, f"1e6 + N(0, 1), top_k = {top_k}", worst)
    err = np.abs(got[1] - ref.std.astype(np.float64)) / ref.std.astype(np.float64)
    print(f"[snorm] ill-conditioned, top_k = {top_k}: std error / bound {worst[1]:.3f}, largest relative error {err.max():.2e}")
    assert err.max() < 1e-9                             # a one-pass sum x^2 form is off by about 1e-2 here


def test_nan_cells_and_skipped_columns():
    C, n = 700, 12
    rng = np.random.default_rng(11)
    host = rng.standard_normal((n, C))
    host[0, rng.random(C) < 0.3] = NAN                  # NaN cells scattered in a row
    host[1] = NAN                                       # all NaN: n_used 0
    host[2] = NAN
    host[2, 17] = 1.5                                   # one valid cell: n_used 1, NaN outputs
    host[3] = NAN
    host[3, [5, 600]] = [2.0, -1.0]                     # two valid cells
    host[4, 9] = NAN
    skip = np.full(n, -1, dtype=np.int32)
    skip[4] = 9                                         # at a NaN cell
    skip[5] = int(np.argmax(host[5]))                   # at the row's maximum
    skip[6] = C - 1                                     # at the last column
    skip[7] = 0
    skip[2] = 17                                        # at the only valid cell: n_used 0
    dev = _dev(host)
    for top_k in (0, 2, 50, C):
        for sk in (None, skip):
            ref = snorm_ref.row_stats(host, top_k, sk)
            got = _stats(dev, top_k, None if sk is None else torch.from_numpy(sk).to(DEV))
            _check(got, ref, C, f"NaN / skip rows, top_k = {top_k}, skip = {sk is not None}")
            if sk is not None and top_k == 2:
                assert got[2][5] < host[5].max() and got[3][1] == 0 and got[3][2] == 0 and got[3][3] == 2
    ref = snorm_ref.row_stats(host, 0, skip)
    assert ref.n_used[4] == C - 1 and ref.n_used[5] == C - 1 and ref.n_used[8] == C


@pytest.mark.parametrize("C", [257, SMALL + 1, LARGE + 1])
def test_a_row_depends_on_nothing_but_itself(C):
    from xvector_amd import snorm
    host = _rows(C)
    r = 123
    for top_k in (0, 40):
        full = snorm.cohort_stats(_dev(host), top_k)
        again = snorm.cohort_stats(_dev(host), top_k)
        alone = snorm.cohort_stats(_dev(host[r:r + 1]), top_k)
        # the row with ld = C + 7, other values around it, from a base that is 8 but not 16 bytes aligned
        buf = torch.full((3 * (C + 7) + 2,), 3.25, dtype=torch.float64, device=DEV)
        off = 1 if buf.data_ptr() % 16 == 0 else 0
        wide = buf[off:off + 3 * (C + 7)].view(3, C + 7)
        assert wide.data_ptr() % 16 == 8
        wide[1, :C] = _dev(host[r])
        strided = snorm.cohort_stats(wide[:, :C], top_k)
        for f in range(4):
            a = full[f].cpu().numpy()
            assert _same_bits(a, again[f].cpu().numpy()) if f < 3 else np.array_equal(a, again[f].cpu().numpy())
            for other, at in ((alone, 0), (strided, 1)):
                b = other[f].cpu().numpy()
                assert _same_bits(a[r:r + 1], b[at:at + 1]) if f < 3 else a[r] == b[at], (C, top_k, f)


@pytest.mark.parametrize("C", [SMALL + 1, 10000, LARGE])
def test_the_resident_and_the_streamed_kernel_give_the_same_bits(C):
    """top_k = 0 streams a row of more than 4096 cells, top_k = C keeps it in LDS; both take every valid cell."""
    host = _rows(C, 40)
    host[9, ::7] = NAN
    dev = _dev(host)
    for a, b in zip(_stats(dev, 0), _stats(dev, C)):
        assert _same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b)


def test_row_stats_inside_a_workspace_window_of_the_reported_size():
    from xvector_amd import hip
    C, n, top_k = 300, 37, 20
    host = _rows(C, n)
    dev = _dev(host)
    want = _stats(dev, top_k)
    need = int(hip.lib.xvec_snorm_workspace_bytes(n, C))
    assert need > 0
    big, off = ss.window(need, DEV)
    vals = torch.empty((3, n), dtype=torch.float64, device=DEV)
    n_used = torch.empty(n, dtype=torch.int32, device=DEV)
    rc = hip.lib.xvec_snorm_row_stats(dev.data_ptr(), C, n, C, top_k, None, vals[0].data_ptr(), vals[1].data_ptr(),
                                      vals[2].data_ptr(), n_used.data_ptr(), big.data_ptr() + off, need,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_snorm_last_error()
    torch.cuda.synchronize()
    assert ss.guards_intact(big, off, need)
    for f in range(3):
        assert _same_bits(vals[f].cpu().numpy(), want[f])
    assert np.array_equal(n_used.cpu().numpy(), want[3])
    # the select records the call leaves there: the cut key's value is kth, n_above + the cells taken at the cut = n_used
    rec = big[off:off + 16 * n].cpu().numpy().view(np.uint64).reshape(n, 2)
    ref = snorm_ref.row_stats(host, top_k)
    n_above = (rec[:, 1] & 0xFFFFFFFF).astype(np.int64)
    assert np.array_equal((rec[:, 1] >> 32).astype(np.int64), np.full(n, C))
    rows = snorm_ref.sorted_valid(host)
    assert np.array_equal(n_above, [int((x > np.float64(ref.kth[i])).sum()) for i, x in enumerate(rows)])


# ---------------------------------------------------------------- apply

def _apply_case(n_rows, n_cols, seed, pad=0):
    from xvector_amd import snorm
    rng = np.random.default_rng(seed)
    host = rng.standard_normal((n_rows, n_cols)) * 3 + 1
    row = (rng.standard_normal(n_rows), rng.random(n_rows) + 0.5)
    col = (rng.standard_normal(n_cols), rng.random(n_cols) + 0.5)
    dev = _dev(host)
    drow, dcol = tuple(_dev(a) for a in row), tuple(_dev(a) for a in col)
    worst = 0.0
    for r, c, dr, dc in ((row, None, drow, None), (None, col, None, dcol), (row, col, drow, dcol)):
        ref = snorm_ref.apply(host, r, c)
        mag = (np.abs(snorm_ref.apply(host, r, None)) if r else 0) + (np.abs(snorm_ref.apply(host, None, c)) if c else 0)
        mag = mag * (0.5 if r and c else 1.0)           # |a| + |b| with the weight S-norm gives each term
        if pad:
            out = torch.full((n_rows, n_cols + pad), 7.5, dtype=torch.float64, device=DEV)
            got = snorm.apply_norm(dev, dr, dc, out=out[:, :n_cols])
            assert (out[:, n_cols:] == 7.5).all()       # ld_out > n_cols: the padding is not written
        else:
            got = snorm.apply_norm(dev, dr, dc)
        g = got.cpu().numpy()
        err = np.abs(g.astype(snorm_ref.LD) - ref).astype(np.float64)
        bound = 3.03 * U * mag.astype(np.float64)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (n_rows, n_cols, worst)
        inplace = dev.clone()
        assert snorm.apply_norm(inplace, dr, dc, out=inplace) is inplace
        assert _same_bits(inplace.cpu().numpy(), g)     # in place = out of place
    return worst


@pytest.mark.parametrize("shape", [(1, 1), (7, 255), (8, 256), (9, 257), (17, 513), (300, 40)])
def test_apply_z_t_s_at_the_tile_edges(shape):
    worst = max(_apply_case(*shape, seed=3), _apply_case(*shape, seed=4, pad=5))
    print(f"[snorm] apply {shape}: largest error / bound {worst:.3f}")


def test_apply_keeps_a_symmetric_matrix_symmetric_and_does_not_clamp():
    from xvector_amd import snorm
    n = 301
    rng = np.random.default_rng(9)
    a = rng.standard_normal((n, n))
    sym = _dev(a + a.T)
    st = snorm.cohort_stats(_dev(rng.standard_normal((n, 77)) * 2 + 0.3), top_k=30)
    out = snorm.apply_norm(sym, st, st)
    assert torch.equal(out, out.T.contiguous())
    # a standard deviation of 0 is not clamped: what IEEE 754 gives
    s = _dev([[1.0, 2.0], [3.0, 3.0]])
    z = snorm.apply_norm(s, row_stats=(_dev([0.0, 3.0]), _dev([0.0, 0.0]))).cpu().numpy()
    assert z[0, 0] == INF and z[0, 1] == INF and np.isnan(z[1]).all()


# ---------------------------------------------------------------- end to end

def _close_to_ref(stats, raw, top_k, skip=None):
    host = raw.cpu().numpy()
    ref = snorm_ref.row_stats(host, top_k, skip)
    _check(tuple(t.cpu().numpy() for t in stats), ref, host.shape[1], f"end to end, top_k = {top_k}")


@pytest.mark.parametrize("kind", ["plda", "cosine"])
def test_score_normalizer_end_to_end(kind, synth):
    from xvector_amd import snorm
    from xvector_amd.scoring import PldaScorer, cosine_scores
    dim, top_k = 64, 50
    rng = np.random.default_rng(21)
    cohort, enroll, test = rng.standard_normal((300, dim)), rng.standard_normal((40, dim)), rng.standard_normal((23, dim))
    if kind == "plda":
        scorer = PldaScorer(*synth.make_plda(dim, 16, seed=3), device=DEV)
        score = scorer.score
    else:
        scorer, score = "cosine", lambda e, t=None: cosine_scores(e, t, device=DEV)
    norm = snorm.ScoreNormalizer(scorer, cohort, top_k=top_k, device=DEV)
    st_e = norm.stats(enroll)
    _close_to_ref(st_e, score(enroll, cohort), top_k)
    # three chunks give the bits of one
    small = snorm.ScoreNormalizer(scorer, cohort, top_k=top_k, device=DEV, max_bytes=14 * 300 * 8)
    assert small.chunk_rows() == 14 and norm.chunk_rows() >= 40
    for a, b in zip(small.stats(enroll), st_e):
        assert torch.equal(a, b)
    # the cohort against itself, every vector's own column skipped
    own = np.arange(300, dtype=np.int32)
    st_c = norm.stats(cohort, skip_col=own)
    _close_to_ref(st_c, score(cohort, cohort), top_k, own)
    assert (st_c.n_used == top_k).all()
    # S-, Z- and T-norm of the trial scores against the reference formula on the device's own statistics
    raw = score(enroll, test)
    st_t = norm.stats(test)
    host = raw.cpu().numpy()
    pair = lambda st: (st.mean.cpu().numpy(), st.std.cpu().numpy())
    for mode, r, c in (("s", st_e, st_t), ("z", st_e, None), ("t", None, st_t)):
        got = norm.normalize(raw, enroll, test, mode=mode).cpu().numpy()
        ref = snorm_ref.apply(host, None if r is None else pair(r), None if c is None else pair(c))
        mag = sum(np.abs(snorm_ref.apply(host, pair(x) if i == 0 else None, pair(x) if i == 1 else None))
                  for i, x in enumerate((r, c)) if x is not None) * (0.5 if mode == "s" else 1.0)
        assert (np.abs(got.astype(snorm_ref.LD) - ref) <= 3.03 * U * mag).all(), mode
    # the self case: one set of statistics on both sides, a symmetric result
    self_raw = score(enroll)
    both = norm.normalize(self_raw, enroll)
    assert torch.equal(both, snorm.apply_norm(self_raw, st_e, st_e))


def test_z_norm_does_not_see_a_constant_added_to_a_row():
    """s and the row's cohort scores shifted by the same c: (s + c - (mean + c)) / std.  Every shifted input is off by its own
    rounding, e = u (|s| + |c|) at most; the mean moves by at most e besides its own (R + 1) u (|c| + |cohort|) of rounding,
    the deviations by 2 e, the std by about as much: |dz| <= (e + d_mean) / std + |z| d_std / std, bounded here by
    (R + 8) u (|c| + max |score|) / std (1 + |z|) with R = snorm_ref.sum_roundings."""
    from xvector_amd import snorm
    n, C, m = 40, 300, 23
    rng = np.random.default_rng(4)
    coh, tri = rng.standard_normal((n, C)) * 2 - 3, rng.standard_normal((n, m)) * 2 - 1
    c = rng.uniform(-1000, 1000, n)[:, None]
    plain = snorm.apply_norm(_dev(tri), row_stats=snorm.cohort_stats(_dev(coh), 60)).cpu().numpy()
    st = snorm.cohort_stats(_dev(coh + c), 60)
    moved = snorm.apply_norm(_dev(tri + c), row_stats=st).cpu().numpy()
    R = snorm_ref.sum_roundings(60, C)
    std = st.std.cpu().numpy()[:, None]
    bound = (R + 8) * U * (np.abs(c) + max(np.abs(coh).max(), np.abs(tri).max())) / std * (1 + np.abs(plain))
    ratio = np.abs(moved - plain) / bound
    print(f"[snorm] shifted rows: largest difference / bound {ratio.max():.3f}")
    assert (ratio <= 1).all()


class _Plda:
    pass


def test_plda_score_stat_object_with_a_cohort(tmp_path):
    import pandas as pd
    from xvector_amd import evaluate as ev, snorm
    from xvector_amd.scoring import PldaScorer
    g = load_golden("g8_trials.npz")
    path = str(tmp_path / "veri_test.txt")
    with open(path, "w") as f:
        f.write(str(g["trial_text"]))
    frame = pd.DataFrame({"index": np.arange(len(g["ids"])), "id": g["ids"].tolist(), "label": g["labels"],
                          "xvector": [str(v) for v in g["vectors"]]})
    plda = _Plda()
    plda.mean, plda.F, plda.Sigma = g["mean"], g["F"], g["Sigma"]
    x = g["read_vectors"]
    cohort = np.random.default_rng(13).standard_normal((90, x.shape[1])) * x.std() + x.mean(0)

    raw = ev.plda_score_stat_object(frame)
    raw.test_plda(plda, path)
    raw.calc_eer_mindcf()
    also = ev.plda_score_stat_object(frame)
    also.test_plda(plda, path, cohort=None, top_k=7)         # no cohort: every attribute as without the arguments
    also.calc_eer_mindcf()
    assert also.positive_scores == raw.positive_scores and also.negative_scores == raw.negative_scores
    assert (also.eer, also.eer_th, also.min_dcf, also.min_dcf_th) == (raw.eer, raw.eer_th, raw.min_dcf, raw.min_dcf_th)
    assert np.array_equal(also.plda_scores.scoremat, raw.plda_scores.scoremat)

    for top_k in (0, 25):
        obj = ev.plda_score_stat_object(frame)
        obj.test_plda(plda, path, cohort=cohort, top_k=top_k)
        obj.calc_eer_mindcf()
        scorer = PldaScorer(plda.mean, plda.F, plda.Sigma, device=DEV)
        st = snorm.cohort_stats(scorer.score(x, cohort), top_k)
        by_hand = snorm.apply_norm(scorer.score(x), st, st)
        want = ev.evaluate_trials(by_hand, ev.TrialList.from_file(path, g["ids"], g["ids"]), p_target=0.5)
        assert (obj.eer, obj.eer_th, obj.min_dcf, obj.min_dcf_th) == (want.eer, want.eer_th, want.min_dcf, want.min_dcf_th)
        assert np.array_equal(obj.plda_scores.scoremat, by_hand.cpu().numpy())
        assert obj.positive_scores != raw.positive_scores and len(obj.positive_scores) == len(raw.positive_scores)
        assert np.array_equal(obj.positive_scores_mask, raw.positive_scores_mask)
