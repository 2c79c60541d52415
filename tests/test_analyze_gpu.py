"""Score analysis on the device (csrc/analyze.hip through xvector_amd.analyze) against the numpy oracle tests/analyze_ref.py, at
the smallest shapes where each mechanism can go wrong: the wave, the slab of 256 trials, the tile of 2048 and the one size at
which a block of the persistent grid walks a second tile; every trial form; what is left out; a poisoned workspace of
exactly the reported size; a repeat call.  Integers (counts, positions, bins, records) are equal to the oracle's.  Moments lie
inside a bound the test computes from the data and the depth D of the kernel's summation tree (analyze.plan), with
g(k) = k u / (1 - k u), u = 2^-53 ("Score analysis"):
  mean   |err| <= dm = g(D + 2) sum|s| / n                                  (D additions, the conversion of n, the division)
  var    |err| <= g(D + 4) (V + dm^2) + dm^2                                (s - mean, the square, D additions, the division;
                                                                             sum (s - m')^2 = sum (s - m)^2 + n (m - m')^2)
  all    mean: D + 3; var: the classes' bounds weighed by n_c / n, the between-class terms n_c d_c^2 with d_c known to
         e_c = dm_c + dm_all, and g(4) V for the merge itself."""
import numpy as np
import pytest
import torch

import analyze_ref as ar
from test_evaluate_gpu import DEV

pytestmark = pytest.mark.gpu

TILE, SLAB, GRID = 2048, 256, 1024
U = 2.0 ** -53
SIZES = [1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


def g(k):
    return k * U / (1.0 - k * U)


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def run_summary(scores, rows, cols, tgt, bins=None, workspace=None, pairs=None):
    from xvector_amd import analyze
    s = scores if isinstance(scores, torch.Tensor) else _dev(np.atleast_2d(scores), np.float64)
    if pairs is not None:
        rc, cc, skip, upper = pairs
        return analyze._run_summary(s, None, None, None, s.shape[0] * s.shape[1], bins, workspace,
                                    (_dev(rc, np.int32), _dev(cc, np.int32), skip, upper))
    return analyze._run_summary(s, _dev(rows, np.int32), _dev(cols, np.int32), _dev(tgt, np.uint8), len(tgt), bins, workspace)


def run_hardest(scores, rows, cols, tgt, k, cand_cap=0, workspace=None, pairs=None):
    from xvector_amd import analyze
    s = scores if isinstance(scores, torch.Tensor) else _dev(np.atleast_2d(scores), np.float64)
    if pairs is not None:
        rc, cc, skip, upper = pairs
        return analyze._run_hardest(s, None, None, None, s.shape[0] * s.shape[1], k, cand_cap, workspace,
                                    (_dev(rc, np.int32), _dev(cc, np.int32), skip, upper))
    return analyze._run_hardest(s, _dev(rows, np.int32), _dev(cols, np.int32), _dev(tgt, np.uint8), len(tgt), k, cand_cap, workspace)


def check_moments(got, u, n_trials, exact=False):
    """Counts, extremes and positions equal to the oracle's; mean and var inside the bound of the module docstring."""
    from xvector_amd import analyze
    D = analyze.plan(n_trials)["sum_depth"]
    want = ar.summary(u)
    assert (got.n_nan, got.n_bad_index) == (u.n_nan, u.n_bad)
    dm, bound_v = [0.0] * 3, [0.0] * 3
    for c, (m, w) in enumerate(zip((got.nontarget, got.target, got.all), want)):
        assert (m.n, m.t_min, m.t_max) == (w["n"], w["t_min"], w["t_max"]), (c, m, w)
        if w["n"] == 0:
            assert all(np.isnan(x) for x in (m.min, m.max, m.mean, m.var))
            continue
        assert m.min == w["min"] and m.max == w["max"]
        s = u.of(c)[0]
        if not np.isfinite(s).all():
            with np.errstate(invalid="ignore"):
                ref_mean, ref_var = np.mean(s), np.var(s)
            assert (np.isnan(m.mean) and np.isnan(ref_mean)) or m.mean == ref_mean, (m.mean, ref_mean)
            assert np.isnan(m.var) and np.isnan(ref_var)
            continue
        V, mean = float(w["var"]), w["mean"]
        dm[c] = g(D + (3 if c == 2 else 2)) * float(np.abs(s).sum()) / w["n"]
        if c < 2 or want[0]["n"] == 0 or want[1]["n"] == 0:
            bound_v[c] = g(D + 4) * (V + dm[c] ** 2) + dm[c] ** 2
        else:
            bound_v[c] = g(4) * V
            for k in (0, 1):
                d, e, share = abs(float(want[k]["mean"] - mean)), dm[k] + dm[2], want[k]["n"] / w["n"]
                bound_v[c] += share * (bound_v[k] + 2 * d * e + e * e + g(4) * d * d)
        err_m, err_v = abs(float(np.longdouble(m.mean) - mean)), abs(float(np.longdouble(m.var) - w["var"]))
        print(f"class {c}: n {w['n']} mean err {err_m:.3e} (bound {dm[c]:.3e}) var err {err_v:.3e} (bound {bound_v[c]:.3e})")
        assert err_m <= dm[c] and err_v <= bound_v[c], (c, err_m, dm[c], err_v, bound_v[c])
        assert m.min <= m.mean <= m.max and m.var >= 0.0
        if exact:
            assert m.mean == s[0] and m.var == 0.0


def check_lists(got, u, k):
    want = ar.hardest(u, k)
    assert (got.n_nan, got.n_bad_index) == (u.n_nan, u.n_bad)
    for mine, theirs in zip((got.nontarget, got.target), want):
        assert len(mine) == len(theirs)
        assert mine.tobytes() == theirs.tobytes(), (mine[:5], theirs[:5])


def vector_case(n, seed=0, spread=9.0, offset=0.0, p_target=0.35):
    rng = np.random.default_rng(seed + n)
    tgt = (rng.random(n) < p_target).astype(np.uint8)
    return rng.normal(0.0, spread, n) + offset + 2.0 * spread * tgt, tgt


def vec_usable(s, tgt):
    return ar.usable_trials(s, None, None, tgt)


# ---------------------------------------------------------------- trial counts, both families

@pytest.mark.parametrize("n", SIZES)
def test_sizes_the_plain_vector(n):
    s, tgt = vector_case(n)
    u = vec_usable(s, tgt)
    from xvector_amd.analyze import Bins
    bins = Bins(first=-20, n_bins=64)
    got = run_summary(s, None, None, tgt, bins)
    check_moments(got, u, n)
    want = ar.histogram(u, 1.0, -20, 64, ar.RINT)
    assert np.array_equal(got.histogram.nontarget, want[0, 1:-1]) and np.array_equal(got.histogram.target, want[1, 1:-1])
    assert got.histogram.under == (want[0, 0], want[1, 0]) and got.histogram.over == (want[0, -1], want[1, -1])
    for k in (1, 200):
        check_lists(run_hardest(s, None, None, tgt, k), u, k)


def test_a_block_walks_a_second_tile():
    """The size the plan names: one trial more than the persistent grid has tiles' worth of blocks."""
    from xvector_amd import analyze
    n = analyze.plan(1)["second_tile_from"]
    assert n == GRID * TILE + 1 and analyze.plan(n)["most_tiles"] == 2 and analyze.plan(n - 1)["most_tiles"] == 1
    s, tgt = vector_case(n, seed=1)
    s[[5, TILE * GRID, TILE * GRID - 1]] = [90.0, 91.0, -90.0]
    tgt[[5, TILE * GRID, TILE * GRID - 1]] = [0, 0, 1]
    u = vec_usable(s, tgt)
    got = run_summary(s, None, None, tgt, analyze.Bins(first=-40, n_bins=100))
    check_moments(got, u, n)
    assert got.nontarget.t_max == TILE * GRID and got.target.t_min == TILE * GRID - 1
    want = ar.histogram(u, 1.0, -40, 100, ar.RINT)
    assert np.array_equal(got.histogram.nontarget, want[0, 1:-1]) and np.array_equal(got.histogram.target, want[1, 1:-1])
    check_lists(run_hardest(s, None, None, tgt, 65), u, 65)


def test_no_usable_trial_and_one_class_empty():
    s = np.full(70, np.nan)
    tgt = (np.arange(70) % 2).astype(np.uint8)
    u = vec_usable(s, tgt)
    got = run_summary(s, None, None, tgt)
    check_moments(got, u, 70)
    assert got.n_nan == 70 and got.all.n == 0
    hard = run_hardest(s, None, None, tgt, 5)
    assert len(hard.nontarget) == 0 == len(hard.target) and hard.n_nan == 70
    for only in (0, 1):
        s, _ = vector_case(300, seed=only)
        tgt = np.full(300, only, dtype=np.uint8)
        u = vec_usable(s, tgt)
        got = run_summary(s, None, None, tgt)
        check_moments(got, u, 300)
        mine, other = (got.target, got.nontarget) if only else (got.nontarget, got.target)
        assert other.n == 0 and (got.all.mean, got.all.var, got.all.sum) == (mine.mean, mine.var, mine.sum)      # bit for bit
        check_lists(run_hardest(s, None, None, tgt, 7), u, 7)


# ---------------------------------------------------------------- trial forms, what is left out, workspace, repeat

def list_case(seed, n, n_rows=37, n_cols=53, pad=4):
    rng = np.random.default_rng(seed)
    full = rng.normal(0.0, 9.0, (n_rows, n_cols + pad))
    rows, cols = rng.integers(0, n_rows, n), rng.integers(0, n_cols, n)
    tgt = (rng.random(n) < 0.3).astype(np.uint8)
    return full, rows, cols, tgt


def test_trial_list_with_nan_cells_and_bad_indices_counts_as_the_evaluation():
    from xvector_amd import analyze, hip
    full, rows, cols, tgt = list_case(2, 3 * TILE + 17)
    full[3, 4] = full[30, 50] = np.nan
    rows[[1, TILE, 2 * TILE + 5]] = [-1, 37, 3]
    cols[[2, TILE + 1, 2 * TILE + 5]] = [53, -2, 4]
    sd = _dev(full, np.float64)[:, :53]                          # ld = 57 > n_cols = 53
    assert sd.stride(0) == 57
    u = ar.usable_trials(full[:, :53], rows, cols, tgt)
    assert u.n_bad == 4 and u.n_nan >= 1
    bins = analyze.Bins(first=-10, n_bins=7, width=3.0, rounding=ar.FLOOR)
    got = run_summary(sd, rows, cols, tgt, bins)
    check_moments(got, u, len(tgt))
    want = ar.histogram(u, 3.0, -10, 7, ar.FLOOR)
    assert np.array_equal(got.histogram.nontarget, want[0, 1:-1]) and got.histogram.under == (want[0, 0], want[1, 0])
    check_lists(run_hardest(sd, rows, cols, tgt, 64), u, 64)
    # the counts are xvec_eval_trials' counts on the same inputs
    from xvector_amd import evaluate
    out = torch.empty(10, dtype=torch.float64, device=DEV)
    ws = evaluate._workspace(len(tgt), sd.device)
    rd, cd, td = _dev(rows, np.int32), _dev(cols, np.int32), _dev(tgt, np.uint8)
    rc = hip.lib.xvec_eval_trials(sd.data_ptr(), 57, 37, 53, rd.data_ptr(), cd.data_ptr(), td.data_ptr(), len(tgt), 1.0, 1.0, 0.5,
                                  out.data_ptr(), ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0
    n_t, n_n, n_nan, n_bad = out.cpu().view(torch.int64)[6:10].tolist()
    assert (n_t, n_n, n_nan, n_bad) == (got.target.n, got.nontarget.n, got.n_nan, got.n_bad_index)


@pytest.mark.parametrize("skip,upper", [(False, False), (True, False), (False, True), (True, True)])
def test_all_pairs_with_a_padded_matrix(skip, upper):
    from xvector_amd import analyze
    rng = np.random.default_rng(3)
    n_rows, n_cols = 71, 67                                      # 4757 cells: two tiles and a part
    full = rng.normal(0.0, 9.0, (n_rows, n_cols + 5))
    full[2, 2] = full[9, 4] = full[4, 9] = np.nan                # on the diagonal, below and above it
    rc, cc = rng.integers(0, 6, n_rows), rng.integers(0, 6, n_cols)
    sd = _dev(full, np.float64)[:, :n_cols]
    u = ar.usable_all_pairs(full[:, :n_cols], rc, cc, skip, upper)
    assert u.n_nan == (1 if upper else 2) + (0 if skip or upper else 1)
    bins = analyze.Bins(first=-128, n_bins=256, width=0.25)
    got = run_summary(sd, None, None, None, bins, pairs=(rc, cc, skip, upper))
    check_moments(got, u, n_rows * n_cols)
    want = ar.histogram(u, 0.25, -128, 256, ar.RINT)
    assert np.array_equal(got.histogram.nontarget, want[0, 1:-1]) and np.array_equal(got.histogram.target, want[1, 1:-1])
    assert got.histogram.under == (want[0, 0], want[1, 0]) and got.histogram.over == (want[0, -1], want[1, -1])
    check_lists(run_hardest(sd, None, None, None, 63, pairs=(rc, cc, skip, upper)), u, 63)


def test_poisoned_workspace_of_the_reported_size_and_a_repeat_call():
    from xvector_amd import analyze, hip
    n = 2 * TILE + 1
    s, tgt = vector_case(n, seed=4)
    bins = analyze.Bins(first=-20, n_bins=64)
    need_s = hip.lib.xvec_analyze_summary_workspace_bytes(n, 64)
    need_h = hip.lib.xvec_analyze_hardest_workspace_bytes(n, 200, 0)
    first = run_summary(s, None, None, tgt, bins)
    hard = run_hardest(s, None, None, tgt, 200)
    for _ in range(2):
        ws = torch.full((need_s,), 0xFF, dtype=torch.uint8, device=DEV)
        again = run_summary(s, None, None, tgt, bins, workspace=ws)
        for a, b in zip((first.nontarget, first.target, first.all), (again.nontarget, again.target, again.all)):
            assert np.array([a.mean, a.var, a.sum, a.min, a.max]).tobytes() == np.array([b.mean, b.var, b.sum, b.min, b.max]).tobytes()
            assert (a.n, a.t_min, a.t_max) == (b.n, b.t_min, b.t_max)
        assert np.array_equal(first.histogram.all, again.histogram.all)
        ws = torch.full((need_h,), 0xFF, dtype=torch.uint8, device=DEV)
        again = run_hardest(s, None, None, tgt, 200, workspace=ws)
        assert again.nontarget.tobytes() == hard.nontarget.tobytes() and again.target.tobytes() == hard.target.tobytes()


# ---------------------------------------------------------------- moments

def test_moments_with_a_common_offset():
    """Offset 1e6, unit spread: what sum x^2 - (sum x)^2 / n loses (1e12 u = 1e-4 of a variance of 1)."""
    n = 2 * TILE + 1
    s, tgt = vector_case(n, seed=5, spread=1.0, offset=1e6)
    got = run_summary(s, None, None, tgt)
    check_moments(got, vec_usable(s, tgt), n)
    assert abs(got.nontarget.var - 1.0) < 0.1 and abs(got.target.var - 1.0) < 0.1


@pytest.mark.parametrize("value", [0.1, -7.3, 1e6 + 0.1])
def test_moments_of_equal_scores_are_exact(value):
    n = 2 * TILE + 1
    tgt = (np.arange(n) % 3 == 0).astype(np.uint8)
    s = np.full(n, value)
    got = run_summary(s, None, None, tgt)
    check_moments(got, vec_usable(s, tgt), n, exact=True)
    assert (got.all.t_min, got.all.t_max, got.target.t_min, got.nontarget.t_min) == (0, 0, 0, 1)


def test_extremes_tied_across_thread_and_tile_edges():
    n = 2 * TILE + 1
    s, tgt = vector_case(n, seed=6, spread=1.0)
    tgt[:] = 0
    for at in ([SLAB - 1, SLAB], [TILE - 1, TILE], [2 * TILE, 70], [63, 64]):
        v = s.copy()
        lo = [(a + 3) % n for a in at]
        v[at], v[lo] = 50.0, -50.0
        got = run_summary(v, None, None, tgt)
        assert got.nontarget.t_max == min(at) and got.nontarget.t_min == min(lo) and got.all.t_max == min(at)
        check_moments(got, vec_usable(v, tgt), n)
    v = s.copy()
    v[[10, 300]] = [-0.0, 0.0]
    v[(v < 0) & (np.arange(n) != 10)] *= -1.0                    # the two zeros are the minimum: the lower t attains it
    assert run_summary(v, None, None, tgt).nontarget.t_min == 10


def test_infinite_scores_are_ordinary_values():
    n = TILE + 1
    from xvector_amd.analyze import Bins
    for put in ((np.inf,), (-np.inf,), (np.inf, -np.inf)):
        s, tgt = vector_case(n, seed=7)
        for i, x in enumerate(put):
            s[100 + 700 * i], s[1500 + 200 * i] = x, x
            tgt[100 + 700 * i], tgt[1500 + 200 * i] = 0, 1
        u = vec_usable(s, tgt)
        got = run_summary(s, None, None, tgt, Bins(first=-5, n_bins=11))
        check_moments(got, u, n)
        want = ar.histogram(u, 1.0, -5, 11, ar.RINT)
        assert got.histogram.under == (want[0, 0], want[1, 0]) and got.histogram.over == (want[0, -1], want[1, -1])
        assert got.n_nan == 0 and got.all.n == n
        check_lists(run_hardest(s, None, None, tgt, 3), u, 3)


# ---------------------------------------------------------------- histogram

@pytest.mark.parametrize("rounding", [ar.FLOOR, ar.RINT])
@pytest.mark.parametrize("n_bins", [1, 2, 64, 2061, 2062, 4094])
def test_histogram_equals_the_oracle(n_bins, rounding):
    from xvector_amd import analyze
    n = 2 * TILE + 1
    rng = np.random.default_rng(n_bins)
    tgt = (rng.random(n) < 0.4).astype(np.uint8)
    first = -(n_bins // 2)
    s = rng.normal(0.0, max(1.0, n_bins / 5.0), n)               # both ends are filled
    ties = np.arange(first - 2, first + n_bins + 2) + 0.5        # exact ties of rint, edges of floor
    s[: len(ties)] = ties[: n]
    room = len(s[len(ties): 2 * len(ties)])
    s[len(ties): len(ties) + room] = np.floor(ties)[: room]
    s[-4:], tgt[-4:] = [first - 5.0, first - 5.0, first + n_bins + 5.0, first + n_bins + 5.0], [0, 1, 0, 1]
    u = vec_usable(s, tgt)
    want = ar.histogram(u, 1.0, first, n_bins, rounding)
    assert want[:, 0].min() > 0 and want[:, -1].min() > 0
    copies = analyze.plan(n, n_bins)["hist_copies"]
    assert copies == (1 if n_bins >= 2062 else 2 if n_bins == 2061 else 32)
    for asked in sorted({0, 1, copies}):
        got = run_summary(s, None, None, tgt, analyze.Bins(first, n_bins, 1.0, rounding, asked)).histogram
        assert np.array_equal(got.nontarget, want[0, 1:-1]) and np.array_equal(got.target, want[1, 1:-1])
        assert got.under == (want[0, 0], want[1, 0]) and got.over == (want[0, -1], want[1, -1])
        assert np.array_equal(got.values, np.arange(first, first + n_bins, dtype=np.float64))
    # width 0.25: the lattice is finer, the map the same
    got = run_summary(s, None, None, tgt, analyze.Bins(4 * first, n_bins, 0.25, rounding)).histogram
    want = ar.histogram(u, 0.25, 4 * first, n_bins, rounding)
    assert np.array_equal(got.nontarget, want[0, 1:-1]) and got.over == (want[0, -1], want[1, -1])


def test_histogram_with_every_score_in_one_bin():
    from xvector_amd import analyze
    n = 2 * TILE + 1
    tgt = (np.arange(n) % 5 == 0).astype(np.uint8)
    s = np.full(n, 3.25)
    for copies in (0, 1):
        got = run_summary(s, None, None, tgt, analyze.Bins(0, 8, hist_copies=copies)).histogram
        assert got.target.tolist() == [0, 0, 0, int(tgt.sum()), 0, 0, 0, 0] and got.nontarget[3] == n - tgt.sum()
        assert got.under == (0, 0) == got.over and got.all.sum() == n


# ---------------------------------------------------------------- hardest

@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 200, 2048])
def test_hardest_equals_the_oracle(k):
    n = 3 * TILE + 5
    s, tgt = vector_case(n, seed=8)
    check_lists(run_hardest(s, None, None, tgt, k), vec_usable(s, tgt), k)


def test_hardest_with_k_above_a_class():
    s, tgt = vector_case(300, seed=9, p_target=0.1)
    u = vec_usable(s, tgt)
    got = run_hardest(s, None, None, tgt, 200)
    assert len(got.target) == int(tgt.sum()) < 200 and len(got.nontarget) == 200
    check_lists(got, u, 200)
    check_lists(run_hardest(s, None, None, tgt, 2048), u, 2048)


def test_hardest_of_equal_scores_goes_by_t_alone():
    n = 2 * TILE + 1
    tgt = (np.arange(n) % 2).astype(np.uint8)
    s = np.full(n, 1.5)
    for k, cap in ((65, 0), (300, 0), (2048, 0), (65, 65)):
        got = run_hardest(s, None, None, tgt, k, cap)
        assert got.nontarget["t"].tolist() == list(range(0, 2 * k, 2)) and got.target["t"].tolist() == list(range(1, 2 * k, 2))
    # across a tile edge: only the trials around it are non-targets
    tgt[:] = 1
    tgt[TILE - 2: TILE + 2] = 0
    got = run_hardest(s, None, None, tgt, 3)
    assert got.nontarget["t"].tolist() == [TILE - 2, TILE - 1, TILE]
    check_lists(got, vec_usable(s, tgt), 3)


def test_hardest_walks_to_the_last_digit():
    """Scores that differ in the last bits of the mantissa only: every digit pass but the last keeps them in one bucket."""
    n = TILE + 300
    rng = np.random.default_rng(10)
    tgt = (rng.random(n) < 0.5).astype(np.uint8)
    bits = np.float64(3.0).view(np.uint64) + rng.permutation(n).astype(np.uint64) % np.uint64(200)
    s = bits.view(np.float64)
    u = vec_usable(s, tgt)
    for cap in (0, 64):
        check_lists(run_hardest(s, None, None, tgt, 64, cap), u, 64)
    s = -s
    check_lists(run_hardest(s, None, None, tgt, 10, 64), vec_usable(s, tgt), 10)


def test_hardest_orders_by_the_double_not_its_float32_rounding():
    a, b = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -40
    assert np.float32(a) == np.float32(b) == np.float32(1.0) and a > b > 1.0
    s = np.array([1.0, b, a, 1.0, b, a, 0.5, 2.0])
    got = run_hardest(s, None, None, np.zeros(8, np.uint8), 6)
    assert got.nontarget["t"].tolist() == [7, 2, 5, 1, 4, 0]
    got = run_hardest(s, None, None, np.ones(8, np.uint8), 6)
    assert got.target["t"].tolist() == [6, 0, 3, 1, 4, 2] and len(got.nontarget) == 0


def test_hardest_with_a_small_candidate_cap_runs_further_passes():
    """A few thousand trials in one exponent bucket and room for 64 candidates: the digit passes go on over the trials; the
    result is the default cap's."""
    n = 2 * TILE + 100
    rng = np.random.default_rng(11)
    tgt = (rng.random(n) < 0.5).astype(np.uint8)
    s = 1.0 + rng.random(n)                                      # all in [1, 2): one exponent
    s[::7] = s[3]                                                # and a run of equal scores among them
    u = vec_usable(s, tgt)
    for k in (1, 64):
        small, default = run_hardest(s, None, None, tgt, k, 64), run_hardest(s, None, None, tgt, k)
        assert small.nontarget.tobytes() == default.nontarget.tobytes() and small.target.tobytes() == default.target.tobytes()
        check_lists(small, u, k)


def test_hardest_with_zeros_of_both_signs_and_infinities_at_the_ends():
    s = np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, np.inf, -np.inf, np.inf, -np.inf, 2.0, -2.0])
    for tgt in (np.zeros(12, np.uint8), np.ones(12, np.uint8), (np.arange(12) % 2).astype(np.uint8)):
        u = vec_usable(s, tgt)
        got = run_hardest(s, None, None, tgt, 12)
        check_lists(got, u, 12)
    got = run_hardest(s, None, None, np.zeros(12, np.uint8), 12)
    assert got.nontarget["t"].tolist() == [6, 8, 10, 2, 0, 1, 3, 4, 5, 11, 7, 9]
    assert np.signbit(got.nontarget["score"][5]) and not np.signbit(got.nontarget["score"][4])      # the records keep the sign


# ---------------------------------------------------------------- the Python layer

def test_plda_score_stat_object_analyze_and_compare_speaker_results(tmp_path):
    import pandas as pd
    from conftest import load_golden
    from xvector_amd import analyze
    from xvector_amd.evaluate import plda_score_stat_object
    from test_evaluate_gpu import _Plda
    g8 = load_golden("g8_trials.npz")
    path = str(tmp_path / "veri_test.txt")
    with open(path, "w") as f:
        f.write(str(g8["trial_text"]))
    frame = pd.DataFrame({"index": np.arange(len(g8["ids"])), "id": g8["ids"].tolist(), "label": g8["labels"],
                          "xvector": [str(v) for v in g8["vectors"]]})
    plda = _Plda()
    plda.mean, plda.F, plda.Sigma = g8["mean"], g8["F"], g8["Sigma"]
    obj = plda_score_stat_object(frame)
    with pytest.raises(RuntimeError, match="call test_plda first"):
        obj.analyze()
    obj.test_plda(plda, path)
    summ, hard = obj.analyze(k=20, bins=analyze.Bins(first=-200, n_bins=400))
    assert obj.score_summary is summ and obj.hardest is hard
    mat = obj._scoremat.cpu().numpy()
    tr = obj._trials
    u = ar.usable_trials(mat, tr.row_idx, tr.col_idx, tr.is_target)
    check_moments(summ, u, len(tr))
    check_lists(hard, u, 20)
    want = ar.histogram(u, 1.0, -200, 400, ar.RINT)
    assert np.array_equal(summ.histogram.target, want[1, 1:-1]) and summ.histogram.all.sum() + sum(summ.histogram.under) + \
        sum(summ.histogram.over) == len(tr)
    grid, dens = summ.histogram.density("target")
    rg, rd = ar.density(summ.histogram.values, summ.histogram.target)
    assert np.array_equal(grid, rg) and np.array_equal(dens, rd)
    # the reference script's numbers
    ids = g8["ids"].tolist()
    got, ref = analyze.compare_speaker_results(obj._scoremat, ids, ids, k=10), ar.compare_speaker_results(mat, ids, ids, k=10)
    assert got["false_pos"] == ref["false_pos"] and got["false_neg"] == ref["false_neg"] and len(got["false_pos"][1]) == 10
    spk = [x.split(".")[0].split("/")[0] for x in ids]
    full = analyze.score_summary_all_pairs(obj._scoremat, spk, spk, skip_diagonal=False)
    check_moments(full, ar.usable_all_pairs(mat, np.array(spk), np.array(spk), skip_diagonal=False), mat.size)
    for name, m in (("all", full.all), ("positive", full.target), ("negative", full.nontarget)):
        assert got[name] == dict(highest=m.max, lowest=m.min, mean=m.mean, variance=m.var)
        assert got[name]["highest"] == ref[name]["highest"] and got[name]["lowest"] == ref[name]["lowest"]
