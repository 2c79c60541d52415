"""The bootstrap on the device (csrc/boot.hip through xvector_amd.bootstrap) against the numpy restatement tests/boot_ref.py:
every record with equal integers and equal doubles, at the smallest shapes where the kernels can still go wrong -- the tile of
4096 trials and its 16 per thread, runs of equal scores over a thread and a tile edge, the group counts around the wave and
at the most, every mode, what is left out, a poisoned workspace, record 0 against the library's own evaluation, replicates
against the library's evaluation of the literally expanded list, independence of n_boot and of the batching, pairing, and
xvec_eval_sorted_order against a stable argsort.  Costs are the defaults, or powers of two where they are not: with those
every product of the detection cost is exact, so equal doubles do not depend on how the compiler fuses the sum."""
import ctypes as C

import numpy as np
import pytest
import torch

import boot_ref as br
from test_evaluate_gpu import DEV, host_keys

pytestmark = pytest.mark.gpu

TILE = 4096
FIELDS = ("eer", "eer_threshold", "far", "frr", "min_dcf", "min_dcf_threshold")


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _want(srt, n_boot, seed, joint, costs, replicates=None):
    recs, summary = br.bootstrap(srt, n_boot, seed, joint, *costs, replicates=replicates)
    rows = sorted(range(n_boot + 1) if replicates is None else replicates)
    doubles = np.array([[recs[b][f] for f in FIELDS] for b in rows], dtype=np.float64)
    counts = np.array([[recs[b]["n_target"], recs[b]["n_nontarget"]] for b in rows], dtype=np.int64)
    return rows, doubles, counts, summary


def _got(res):
    rec = res.records.cpu().numpy()
    return rec[:, :6], rec.view(np.int64)[:, 6:8]


def check(res, srt, n_boot, seed, joint=False, costs=(1.0, 1.0, 0.5), replicates=None):
    """Every record (or the listed ones) of `res` equal to the restatement's: integers and doubles, NaN where it has NaN."""
    rows, doubles, counts, summary = _want(srt, n_boot, seed, joint, costs, replicates)
    got_d, got_c = _got(res)
    assert got_d.shape[0] == n_boot + 1
    np.testing.assert_array_equal(got_c[rows], counts)
    np.testing.assert_array_equal(got_d[rows], doubles)
    assert (res.n_nan, res.n_bad_index, res.n_bad_group) == (summary["n_nan"], summary["n_bad_index"], summary["n_bad_group"])
    if replicates is None:
        assert (res.n_degenerate, res.n_overflow) == (summary["n_degenerate"], summary["n_overflow"])
    return doubles, counts


def run_trials(scores, rows, cols, tgt, rg=None, cg=None, g_rows=0, g_cols=0, joint=False, n_boot=12, seed=7,
               costs=(1.0, 1.0, 0.5), workspace=None):
    from xvector_amd import bootstrap
    s = _dev(np.atleast_2d(scores), np.float64)
    n = len(tgt)
    return bootstrap._run_trials(s, _dev(rows, np.int32), _dev(cols, np.int32), _dev(tgt, np.uint8), n, _dev(rg, np.int32),
                                 _dev(cg, np.int32), g_rows, g_cols, joint, n_boot, seed, *costs, workspace, "test", strict=False)


def matrix_case(seed, n, n_rows=61, n_cols=83, g_rows=7, g_cols=5, levels=0):
    """n trials over distinct-ish random cells of a [n_rows, n_cols] matrix; targets score higher; `levels`: quantised scores."""
    rng = np.random.default_rng(seed)
    rows, cols = rng.integers(0, n_rows, n), rng.integers(0, n_cols, n)
    tgt = (rng.random(n) < 0.3).astype(np.uint8)
    scores = rng.normal(0.0, 1.0, (n_rows, n_cols))
    scores[rows, cols] = rng.normal(0.0, 1.0, n) + 1.5 * tgt          # (a cell hit twice keeps the later value: still a trial list)
    tgt = (scores[rows, cols] + rng.normal(0, 0.7, n) > 1.0).astype(np.uint8)
    if levels:
        scores = np.round(scores * levels) / levels
    rg, cg = rng.integers(0, g_rows, n_rows), rng.integers(0, g_cols, n_cols)
    rg[:g_rows], cg[:g_cols] = np.arange(g_rows), np.arange(g_cols)     # every group occurs
    return scores, rows, cols, tgt, rg, cg


# ---------------------------------------------------------------- tile edges

@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_tile_edges(n):
    scores, rows, cols, tgt, rg, cg = matrix_case(n, n)
    res = run_trials(scores, rows, cols, tgt, rg, cg, 7, 5)
    check(res, br.Sorted.trials(scores, rows, cols, tgt, rg, cg, 7, 5), 12, 7)
    vec = np.random.default_rng(n).normal(0, 1, n) + tgt
    res = run_trials(vec, None, None, tgt, n_boot=9, seed=n)
    check(res, br.Sorted.trials(vec, None, None, tgt), 9, n)


# ---------------------------------------------------------------- equal scores

def test_runs_of_equal_scores_over_a_thread_edge_and_a_tile_edge():
    """Sorted position = trial index here (rising scores): one run over positions 10 .. 20 (the edge between the first two
    threads at 16), one over 4090 .. 4100 (the tile edge), both with targets and non-targets inside."""
    n = 2 * TILE + 3
    rng = np.random.default_rng(1)
    vec = np.arange(n, dtype=np.float64) / 64.0
    vec[10:21], vec[4090:4101] = vec[10], vec[4090]
    tgt = (rng.random(n) < np.linspace(0.1, 0.9, n)).astype(np.uint8)
    tgt[10:21:2], tgt[4090:4101:3] = 1, 0
    srt = br.Sorted.trials(vec, None, None, tgt)
    assert np.array_equal(srt.t, np.arange(n))
    check(run_trials(vec, None, None, tgt, n_boot=16, seed=3), srt, 16, 3)
    # and with groups: the same vector as the row 0 .. of a matrix, every column its own trial
    cg = rng.integers(0, 9, n)
    cols, rows = np.arange(n), np.zeros(n, dtype=np.int64)
    check(run_trials(vec, rows, cols, tgt, None, cg, 0, 9, n_boot=16, seed=3), br.Sorted.trials(vec, rows, cols, tgt, None, cg, 0, 9), 16, 3)


def test_all_scores_equal():
    """One run over three tiles: a single candidate, the last position, wherever the weights fall."""
    n = 2 * TILE + 3
    tgt = (np.arange(n) % 3 == 0).astype(np.uint8)
    vec = np.full(n, 0.25)
    doubles, _ = check(run_trials(vec, None, None, tgt, n_boot=8, seed=5), br.Sorted.trials(vec, None, None, tgt), 8, 5)
    assert (doubles[:, 1] == 0.25).all() and (doubles[:, 0] == 0.5).all()          # FRR = 1, FAR = 0 at the only threshold


def test_best_candidate_in_the_last_tile():
    """Non-targets on every position up to the first of the last tile, the two targets above: EER = 0 at position 8192."""
    n = 2 * TILE + 3
    vec = np.arange(n, dtype=np.float64)
    tgt = np.zeros(n, dtype=np.uint8)
    tgt[-2:] = 1
    srt = br.Sorted.trials(vec, None, None, tgt)
    doubles, _ = check(run_trials(vec, None, None, tgt, n_boot=24, seed=9), srt, 24, 9)
    assert doubles[0, 0] == 0.0 and doubles[0, 1] == 2.0 * TILE
    ok = ~np.isnan(doubles[1:, 0])
    assert ok.sum() >= 8 and (doubles[1:, 1][ok] >= 2.0 * TILE - 64).all()           # every evaluated replicate ends up there too
    # groups: the columns in groups of 512 neighbours, so that whole stretches of the order vanish from a replicate
    cols, rows, cg = np.arange(n), np.zeros(n, dtype=np.int64), np.arange(n) // 512
    check(run_trials(vec, rows, cols, tgt, None, cg, 0, 17, n_boot=24, seed=9), br.Sorted.trials(vec, rows, cols, tgt, None, cg, 0, 17), 24, 9)


# ---------------------------------------------------------------- group counts

@pytest.mark.parametrize("g", [1, 2, 63, 64, 65, 16384])
def test_group_counts(g):
    n_rows, n = max(g, 40), 5000
    scores, rows, cols, tgt, _, cg = matrix_case(g, n, n_rows=n_rows, n_cols=3, g_cols=3)
    rg = np.arange(n_rows) % g
    if g == 2:
        tgt = (rg[rows] == 0).astype(np.uint8)      # targets in one group, non-targets in the other: half the replicates lose a kind
    srt = br.Sorted.trials(scores, rows, cols, tgt, rg, None, g, 0)
    res = run_trials(scores, rows, cols, tgt, rg, None, g, 0, n_boot=20, seed=g)
    doubles, counts = check(res, srt, 20, g)
    if g == 1:      # one group drawn once: every replicate is the point estimate
        assert (doubles == doubles[0]).all() and (counts == counts[0]).all() and res.n_degenerate == 0
    if g == 2:
        assert 0 < res.n_degenerate < 20 and res.n_degenerate == int(np.isnan(doubles[1:, 0]).sum())
    # and on both sides, independently
    check(run_trials(scores, rows, cols, tgt, rg, cg, g, 3, n_boot=6, seed=g + 1), br.Sorted.trials(scores, rows, cols, tgt, rg, cg, g, 3), 6, g + 1)


# ---------------------------------------------------------------- modes

@pytest.mark.parametrize("mode", ["rows", "cols", "independent", "joint"])
def test_modes_of_a_trial_list(mode):
    scores, rows, cols, tgt, rg, cg = matrix_case(11, TILE + 1, g_rows=6, g_cols=6, levels=8)
    joint = mode == "joint"
    rgm = rg if mode != "cols" else None
    cgm = cg if mode != "rows" else None
    g0, g1 = (6 if rgm is not None else 0), (6 if cgm is not None else 0)
    costs = (1.0, 2.0, 0.25)
    res = run_trials(scores, rows, cols, tgt, rgm, cgm, g0, g1, joint, n_boot=14, seed=21, costs=costs)
    check(res, br.Sorted.trials(scores, rows, cols, tgt, rgm, cgm, g0, g1), 14, 21, joint, costs)
    assert res.mode == mode


@pytest.mark.parametrize("joint", [True, False])
def test_all_pairs(joint):
    """Every cell a trial, the labels the groups; a view with a row stride; the diagonal skipped when the set meets itself."""
    from xvector_amd import bootstrap
    rng = np.random.default_rng(31)
    n_rows, n_cols = (71, 71) if joint else (53, 90)
    row_lab = rng.integers(0, 9, n_rows)
    col_lab = row_lab if joint else rng.integers(0, 9, n_cols)
    scores = rng.normal(0, 1, (n_rows, n_cols)) + 2.0 * (row_lab[:, None] == col_lab[None, :])
    buf = torch.full((n_rows, n_cols + 3), float("nan"), dtype=torch.float64, device=DEV)
    buf[:, :n_cols] = torch.from_numpy(scores).to(DEV)
    res = bootstrap.bootstrap_all_pairs(buf[:, :n_cols], row_lab, None if joint else col_lab, skip_diagonal=joint, n_boot=10, seed=4)
    ids = np.unique(np.r_[row_lab, col_lab], return_inverse=True)[1]
    rid, cid = ids[:n_rows], ids[n_rows:]
    g = int(ids.max()) + 1
    srt = br.Sorted.all_pairs(scores, rid, cid, joint, rid, cid, g, g)
    check(res, srt, 10, 4, joint)
    assert res.mode == ("joint" if joint else "independent") and res.n_row_groups == res.n_col_groups == g
    assert srt.t.size == n_rows * n_cols - (n_rows if joint else 0) and n_rows * n_cols > TILE


# ---------------------------------------------------------------- bad inputs

def test_bad_inputs_are_counted_and_left_out_and_the_workspace_may_hold_anything():
    from xvector_amd import bootstrap, hip
    n = TILE + 1
    scores, rows, cols, tgt, rg, cg = matrix_case(41, n)
    scores[rows[5], cols[5]] = scores[rows[4000], cols[4000]] = np.nan
    rows[17], cols[4096], rows[300] = -1, 83, 61                       # outside the [61, 83] matrix
    rg[rows[40]], cg[cols[4090]] = 7, -1                               # outside [0, 7) and [0, 5)
    srt = br.Sorted.trials(scores, rows, cols, tgt, rg, cg, 7, 5)
    assert srt.n_bad_index == 3 and srt.n_nan >= 2 and srt.n_bad_group >= 2
    res = run_trials(scores, rows, cols, tgt, rg, cg, 7, 5, n_boot=10, seed=2)
    check(res, srt, 10, 2)
    assert int(res.n_target[0]) + int(res.n_nontarget[0]) > 0
    # a poisoned workspace of exactly the reported size, inside a guarded buffer
    need = hip.lib.xvec_boot_workspace_bytes(n, 10, 7, 5)
    for fill in (0xFF, 0x5A):
        guard = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=DEV)
        ws = guard[256:256 + need]
        ws.fill_(fill)
        again = run_trials(scores, rows, cols, tgt, rg, cg, 7, 5, n_boot=10, seed=2, workspace=ws)
        assert torch.equal(again.records.view(torch.int64), res.records.view(torch.int64))
        assert (guard[:256] == 0xA5).all() and (guard[256 + need:] == 0xA5).all()
    # the public functions raise on what the counters say
    from xvector_amd import TrialList
    with pytest.raises(IndexError, match="3 trial"):
        bootstrap.bootstrap_trials(_dev(scores), TrialList(rows, cols, tgt), n_boot=2)


# ---------------------------------------------------------------- the point estimate and the library's own evaluation

def test_record_zero_is_the_library_s_point_estimate():
    from xvector_amd import TrialList, bootstrap, evaluate
    scores, rows, cols, tgt, rg, cg = matrix_case(51, 2 * TILE + 3, levels=16)
    s, trials = _dev(scores), TrialList(rows, cols, tgt)
    for p_target in (0.5, 0.05):
        want = evaluate.evaluate_trials(s, trials, c_fa=2.0, p_target=p_target)
        for kw in (dict(row_groups=rg, col_groups=cg), dict(row_groups=rg), dict()):
            assert bootstrap.bootstrap_trials(s, trials, n_boot=1, c_fa=2.0, p_target=p_target, **kw).point == want
    lab = np.random.default_rng(3).integers(0, 12, 80)
    sq = _dev(np.random.default_rng(4).normal(0, 1, (80, 80)) + 1.5 * (lab[:, None] == lab[None, :]))
    assert bootstrap.bootstrap_all_pairs(sq, lab, n_boot=1, p_target=0.05).point == evaluate.evaluate_all_pairs(sq, lab, p_target=0.05)
    assert bootstrap.bootstrap_all_pairs(sq, lab, lab[::-1].copy(), skip_diagonal=False, n_boot=1).point == \
        evaluate.evaluate_all_pairs(sq, lab, lab[::-1].copy(), skip_diagonal=False)


@pytest.mark.parametrize("mode", ["joint", "poisson"])
def test_replicates_equal_the_library_s_evaluation_of_the_expanded_list(mode):
    """Every replicate against evaluate_trials on the list in which trial t occurs w_b(t) times (repeat_interleave on the
    device): the same kernels' definitions, reached the long way round."""
    from xvector_amd import TrialList, bootstrap, evaluate
    scores, rows, cols, tgt, rg, cg = matrix_case(61, 700, g_rows=6, g_cols=6, levels=8)
    s, seed, n_boot, costs = _dev(scores), 13, 8, (1.0, 2.0, 0.25)
    if mode == "joint":
        res = run_trials(scores, rows, cols, tgt, rg, cg, 6, 6, True, n_boot, seed, costs)
        srt = br.Sorted.trials(scores, rows, cols, tgt, rg, cg, 6, 6)
    else:
        res = run_trials(scores, rows, cols, tgt, n_boot=n_boot, seed=seed, costs=costs)      # a list without groups
        srt = br.Sorted.trials(scores, rows, cols, tgt)
    got_d, got_c = _got(res)
    evaluated = 0
    for b in range(1, n_boot + 1):
        w = np.zeros(len(tgt), dtype=np.int64)
        w[srt.t] = srt.weights(seed, b, mode == "joint")
        rep = lambda a, dtype: torch.repeat_interleave(_dev(a, dtype), _dev(w)).cpu().numpy()
        if w[tgt == 1].sum() == 0 or w[tgt == 0].sum() == 0:
            assert np.isnan(got_d[b]).all()
            continue
        want = evaluate.evaluate_trials(s, TrialList(rep(rows, np.int32), rep(cols, np.int32), rep(tgt, np.uint8)), *costs)
        assert tuple(got_d[b]) == (want.eer, want.eer_th, want.far, want.frr, want.min_dcf, want.min_dcf_th), b
        assert tuple(got_c[b]) == (want.n_target, want.n_nontarget), b
        evaluated += 1
    assert evaluated >= 6


# ---------------------------------------------------------------- determinism: n_boot, batching, pairing

def test_replicates_do_not_depend_on_n_boot_or_on_the_batching():
    """Replicates 1 .. 5 of n_boot = 5 (one batch of 8) are those of n_boot = 50 (one batch of 56) and of n_boot = 300, which
    spans the boundary between two batches of 256; around that boundary the records are the restatement's; two calls are
    bit-identical."""
    from xvector_amd import hip
    scores, rows, cols, tgt, rg, cg = matrix_case(71, TILE + 1)
    n = len(tgt)
    assert [hip.lib.xvec_boot_batch(n, k) for k in (5, 50, 300)] == [8, 56, 256]
    assert [hip.lib.xvec_boot_batches(n, k) for k in (5, 50, 300)] == [1, 1, 2]
    run = lambda n_boot: run_trials(scores, rows, cols, tgt, rg, cg, 7, 5, False, n_boot, 99)
    a, b, c = run(5), run(50), run(300)
    bits = lambda r: r.records.view(torch.int64)
    assert torch.equal(bits(a), bits(b)[:6]) and torch.equal(bits(b), bits(c)[:51])
    assert torch.equal(bits(run(300)), bits(c))
    check(c, br.Sorted.trials(scores, rows, cols, tgt, rg, cg, 7, 5), 300, 99, replicates=[0, 1, 5, 254, 255, 256, 257, 300])
    # the Poisson mode likewise
    vec = scores[rows, cols]
    p = lambda n_boot: run_trials(vec, None, None, tgt, n_boot=n_boot, seed=99)
    a, c = p(5), p(300)
    assert torch.equal(bits(a), bits(c)[:6])
    check(c, br.Sorted.trials(vec, None, None, tgt), 300, 99, replicates=[0, 1, 255, 256, 300])


def test_two_systems_under_one_seed_see_the_same_resamples():
    from xvector_amd import TrialList, bootstrap
    scores, rows, cols, tgt, rg, cg = matrix_case(81, 3000)
    other = scores + np.random.default_rng(5).normal(0, 0.5, scores.shape)
    trials = TrialList(rows, cols, tgt)
    kw = dict(row_groups=rg, col_groups=cg, n_boot=40, seed=17)
    a, b = bootstrap.bootstrap_trials(_dev(scores), trials, **kw), bootstrap.bootstrap_trials(_dev(other), trials, **kw)
    assert torch.equal(a.n_target, b.n_target) and torch.equal(a.n_nontarget, b.n_nontarget)
    assert not torch.equal(a.eer, b.eer) and len(set(a.n_target.tolist())) > 10
    c = bootstrap.compare(a, b, "eer")
    assert c.n_valid == 40 and c.lo <= c.hi and 0.0 <= c.share_a_lower <= 1.0
    assert abs(c.difference - (a.point.eer - b.point.eer)) == 0.0
    lo, hi = a.interval("eer")
    assert lo <= hi and a.stderr("eer") > 0.0
    with pytest.raises(ValueError, match="differ in seed"):
        bootstrap.compare(a, bootstrap.bootstrap_trials(_dev(other), trials, **dict(kw, seed=18)))


# ---------------------------------------------------------------- xvec_eval_sorted_order

@pytest.mark.parametrize("n", [TILE + 1, 2 * TILE + 3])
def test_sorted_order_is_a_stable_argsort_of_the_keys(n):
    from xvector_amd import evaluate as ev
    rng = np.random.default_rng(n)
    x = np.round(rng.normal(0, 1, n) * 4) / 4                     # many equal keys
    x[rng.integers(0, n, 30)] = np.nan                            # left out: key 0xffffffff, last, in index order
    x[:5] = [-0.0, 0.0, np.inf, -np.inf, 1e39]
    keys = host_keys(np.where(np.isnan(x), 0.0, x))
    keys[np.isnan(x)] = 0xFFFFFFFF
    order = np.argsort(keys, kind="stable")
    got_keys, got_order = ev.sorted_order(_dev(x), np.ones(n, dtype=np.uint8))
    assert np.array_equal(got_order.cpu().numpy(), order) and np.array_equal(got_keys.cpu().numpy(), keys[order])
    # the byte payload's sort of the same scores ends in the same keys
    assert torch.equal(ev.sorted_keys(_dev(x), np.ones(n, dtype=np.uint8))[0], got_keys)


def test_sorted_order_of_all_pairs_counts_cells_row_by_row():
    from xvector_amd import hip
    rng = np.random.default_rng(8)
    n_rows, n_cols = 70, 61
    scores = np.round(rng.normal(0, 1, (n_rows, n_cols)) * 2) / 2
    lab_r, lab_c = rng.integers(0, 5, n_rows).astype(np.int32), rng.integers(0, 5, n_cols).astype(np.int32)
    n = n_rows * n_cols
    s, r, c = _dev(scores), _dev(lab_r), _dev(lab_c)
    keys = torch.empty(n, dtype=torch.int32, device=DEV)
    order = torch.empty(n, dtype=torch.int32, device=DEV)
    ws = torch.empty(hip.lib.xvec_eval_sorted_order_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    rc = hip.lib.xvec_eval_sorted_order_all_pairs(s.data_ptr(), n_cols, n_rows, n_cols, r.data_ptr(), c.data_ptr(), 1, keys.data_ptr(),
                                                  order.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == 0, hip.lib.xvec_eval_last_error().decode()
    torch.cuda.synchronize()
    want = host_keys(scores.reshape(-1))
    want[np.arange(min(n_rows, n_cols)) * (n_cols + 1)] = 0xFFFFFFFF          # the diagonal cells t = i * n_cols + i
    perm = np.argsort(want, kind="stable")
    assert np.array_equal(order.cpu().numpy().astype(np.int64), perm)
    assert np.array_equal(keys.cpu().numpy().view(np.uint32).astype(np.int64), want[perm])
