"""Trial evaluation on the GPU (csrc/eval.hip through xvector_amd.evaluate) against the oracles of tests/eer_ref.py.

Bars as tests/test_evaluate.py derives them: values within 2^-22 of the literal float32 walk (`naive`) and within 1e-12 of the
same arithmetic in float64 (`by_sort`); thresholds equal to the oracle's or -- at most 2 % of a test's cases -- a threshold
at which the oracle's own objective is within 2^-22 of its minimum.  The sort is compared bit for bit with a stable sort of
the same keys."""
import numpy as np
import pytest
import torch

import eer_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VAL_BAR = 2.0 ** -22
SORT_BAR = 1e-12


def host_keys(scores):
    """The order-preserving 32-bit key of include/xvec_eval.h, on the host (int64 holding the unsigned value)."""
    with np.errstate(over="ignore"):                      # beyond the float32 range: infinity, as on the device
        f = np.asarray(scores, dtype=np.float64).astype(np.float32) + np.float32(0.0)       # -0.0 + 0.0 = +0.0
    u = f.view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


class Tally:
    """Counts the threshold comparisons of one test that took the second branch of the bar."""

    def __init__(self):
        self.total = self.second = 0

    def check(self, res, ref, pos, neg, objectives_at, bar, p_target=0.5, what=""):
        for name, got in (("eer", res.eer), ("far", res.far), ("frr", res.frr), ("min_dcf", res.min_dcf)):
            print(f"{what} {name}: got {got!r} oracle {getattr(ref, name)!r}")
            assert abs(got - getattr(ref, name)) <= bar, (what, name, got, getattr(ref, name))
        for which, (got, want, best) in enumerate(((res.eer_th, ref.eer_th, ref.eer_gap),
                                                   (res.min_dcf_th, ref.min_dcf_th, ref.min_dcf))):
            self.total += 1
            if got != want:
                self.second += 1
                at = objectives_at(pos, neg, got, p_target=p_target)[which]
                print(f"{what} threshold {which}: got {got!r} oracle {want!r}; oracle's objective there {at!r}, minimum {best!r}")
                assert at <= best + VAL_BAR, (what, which, got, want, at, best)

    def done(self):
        assert self.second <= 0.02 * self.total, f"{self.second} of {self.total} thresholds differ from the oracle's"


def scattered(pos, neg, seed, n_rows=300, n_cols=411, pad=5):
    """A score matrix (a view with ld = n_cols + pad) holding the given scores in distinct random cells, NaN everywhere else,
    and the TrialList that selects them in a shuffled order."""
    from xvector_amd.evaluate import TrialList
    rng = np.random.default_rng(seed)
    n = pos.size + neg.size
    while n_rows * n_cols < n:
        n_rows *= 2
    cells = rng.permutation(n_rows * n_cols)[:n]
    host = np.full((n_rows, n_cols + pad), np.nan)
    vals = np.r_[pos, neg]
    tgt = np.r_[np.ones(pos.size, dtype=np.uint8), np.zeros(neg.size, dtype=np.uint8)]
    order = rng.permutation(n)
    cells, vals, tgt = cells[order], vals[order], tgt[order]
    host[cells // n_cols, cells % n_cols] = vals
    mat = torch.from_numpy(host).to(DEV)[:, :n_cols]
    return mat, TrialList(cells // n_cols, cells % n_cols, tgt)


# ------------------------------------------------------------------ the sort

# (1024: a wave's share of a tile in the scatter; 4096: a tile; 65536 = 16 tiles: the digit table of 256 x tiles entries fills
#  one scan chunk exactly, 17 tiles spill into a second)
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 37720, 65535, 65536,
                               65537, 69633, 2 ** 20 + 3])
@pytest.mark.parametrize("ties", [False, True])
def test_sorted_pairs_equal_a_stable_sort_bit_for_bit(n, ties):
    from xvector_amd import evaluate as ev
    rng = np.random.default_rng(n + ties)
    x = rng.normal(0, 3, n)
    if ties:
        x = np.clip(np.round(x), -8, 7)                       # 16 levels
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 3.4e38, -3.4e38, 1e39, -1e39, 1e-50])
    idx = rng.permutation(n)[: min(n, 4 * special.size)]
    x[idx] = np.resize(special, idx.size)
    bits = rng.integers(0, 2, n).astype(np.uint8)
    keys = torch.from_numpy(host_keys(x))
    want_keys, perm = torch.sort(keys, stable=True)
    want_bits = torch.from_numpy(bits)[perm]
    got_keys, got_bits = ev.sorted_keys(torch.from_numpy(x).to(DEV), bits)
    assert torch.equal(got_keys.cpu(), want_keys)
    assert torch.equal(got_bits.cpu(), want_bits)
    again_keys, again_bits = ev.sorted_keys(torch.from_numpy(x).to(DEV), bits)
    assert torch.equal(again_keys, got_keys) and torch.equal(again_bits, got_bits)


# ------------------------------------------------------------------ evaluate_trials

@pytest.mark.parametrize("n_pos,n_neg,levels", [(50, 80, None), (50, 80, 16), (2000, 5000, None), (2000, 5000, 16),
                                               (1, 1, None), (7, 4090, None), (4096, 4096, 16)])
def test_evaluate_trials_against_the_walk(n_pos, n_neg, levels):
    from xvector_amd import evaluate as ev
    tally = Tally()
    for seed in range(3):
        pos, neg = eer_ref.draw(np.random.default_rng(7 * n_pos + seed), n_pos, n_neg, levels)
        mat, trials = scattered(pos, neg, seed)
        for p_target in (0.5, 0.05, 0.01):
            res = ev.evaluate_trials(mat, trials, p_target=p_target)
            assert (res.n_target, res.n_nontarget) == (n_pos, n_neg)
            what = f"[{n_pos}+{n_neg} levels={levels} seed={seed} p={p_target}]"
            tally.check(res, eer_ref.naive(pos, neg, p_target=p_target), pos, neg, eer_ref.naive_objectives_at, VAL_BAR,
                        p_target, what + " walk")
            tally.check(res, eer_ref.by_sort(pos, neg, p_target=p_target), pos, neg, eer_ref.by_sort_objectives_at, SORT_BAR,
                        p_target, what + " sort")
    tally.done()


def test_evaluate_trials_at_the_trial_list_size_against_the_walk():
    """37 720 trials, 3000 of them targets: the size of the reference's trial file."""
    from xvector_amd import evaluate as ev
    tally = Tally()
    pos, neg = eer_ref.draw(np.random.default_rng(37720), 3000, 34720)
    mat, trials = scattered(pos, neg, 1, n_rows=487, n_cols=487)
    res = ev.evaluate_trials(mat, trials, p_target=0.5)
    tally.check(res, eer_ref.naive(pos, neg, p_target=0.5), pos, neg, eer_ref.naive_objectives_at, VAL_BAR, 0.5, "[37720] walk")
    for p_target in (0.5, 0.05, 0.01):
        res = ev.evaluate_trials(mat, trials, p_target=p_target)
        tally.check(res, eer_ref.by_sort(pos, neg, p_target=p_target), pos, neg, eer_ref.by_sort_objectives_at, SORT_BAR,
                    p_target, f"[37720 p={p_target}] sort")
    tally.done()


@pytest.mark.parametrize("levels", [None, 16])
def test_evaluate_trials_above_the_walk_s_reach(levels):
    from xvector_amd import evaluate as ev
    tally = Tally()
    pos, neg = eer_ref.draw(np.random.default_rng(5), 200_000, 800_003, levels)
    mat, trials = scattered(pos, neg, 2, n_rows=1100, n_cols=1000)
    for p_target in (0.5, 0.05, 0.01):
        res = ev.evaluate_trials(mat, trials, c_miss=1.0, c_fa=2.0, p_target=p_target)
        tally.check(res, eer_ref.by_sort(pos, neg, c_fa=2.0, p_target=p_target), pos, neg,
                    lambda p, n, th, p_target: eer_ref.by_sort_objectives_at(p, n, th, c_fa=2.0, p_target=p_target), SORT_BAR,
                    p_target, f"[1M levels={levels} p={p_target}] sort")
    tally.done()


def test_separable_and_all_equal_scores():
    from xvector_amd import evaluate as ev
    rng = np.random.default_rng(3)
    pos, neg = rng.uniform(0.5, 2.0, 700).astype(np.float32).astype(np.float64), rng.uniform(-2.0, 0.25, 900).astype(np.float32).astype(np.float64)
    mat, trials = scattered(pos, neg, 4)
    res = ev.evaluate_trials(mat, trials)
    assert res.eer == 0.0 and res.far == 0.0 and res.frr == 0.0 and res.min_dcf == 0.0
    assert res.eer_th == neg.max() and res.min_dcf_th == neg.max()
    ref = eer_ref.naive(pos, neg)
    assert ref.eer == 0.0 and ref.eer_th == res.eer_th and ref.min_dcf_th == res.min_dcf_th
    same = np.full(300, 0.75)
    mat, trials = scattered(same[:100], same[100:], 5)
    res = ev.evaluate_trials(mat, trials, p_target=0.05)
    ref = eer_ref.naive(same[:100], same[100:], p_target=0.05)
    assert (res.eer, res.far, res.frr, res.eer_th) == (0.5, 0.0, 1.0, 0.75) == (ref.eer, ref.far, ref.frr, ref.eer_th)
    assert abs(res.min_dcf - ref.min_dcf) <= VAL_BAR and res.min_dcf_th == 0.75


def test_drop_ins_on_the_fixture_scores():
    """EER / minDCF with speechbrain's signature and defaults, on the scores the reference itself collected (g8)."""
    from xvector_amd import evaluate as ev
    g = load_golden("g8_trials.npz")
    pos, neg = g["positive_scores"], g["negative_scores"]
    tally = Tally()
    eer, eer_th = ev.EER(torch.tensor(pos.tolist()), torch.tensor(neg.tolist()))          # as plda_score_stat.py:96-97
    dcf5, dcf5_th = ev.minDCF(torch.tensor(pos.tolist()), torch.tensor(neg.tolist()), p_target=0.5)
    dcf1, dcf1_th = ev.minDCF(pos.tolist(), neg)                                            # lists / arrays, default p_target = 0.01
    assert all(isinstance(v, float) for v in (eer, eer_th, dcf5, dcf5_th, dcf1, dcf1_th))
    for oracle, at, bar in ((eer_ref.naive, eer_ref.naive_objectives_at, VAL_BAR),
                            (eer_ref.by_sort, eer_ref.by_sort_objectives_at, SORT_BAR)):
        r5, r1 = oracle(pos, neg, p_target=0.5), oracle(pos, neg, p_target=0.01)
        assert abs(eer - r5.eer) <= bar and abs(dcf5 - r5.min_dcf) <= bar and abs(dcf1 - r1.min_dcf) <= bar
        assert eer_th == r5.eer_th and dcf5_th == r5.min_dcf_th and dcf1_th == r1.min_dcf_th
    with pytest.raises(ValueError):
        ev.EER([], [1.0])


# ------------------------------------------------------------------ evaluate_all_pairs

def test_all_pairs_at_the_test_set_size():
    """4874 x 4874 (23.7 M cells, 40 speakers) against the sort formulation on the same cells taken on the host.  The diagonal
    holds NaN: the call passes only if those cells are really skipped."""
    from xvector_amd import evaluate as ev
    n = 4874
    gen = torch.Generator(device="cpu").manual_seed(11)
    labels = np.arange(n) % 40
    same = torch.from_numpy(labels[:, None] == labels[None, :])
    mat = torch.randn(n, n, generator=gen, dtype=torch.float64) * 1.5 - 1.5 + 2.5 * same
    mat.fill_diagonal_(float("nan"))
    host = mat.numpy()
    off = ~np.eye(n, dtype=bool)
    pos, neg = host[same.numpy() & off], host[~same.numpy()]
    dmat = mat.to(DEV)
    tally = Tally()
    res = ev.evaluate_all_pairs(dmat, labels, p_target=0.05)
    assert (res.n_target, res.n_nontarget) == (pos.size, neg.size) and pos.size + neg.size == n * n - n
    tally.check(res, eer_ref.by_sort(pos, neg, p_target=0.05), pos, neg, eer_ref.by_sort_objectives_at, SORT_BAR, 0.05,
                "[all pairs 4874]")
    tally.done()
    assert ev.evaluate_all_pairs(dmat, labels, p_target=0.05) == res                  # bit-identical from run to run
    with pytest.raises(ValueError, match="NaN"):
        ev.evaluate_all_pairs(dmat, labels, skip_diagonal=False)


def test_all_pairs_of_two_sets_keeps_the_diagonal_when_asked():
    from xvector_amd import evaluate as ev
    rng = np.random.default_rng(8)
    rows, cols = np.array([f"spk{v}" for v in rng.integers(0, 9, 301)]), np.array([f"spk{v}" for v in rng.integers(0, 9, 207)])
    same = rows[:, None] == cols[None, :]
    host = (rng.normal(-1.5, 1.5, same.shape) + 2.5 * same).astype(np.float32).astype(np.float64)
    dmat = torch.from_numpy(host).to(DEV)
    tally = Tally()
    res = ev.evaluate_all_pairs(dmat, rows, cols, skip_diagonal=False)
    tally.check(res, eer_ref.by_sort(host[same], host[~same]), host[same], host[~same], eer_ref.by_sort_objectives_at, SORT_BAR,
                0.5, "[two sets]")
    off = ~np.eye(*same.shape, dtype=bool)
    res = ev.evaluate_all_pairs(dmat, rows, cols, skip_diagonal=True)
    assert res.n_target + res.n_nontarget == same.size - 207
    tally.check(res, eer_ref.by_sort(host[same & off], host[~same & off]), host[same & off], host[~same & off],
                eer_ref.by_sort_objectives_at, SORT_BAR, 0.5, "[two sets, diagonal skipped]")
    tally.done()


# ------------------------------------------------------------------ the reference's class

class _Plda:
    pass


def test_plda_score_stat_object_reproduces_the_reference(tmp_path):
    import pandas as pd
    from xvector_amd.evaluate import plda_score_stat_object
    g = load_golden("g8_trials.npz")
    path = str(tmp_path / "veri_test.txt")
    with open(path, "w") as f:
        f.write(str(g["trial_text"]))
    frame = pd.DataFrame({"index": np.arange(len(g["ids"])), "id": g["ids"].tolist(), "label": g["labels"],
                          "xvector": [str(v) for v in g["vectors"]]})
    plda = _Plda()
    plda.mean, plda.F, plda.Sigma = g["mean"], g["F"], g["Sigma"]
    obj = plda_score_stat_object(frame)
    assert obj.plda_scores == 0 and obj.eer == 0 and obj.positive_scores == []
    assert np.array_equal(obj.x_vec_test, g["read_vectors"])
    obj.test_plda(plda, path)
    assert isinstance(obj.positive_scores, list) and isinstance(obj.positive_scores[0], float)
    for got, want in ((obj.positive_scores, g["positive_scores"]), (obj.negative_scores, g["negative_scores"])):
        got = np.asarray(got)
        assert got.shape == want.shape
        rel = np.abs(got - want).max() / np.abs(want).max()
        print("trial scores: max-norm relative error", rel)
        assert rel < 1e-9
    assert np.array_equal(obj.positive_scores_mask, g["positive_scores_mask"])
    assert np.array_equal(obj.negative_scores_mask, g["negative_scores_mask"])
    assert obj.positive_scores_mask.dtype == g["positive_scores_mask"].dtype
    assert np.array_equal(obj.checked_label, g["checked_label"]) and np.array_equal(obj.checked_xvec, g["checked_xvec"])
    obj.calc_eer_mindcf()
    pos, neg = g["positive_scores"], g["negative_scores"]
    walk, sort = eer_ref.naive(pos, neg, p_target=0.5), eer_ref.by_sort(pos, neg, p_target=0.5)
    assert abs(obj.eer - walk.eer) <= VAL_BAR and abs(obj.min_dcf - walk.min_dcf) <= VAL_BAR
    assert abs(obj.eer - sort.eer) <= SORT_BAR and abs(obj.min_dcf - sort.min_dcf) <= SORT_BAR
    assert obj.eer_th == sort.eer_th and obj.min_dcf_th == sort.min_dcf_th
    sc = obj.plda_scores                                   # the host Scores object, built on first access
    assert sc.scoremat.shape == (60, 60) and list(sc.modelset) == g["ids"].tolist() and obj.plda_scores is sc
    with pytest.raises(NotImplementedError):
        obj.plot_images(None)


# ------------------------------------------------------------------ refusals, determinism, streams, workspace

def test_nan_and_bad_indices_raise_only_when_selected():
    from xvector_amd import evaluate as ev
    pos, neg = eer_ref.draw(np.random.default_rng(2), 40, 60)
    mat, trials = scattered(pos, neg, 6)                   # every cell no trial selects is NaN
    ok = ev.evaluate_trials(mat, trials)
    bad = mat.clone()
    bad[int(trials.row_idx[17]), int(trials.col_idx[17])] = float("nan")
    with pytest.raises(ValueError, match="1 trial score"):
        ev.evaluate_trials(bad, trials)
    for r, c in ((mat.shape[0], 0), (0, mat.shape[1]), (-1, 0), (0, -1), (2 ** 31 - 1, 2 ** 31 - 1)):
        rows, cols = trials.row_idx.copy(), trials.col_idx.copy()
        rows[3], cols[3] = r, c
        with pytest.raises(IndexError, match="1 trial"):
            ev.evaluate_trials(mat, ev.TrialList(rows, cols, trials.is_target))
    for flag in (0, 1):
        with pytest.raises(ValueError, match="both kinds"):
            ev.evaluate_trials(mat, ev.TrialList(trials.row_idx, trials.col_idx, np.full(len(trials), flag)))
    assert ev.evaluate_trials(mat, trials) == ok


def test_repeatable_on_any_stream_with_a_poisoned_workspace():
    from xvector_amd import evaluate as ev, hip
    pos, neg = eer_ref.draw(np.random.default_rng(9), 3000, 34720, 16)
    mat, trials = scattered(pos, neg, 7)
    first = ev.evaluate_trials(mat, trials, p_target=0.05)
    assert ev.evaluate_trials(mat, trials, p_target=0.05) == first
    ws = torch.full((int(hip.lib.xvec_eval_workspace_bytes(len(trials))),), 0xFF, dtype=torch.uint8, device=DEV)
    assert ev.evaluate_trials(mat, trials, p_target=0.05, workspace=ws) == first
    ws.fill_(0xFF)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        assert ev.evaluate_trials(mat, trials, p_target=0.05, workspace=ws) == first
    stream.synchronize()
    assert ev.evaluate_trials(mat, trials, p_target=0.05) == first
