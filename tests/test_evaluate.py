"""Trial evaluation, the parts that need no GPU: the two oracles of tests/eer_ref.py against each other and against sklearn,
the trial-file parser against the reference's own run (tests/golden/g8_trials.npz, made by make_golden_trials.py), the C
ABI's argument errors, and the refusal to run on the CPU.

Bars (derived, not measured).  Values against the literal float32 walk (`naive`): 2^-22 absolute -- every quantity is at most
1 and the walk makes at most four float32 roundings of 2^-24 relative each on the way to it.  Against `by_sort` (the same
arithmetic in float64): 1e-12.  Thresholds: the oracle's, or -- the walk's float32 rounding may break a near-tie the other
way -- a threshold at which the oracle's own objective is within 2^-22 of its minimum; at most 2 % of a test's cases may
take that second branch."""
import os

import numpy as np
import pytest
import torch

import eer_ref
import plda_oracle as po
from conftest import load_golden

VAL_BAR = 2.0 ** -22
CASES = [(seed, levels) for seed in range(20) for levels in (None, 16)]


def _case(seed, levels):
    rng = np.random.default_rng(1000 + seed)
    return eer_ref.draw(rng, int(rng.integers(5, 201)), int(rng.integers(5, 401)), levels)


def test_walk_and_sort_formulations_agree():
    second_branch = 0
    total = 0
    for seed, levels in CASES:
        pos, neg = _case(seed, levels)
        for p_target in (0.5, 0.05, 0.01):
            a = eer_ref.naive(pos, neg, p_target=p_target)
            b = eer_ref.by_sort(pos, neg, p_target=p_target)
            for name in ("eer", "far", "frr", "min_dcf"):
                assert abs(getattr(a, name) - getattr(b, name)) <= VAL_BAR, (seed, levels, p_target, name, a, b)
            for name, which in (("eer_th", 0), ("min_dcf_th", 1)):
                total += 1
                if getattr(a, name) != getattr(b, name):
                    second_branch += 1
                    at = eer_ref.naive_objectives_at(pos, neg, getattr(b, name), p_target=p_target)[which]
                    best = (a.eer_gap, a.min_dcf)[which]
                    assert at <= best + VAL_BAR, (seed, levels, p_target, name, a, b)
    assert second_branch <= 0.02 * total, f"{second_branch} of {total} thresholds differ from the walk's"


def test_sort_formulation_against_sklearn_roc_curve():
    from sklearn.metrics import roc_curve
    for seed, levels in CASES[:12]:
        pos, neg = _case(seed, levels)
        u, tp, fa = eer_ref.curves(pos, neg)
        y = np.r_[np.ones(pos.size), np.zeros(neg.size)]
        fpr, tpr, thr = roc_curve(y, np.r_[pos, neg].astype(np.float32), drop_intermediate=False)
        K = u.size
        assert fpr.size == K + 1 and np.array_equal(thr[1:][::-1].astype(np.float32), u)
        # sklearn decides score >= thr: the rates "above u_k" are its rates at the next distinct score (thr = inf for the last)
        np.testing.assert_allclose(fa / neg.size, fpr[:K][::-1], rtol=0, atol=1e-12)
        np.testing.assert_allclose(tp / pos.size, 1.0 - tpr[:K][::-1], rtol=0, atol=1e-12)


def test_signed_zeros_and_infinities_in_the_oracle():
    r = eer_ref.by_sort([0.0, np.inf, 1.0], [-0.0, -np.inf, 0.5])
    u, tp, fa = eer_ref.curves([0.0, np.inf, 1.0], [-0.0, -np.inf, 0.5])
    assert u.tolist() == [-np.inf, 0.0, 0.5, 1.0, np.inf] and tp.tolist() == [0, 1, 1, 2, 3] and fa.tolist() == [2, 1, 0, 0, 0]
    assert r.eer == pytest.approx(1.0 / 3.0) and r.eer_th == 0.0


# ------------------------------------------------------------------ the trial file

def _g8_trials(tmp_path):
    g = load_golden("g8_trials.npz")
    path = str(tmp_path / "veri_test.txt")
    with open(path, "w") as f:
        f.write(str(g["trial_text"]))
    return g, path


def test_trial_file_parsing_matches_the_reference(tmp_path):
    from xvector_amd.evaluate import TrialList
    g, path = _g8_trials(tmp_path)
    ids = g["ids"].tolist()
    tl = TrialList.from_file(path, np.array(ids, dtype=object), np.array(ids, dtype=object))
    assert tl.row_idx.dtype == np.int32 and tl.col_idx.dtype == np.int32 and tl.is_target.dtype == np.uint8
    n_pos, n_neg = g["positive_scores"].size, g["negative_scores"].size
    assert len(tl) == n_pos + n_neg and int(tl.is_target.sum()) == n_pos
    match = tl.is_target.astype(bool)
    for m, want in ((match, g["positive_scores_mask"]), (~match, g["negative_scores_mask"])):
        mask = np.zeros_like(want)
        mask[tl.row_idx[m], tl.col_idx[m]] = 1
        assert np.array_equal(mask, want)
    # the scores the reference picked, in its order: the oracle's matrix read at the parsed positions
    mat = po.fast_plda_scoring(g["read_vectors"], g["read_vectors"], g["mean"], g["F"], g["Sigma"])
    picked = mat[tl.row_idx, tl.col_idx]
    np.testing.assert_allclose(picked[match], g["positive_scores"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(picked[~match], g["negative_scores"], rtol=1e-12, atol=1e-12)
    # both spellings of the label occur in the file
    firsts = {line.split(" ")[0] for line in str(g["trial_text"]).splitlines()}
    assert firsts == {"0", "1", "0.0", "1.0"}


def test_duplicate_id_resolves_to_its_first_position_and_missing_id_raises(tmp_path):
    from xvector_amd.evaluate import TrialList
    g = load_golden("g8_trials.npz")
    ids = g["ids"].tolist()
    assert ids[41] == ids[7] and ids.count(ids[7]) == 2
    path = str(tmp_path / "t.txt")
    with open(path, "w") as f:
        f.write(f"1 {ids[7]} {ids[3]}\n0.0 {ids[5]} {ids[41]} \n\n")
    tl = TrialList.from_file(path, ids, ids)
    assert tl.row_idx.tolist() == [7, 5] and tl.col_idx.tolist() == [3, 7] and tl.is_target.tolist() == [1, 0]
    assert int(np.where(np.array(ids, dtype=object) == ids[41])[0][0]) == 7          # the reference's lookup
    with open(path, "w") as f:
        f.write(f"1 {ids[2]} id99999/nope/00001.wav\n")
    with pytest.raises(KeyError, match="id99999/nope/00001.wav"):
        TrialList.from_file(path, ids, ids)
    with pytest.raises(ValueError):
        TrialList([0, 1], [0], [1, 0])


# ------------------------------------------------------------------ the boundary

def test_eval_abi_argument_errors_without_gpu():
    """Error paths that never touch the device.  Return codes as every other entry point of the library: XVEC_ERR_ARG for
    null pointers and counts, XVEC_ERR_WORKSPACE for a workspace below the queried size."""
    from xvector_amd import hip
    L = hip.lib
    err = lambda: L.xvec_eval_last_error().decode()
    one = 0x1000          # stands for a non-null device pointer: no call below gets as far as reading it
    assert L.xvec_eval_workspace_bytes(0) == 0 and L.xvec_eval_workspace_bytes(-5) == 0
    assert L.xvec_eval_workspace_bytes(2 ** 31) == 0
    need = L.xvec_eval_workspace_bytes(1000)
    assert need > 0 and L.xvec_eval_workspace_bytes(2 ** 31 - 1) > 2 ** 34
    assert L.xvec_eval_trials(None, 8, 8, 8, one, one, one, 10, 1.0, 1.0, 0.5, one, one, need, None) == hip.ERR_ARG
    assert "null" in err()
    assert L.xvec_eval_trials(one, 8, 8, 8, one, one, None, 10, 1.0, 1.0, 0.5, one, one, need, None) == hip.ERR_ARG
    assert "null" in err()
    assert L.xvec_eval_trials(one, 8, 8, 8, one, one, one, 10, 1.0, 1.0, 0.5, None, one, need, None) == hip.ERR_ARG
    assert "null" in err()
    for n in (0, -3):
        assert L.xvec_eval_trials(one, 8, 8, 8, one, one, one, n, 1.0, 1.0, 0.5, one, one, need, None) == hip.ERR_ARG
        assert "n_trials" in err()
    assert L.xvec_eval_trials(one, 8, 8, 8, one, one, one, 2 ** 31, 1.0, 1.0, 0.5, one, one, need, None) == hip.ERR_TOO_LARGE
    assert L.xvec_eval_trials(one, 8, 8, 8, one, one, one, 1000, 1.0, 1.0, 0.5, one, one, need - 1, None) == hip.ERR_WORKSPACE
    assert "workspace too small" in err()
    assert L.xvec_eval_trials(one, 4, 8, 8, one, one, one, 10, 1.0, 1.0, 0.5, one, one, need, None) == hip.ERR_ARG      # ld < n_cols
    assert L.xvec_eval_trials(one, 8, 8, 8, one, None, one, 10, 1.0, 1.0, 0.5, one, one, need, None) == hip.ERR_ARG     # one index array
    assert L.xvec_eval_trials(one, 8, 1, 8, None, None, one, 10, 1.0, 1.0, 0.5, one, one, need, None) == hip.ERR_ARG    # vector too short
    assert L.xvec_eval_trials(one, 8, 8, 8, one, one, one, 10, 1.0, 1.0, 1.5, one, one, need, None) == hip.ERR_ARG
    assert "p_target" in err()
    assert L.xvec_eval_all_pairs(one, 8, 8, 8, None, one, 1, 1.0, 1.0, 0.5, one, one, need, None) == hip.ERR_ARG
    assert L.xvec_eval_all_pairs(one, 8, 8, 8, one, one, 1, 1.0, 1.0, 0.5, one, one, 0, None) == hip.ERR_WORKSPACE
    assert L.xvec_eval_all_pairs(one, 2 ** 20, 2 ** 20, 2 ** 20, one, one, 1, 1.0, 1.0, 0.5, one, one, need, None) == hip.ERR_TOO_LARGE
    assert L.xvec_eval_sorted_keys(one, 8, 8, 8, one, one, one, 10, None, one, one, need, None) == hip.ERR_ARG
    assert L.xvec_eval_sorted_keys(one, 8, 8, 8, one, one, one, 0, one, one, one, need, None) == hip.ERR_ARG


def test_evaluation_refuses_cpu():
    from xvector_amd import evaluate as ev
    import xvector_amd as xa
    assert xa.evaluate_trials is ev.evaluate_trials and xa.plda_score_stat_object is ev.plda_score_stat_object
    tl = ev.TrialList([0, 1], [1, 0], [1, 0])
    with pytest.raises(RuntimeError, match="HIP device"):
        ev.evaluate_trials(torch.zeros(2, 2, dtype=torch.float64), tl)
    with pytest.raises(RuntimeError, match="HIP device"):
        ev.evaluate_all_pairs(torch.zeros(2, 2, dtype=torch.float64), [0, 1])
    with pytest.raises(RuntimeError, match="HIP device"):
        ev.EER([1.0, 2.0], [0.0], device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        ev.minDCF(torch.tensor([1.0]), torch.tensor([0.0]), device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        ev.sorted_keys(torch.zeros(4, dtype=torch.float64), [0, 1, 0, 1])
    import pandas as pd
    frame = pd.DataFrame({"index": [0], "id": ["id10001/a/00001.wav"], "label": [1], "xvector": ["[1. 2.]"]})
    with pytest.raises(RuntimeError, match="HIP device"):
        ev.plda_score_stat_object(frame, device="cpu")


def test_plot_images_is_out_of_scope():
    from xvector_amd import evaluate as ev
    with pytest.raises(NotImplementedError):
        ev.plda_score_stat_object.plot_images(object(), None)
