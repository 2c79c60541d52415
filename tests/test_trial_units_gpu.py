"""The units that consume trials -- trial evaluation (csrc/eval.hip), score calibration (csrc/calib.hip) and the trial report
(csrc/report.hip) -- leave out exactly the same trials: all of them read a trial through csrc/trial_device.h's read_trial.

One seeded trial list over a 67 x 61 matrix with planted cells (three NaN, +inf, -inf, a -0.0 / +0.0 pair, a run of six equal
scores), which repeats cells, hits every planted one and carries two bad indices (a row of -1, a column equal to n_cols; their
cells are never read), at n_trials = 4095, 4096 and 4097: one below, at and one above the 4096-trial tile that eval.hip, the
hull's first level and the DET pass share.  n_target, n_nontarget, n_nan and n_bad_index of xvec_eval_trials, xvec_calib_fit
(which ends with XVEC_CALIB_INF_SCORE and still reports its counts), xvec_calib_cllr and xvec_report_det's header, and
xvec_calib_min_cllr's n_target, n_nontarget and n_left_out, all equal a numpy count of the list; the kept prefix of
xvec_eval_sorted_keys (the call behind evaluate.sorted_keys, here with the index arrays) has n_target + n_nontarget entries in
ascending key order; the last DET point has tp = n_target and nn = n_nontarget.  The same counts for every cell of a 65 x 65
matrix (4225 cells) as a trial, labels of seven classes, with and without the diagonal: n_bad_index is 0 there."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BIT_VOID = 2


def planted_matrix(n_rows, n_cols, seed):
    """(matrix, [(row, col), ...] of the planted cells); the NaN at (3, 3) lies on the diagonal."""
    s = np.random.default_rng(seed).normal(0.0, 3.0, (n_rows, n_cols))
    cells = {(3, 3): np.nan, (13, n_cols - 1): np.nan, (n_rows - 1, 7): np.nan, (5, 6): np.inf, (40, 33): -np.inf,
             (1, 2): -0.0, (2, 1): 0.0}
    cells.update({(10, j): 0.25 for j in range(6)})
    for (i, j), v in cells.items():
        s[i, j] = v
    return s, list(cells)


def count(s, rows, cols, tgt):
    """dict(n_target, n_nontarget, n_nan, n_bad_index) of a trial list by the rule of include/xvec_eval.h"""
    inside = (rows >= 0) & (rows < s.shape[0]) & (cols >= 0) & (cols < s.shape[1])
    nan = np.zeros(len(rows), dtype=bool)
    nan[inside] = np.isnan(s[rows[inside], cols[inside]])
    kept = inside & ~nan
    return dict(n_target=int((kept & tgt).sum()), n_nontarget=int((kept & ~tgt).sum()), n_nan=int(nan.sum()),
                n_bad_index=int((~inside).sum()))


def counts_of(r):
    return {k: int(getattr(r, k)) for k in ("n_target", "n_nontarget", "n_nan", "n_bad_index")}


def eval_record(call, n, *args):
    """xvec_eval_result of a raw call (evaluate_trials raises on the first NaN or bad index)."""
    from xvector_amd import evaluate as ev, hip
    ws = torch.empty(int(hip.lib.xvec_eval_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
    out = torch.empty(len(ev._Result._fields_), dtype=torch.float64, device=DEV)
    rc = call(*args, 1.0, 1.0, 0.5, out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_eval_last_error()
    return ev._Result.from_buffer_copy(out.cpu().numpy().tobytes())


@pytest.fixture(scope="module")
def listed():
    """The matrix on the device and the longest trial list; the shorter ones are its prefixes."""
    s, cells = planted_matrix(67, 61, seed=20)
    rng = np.random.default_rng(21)
    n = 4097
    rows, cols = rng.integers(0, 67, n), rng.integers(0, 61, n)      # cells repeat: 4097 draws of 4087
    for k, (i, j) in enumerate(cells):
        rows[3 * k], cols[3 * k] = i, j
    rows[100], cols[200] = -1, 61
    return s, torch.from_numpy(s).to(DEV), rows, cols, rng.integers(0, 2, n).astype(bool)


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_every_unit_counts_the_same_trials(listed, n):
    from xvector_amd import calibrate as cal, evaluate as ev, hip, report as rp
    s, s_d, rows, cols, tgt = listed
    rows, cols, tgt = rows[:n], cols[:n], tgt[:n]
    want = count(s, rows, cols, tgt)
    assert want["n_nan"] >= 3 and want["n_bad_index"] == 2 and want["n_target"] > 0 and want["n_nontarget"] > 0
    kept = want["n_target"] + want["n_nontarget"]
    trials = ev.TrialList(rows, cols, tgt)
    r_d, c_d, t_d = trials.on(DEV)
    shape = (s_d.data_ptr(), s_d.stride(0), 67, 61, r_d.data_ptr(), c_d.data_ptr(), t_d.data_ptr(), n)

    assert counts_of(eval_record(hip.lib.xvec_eval_trials, n, *shape)) == want
    assert counts_of(cal.fit_calibration(s_d, trials).result()) == want      # (status XVEC_CALIB_INF_SCORE: the counts stand)
    assert counts_of(cal.cllr(s_d, trials)) == want
    pav = cal.pav_segments(s_d, trials, capacity=0)
    assert (pav.n_target, pav.n_nontarget, pav.n_left_out) == (want["n_target"], want["n_nontarget"], n - kept)

    keys = torch.empty(n, dtype=torch.int32, device=DEV)
    bits = torch.empty(n, dtype=torch.uint8, device=DEV)
    ws = torch.empty(int(hip.lib.xvec_eval_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
    rc = hip.lib.xvec_eval_sorted_keys(*shape, keys.data_ptr(), bits.data_ptr(), ws.data_ptr(), ws.numel(),
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_eval_last_error()
    keys, bits = keys.cpu().numpy().view(np.uint32), bits.cpu().numpy()
    assert (bits[:kept] != BIT_VOID).all() and (bits[kept:] == BIT_VOID).all()
    assert (np.diff(keys[:kept].astype(np.int64)) >= 0).all()

    det = rp.det_curve(s_d, trials)
    assert counts_of(det) == want
    assert (int(det.tp[-1]), int(det.nn[-1])) == (want["n_target"], want["n_nontarget"])


@pytest.mark.parametrize("skip_diagonal", [False, True])
def test_every_unit_counts_the_same_cells(skip_diagonal):
    from xvector_amd import calibrate as cal, hip, report as rp
    n = 65
    s, _ = planted_matrix(n, n, seed=22)
    labels = (np.arange(n) % 7).astype(np.int32)
    ii, jj = np.nonzero(~np.eye(n, dtype=bool) if skip_diagonal else np.ones((n, n), dtype=bool))
    want = count(s, ii, jj, labels[ii] == labels[jj])
    assert want["n_bad_index"] == 0 and want["n_nan"] == (2 if skip_diagonal else 3)
    s_d, l_d = torch.from_numpy(s).to(DEV), torch.from_numpy(labels).to(DEV)

    got = eval_record(hip.lib.xvec_eval_all_pairs, n * n, s_d.data_ptr(), s_d.stride(0), n, n, l_d.data_ptr(), l_d.data_ptr(),
                      int(skip_diagonal))
    assert counts_of(got) == want
    assert counts_of(cal.fit_calibration_all_pairs(s_d, labels, skip_diagonal=skip_diagonal).result()) == want
    assert counts_of(cal.cllr_all_pairs(s_d, labels, skip_diagonal=skip_diagonal)) == want
    det = rp.det_curve_all_pairs(s_d, labels, skip_diagonal=skip_diagonal)
    assert counts_of(det) == want
    assert (int(det.tp[-1]), int(det.nn[-1])) == (want["n_target"], want["n_nontarget"])
