"""Trial evaluation (csrc/eval.hip) at its internal boundaries: kTile = 4096 elements per block, 16 per thread, 1024 per wave
in the scatter, a digit table of 256 x tiles entries scanned in chunks of 4096.

  sort         adversarial digit distributions at n = 4097 and 65537 (one tile plus one element; 17 tiles, whose digit table
               spills into a second scan chunk): all keys equal, keys that differ in one byte, sorted and reverse-sorted input,
               two values in halves; void entries (NaN scores: key 0xffffffff, bit 2) behind +inf.  The sizes themselves
               are in tests/test_evaluate_gpu.py's list.
  trial list   NaN cells and out-of-range index pairs through the C ABI (the Python wrapper raises on the first): the exact
               counters and the results over the kept trials
  sweep        the optimum at the last element of a thread / a tile and at the first of the next, runs of equal scores lying
               over a thread edge and a tile edge with the optimum at their end, one run over several tiles
  all pairs    skipped diagonals that leave the last tile all void, vectors, a view with a row stride
  workspace    a window of exactly xvec_eval_workspace_bytes(n) in a guarded buffer
Oracles and bars are those of tests/test_evaluate_gpu.py: tests/eer_ref.py (`naive` within 2^-22, `by_sort` within 1e-12) and a
stable sort of the host keys, bit for bit."""
import numpy as np
import pytest
import torch

import eer_ref
import score_support as ss
from test_evaluate_gpu import DEV, SORT_BAR, VAL_BAR, Tally, host_keys, scattered

pytestmark = pytest.mark.gpu

KEY_VOID = 0xFFFFFFFF
BIT_VOID = 2


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def check_sort(x, bits):
    """sorted_keys of the scores x against a stable sort of the host keys; a NaN score is a void entry.  Returns the sorted
    (keys, bits) of the device."""
    from xvector_amd import evaluate as ev
    x = np.asarray(x, dtype=np.float64)
    void = np.isnan(x)
    keys = host_keys(np.where(void, 0.0, x))
    keys[void] = KEY_VOID
    want_keys, perm = torch.sort(torch.from_numpy(keys), stable=True)
    want_bits = torch.from_numpy(np.where(void, BIT_VOID, bits).astype(np.uint8))[perm]
    got_keys, got_bits = ev.sorted_keys(torch.from_numpy(x).to(DEV), bits)
    assert torch.equal(got_keys.cpu(), want_keys)
    assert torch.equal(got_bits.cpu(), want_bits)
    again_keys, again_bits = ev.sorted_keys(torch.from_numpy(x).to(DEV), bits)
    assert torch.equal(again_keys, got_keys) and torch.equal(again_bits, got_bits)
    return got_keys.cpu().numpy(), got_bits.cpu().numpy()


# ------------------------------------------------------------------ the sort: digit distributions

@pytest.mark.parametrize("n", [4097, 65537])
def test_sort_of_equal_keys_keeps_the_input_order(n):
    """One digit bin holds the whole tile in every pass (ranks up to 4095): a stable sort leaves the bits where they were."""
    bits = np.random.default_rng(n).integers(0, 2, n).astype(np.uint8)
    for value in (0.75, -0.0, np.inf):
        keys, out = check_sort(np.full(n, value), bits)
        assert np.array_equal(out, bits) and (keys == keys[0]).all()


@pytest.mark.parametrize("byte", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [4097, 65537])
def test_sort_of_keys_that_differ_in_one_byte(n, byte):
    """Positive float32 scores 0x3f000000 | v << 8 byte (0x00400000 | v << 24 for the top byte, v < 128): three passes see one
    digit, one pass does all the work."""
    rng = np.random.default_rng(10 * n + byte)
    v = rng.integers(0, 128 if byte == 3 else 256, n).astype(np.uint32)
    x = (np.uint32(0x00400000 if byte == 3 else 0x3F000000) | (v << np.uint32(8 * byte))).view(np.float32).astype(np.float64)
    keys = host_keys(x)
    assert np.isfinite(x).all() and not ((keys ^ keys[0]) & ~(0xFF << (8 * byte))).any() and np.unique(keys).size > 100
    check_sort(x, rng.integers(0, 2, n).astype(np.uint8))


@pytest.mark.parametrize("n", [4097, 65537])
def test_sort_of_sorted_reversed_and_two_valued_input(n):
    rng = np.random.default_rng(n + 5)
    bits = rng.integers(0, 2, n).astype(np.uint8)
    up = np.sort(_f32(rng.normal(0, 3, n)))
    check_sort(up, bits)
    check_sort(up[::-1].copy(), bits)
    half = np.r_[np.full(n // 2, 1.5), np.full(n - n // 2, -2.25)]           # the larger value first: every element moves
    keys, out = check_sort(half, bits)
    assert np.array_equal(out, np.r_[bits[n // 2:], bits[:n // 2]])
    tile_halves = np.where((np.arange(n) % 4096) < 2048, 1.5, -2.25)         # ... and half of every tile one value
    check_sort(tile_halves, bits)


# ------------------------------------------------------------------ the sort: void entries

@pytest.mark.parametrize("n,n_nan", [(3 * 4096 + 100, 41), (3 * 4096 + 100, 5000), (4097, 1), (8192, 4096)])
def test_void_entries_sort_behind_infinity(n, n_nan):
    """NaN scores scattered over the tiles (5000 of them: more than a whole tile) with +inf and 3.4e38 among the rest."""
    rng = np.random.default_rng(n + n_nan)
    x = np.clip(np.round(rng.normal(0, 3, n)), -8, 7)
    order = rng.permutation(n)
    x[order[:n_nan]] = np.nan
    x[order[n_nan:n_nan + 9]] = np.resize([np.inf, 3.4e38, -np.inf, 1e39], 9)
    bits = rng.integers(0, 2, n).astype(np.uint8)
    keys, out = check_sort(x, bits)
    m = n - n_nan
    assert (keys[m:] == KEY_VOID).all() and (out[m:] == BIT_VOID).all()
    assert keys[m - 1] == 0xFF800000 and (out[:m] < BIT_VOID).all()         # +inf is the last valid entry


# ------------------------------------------------------------------ the trial list with voids, through the C ABI

def eval_trials_abi(mat, rows, cols, tgt, p_target=0.5):
    """xvec_eval_trials by hand: the xvec_eval_result as the library wrote it (the Python wrapper raises on n_nan / n_bad_index)."""
    from xvector_amd import evaluate as ev, hip
    n = len(tgt)
    need = int(hip.lib.xvec_eval_workspace_bytes(n))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((len(ev._Result._fields_),), float("nan"), dtype=torch.float64, device=DEV)
    r_d, c_d, t_d = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (rows.astype(np.int32), cols.astype(np.int32),
                                                                                  tgt.astype(np.uint8)))
    rc = hip.lib.xvec_eval_trials(mat.data_ptr(), mat.stride(0), mat.shape[0], mat.shape[1], r_d.data_ptr(), c_d.data_ptr(),
                                  t_d.data_ptr(), n, 1.0, 1.0, float(p_target), out.data_ptr(), ws.data_ptr(), need,
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_eval_last_error()
    torch.cuda.synchronize()
    return ev._Result.from_buffer_copy(out.cpu().numpy().tobytes())


def trials_with_voids(n, k, j):
    """(host matrix, rows, cols, targets, kept targets' scores, kept non-targets' scores): n trials on cells of their own, k of
    the cells NaN, j index pairs outside the matrix; at n = 3 x 4096 both kinds fall into each of the three tiles."""
    rng = np.random.default_rng(n + k)
    n_rows, n_cols = 120, 131
    pos, neg = eer_ref.draw(rng, n // 3, n - n // 3)
    vals = np.r_[pos, neg]
    tgt = np.r_[np.ones(pos.size, dtype=np.uint8), np.zeros(neg.size, dtype=np.uint8)]
    order = rng.permutation(n)
    vals, tgt = vals[order], tgt[order]
    cells = rng.permutation(n_rows * n_cols)[:n]
    rows, cols = (cells // n_cols).astype(np.int64), (cells % n_cols).astype(np.int64)
    host = np.full((n_rows, n_cols + 3), 1e30)                               # a cell no trial selects: finite and absurd
    host[rows, cols] = vals
    where = rng.permutation(n)
    nan_at, bad_at = where[:k], where[k:k + j]
    if n == 3 * 4096:
        assert {int(v) // 4096 for v in nan_at} == {0, 1, 2} == {int(v) // 4096 for v in bad_at}
    host[rows[nan_at], cols[nan_at]] = np.nan
    outside = [(-1, 0), (0, -1), (n_rows, 0), (0, n_cols), (2 ** 31 - 1, 5), (5, 2 ** 31 - 1), (-7, n_cols), (2 ** 31 - 1, 2 ** 31 - 1)]
    for i, t in enumerate(bad_at):
        dr, dc = outside[i % len(outside)]
        rows[t] = dr if dr else rows[t]
        cols[t] = dc if dc else cols[t]
    keep = np.ones(n, dtype=bool)
    keep[nan_at] = keep[bad_at] = False
    kp, kn = vals[keep & (tgt == 1)], vals[keep & (tgt == 0)]
    assert kp.size + kn.size == n - k - j
    return host, rows, cols, tgt, kp, kn


@pytest.mark.parametrize("n,k,j", [(3 * 4096, 37, 23), (4200, 60, 44), (4200, 60, 43), (3 * 4096, 4000, 200)])
def test_trial_list_with_nan_cells_and_bad_indices(n, k, j):
    """k NaN cells and j index pairs outside the matrix (negative, equal to the size, 2^31 - 1; row, column or both) spread
    over the tiles: the counters are exact and the results are those of the n - k - j kept trials (4096 and 4097 of 4200: the
    sorted prefix ends with a tile and one element into the next)."""
    from xvector_amd.evaluate import TrialResult
    host, rows, cols, tgt, kp, kn = trials_with_voids(n, k, j)
    mat = torch.from_numpy(host).to(DEV)[:, :host.shape[1] - 3]
    tally = Tally()
    for p_target in (0.5, 0.05):
        r = eval_trials_abi(mat, rows, cols, tgt, p_target)
        assert (r.n_nan, r.n_bad_index) == (k, j)
        assert (r.n_target, r.n_nontarget) == (kp.size, kn.size)
        res = TrialResult(r.eer, r.eer_threshold, r.far, r.frr, r.min_dcf, r.min_dcf_threshold, r.n_target, r.n_nontarget)
        tally.check(res, eer_ref.by_sort(kp, kn, p_target=p_target), kp, kn, eer_ref.by_sort_objectives_at, SORT_BAR, p_target,
                    f"[{n} trials, {k} NaN, {j} bad, p={p_target}]")
        assert eval_trials_abi(mat, rows, cols, tgt, p_target).eer == r.eer
    tally.done()


# ------------------------------------------------------------------ the sweep: the optimum at an edge

@pytest.mark.parametrize("n_neg,n_pos", [(15, 700), (16, 700), (17, 700), (4095, 700), (4096, 700), (4097, 700), (8192, 700),
                                         (4097, 1), (4097, 4095), (8193, 1), (8193, 4095)])
def test_optimum_at_a_thread_or_tile_edge(n_neg, n_pos):
    """Separable float32-exact scores: the optimum is the largest non-target, sorted index n_neg - 1 -- the last element of a
    thread (15), of a tile (4095, 8191), or the first of the next (16, 4096, 8192), there with 1, 700 or 4095 targets (the
    rest of the tile) behind it.  Both error rates and the cost are exactly 0 and both thresholds that score."""
    from xvector_amd import evaluate as ev
    rng = np.random.default_rng(n_neg + n_pos)
    pos, neg = _f32(rng.uniform(0.5, 2.0, n_pos)), _f32(rng.uniform(-2.0, 0.25, n_neg))
    mat, trials = scattered(pos, neg, n_neg)
    for p_target in (0.5, 0.01):
        res = ev.evaluate_trials(mat, trials, p_target=p_target)
        assert (res.n_target, res.n_nontarget) == (n_pos, n_neg)
        assert res.eer == 0.0 and res.far == 0.0 and res.frr == 0.0 and res.min_dcf == 0.0
        assert res.eer_th == neg.max() and res.min_dcf_th == neg.max()
    ref = eer_ref.by_sort(pos, neg)
    assert ref.eer == 0.0 and ref.min_dcf == 0.0 and ref.eer_th == neg.max() == ref.min_dcf_th


# ------------------------------------------------------------------ the sweep: runs of equal scores across edges

@pytest.mark.parametrize("start,n", [(4090, 9000), (10, 100), (8186, 17000)])
def test_run_of_equal_scores_across_an_edge(start, n):
    """Sorted order: `start` distinct non-targets, a run of 12 equal scores (its six non-targets first), then distinct targets:
    the optimum is the run's end, sorted index start + 11, at FRR = 6 / P and FAR = 0.  The run lies over the edge of a tile
    (4095 | 4096, 8191 | 8192) or of a thread (15 | 16); a threshold taken inside the run, where the six non-targets are
    behind and no target yet, would score a perfect 0."""
    from xvector_amd import evaluate as ev
    rng = np.random.default_rng(start)
    n_after = n - start - 12
    below = -1.0 - np.arange(start, 0, -1) / 8192.0                          # distinct, ascending, exact in float32
    above = 1.0 + np.arange(1, n_after + 1) / 8192.0
    assert np.array_equal(_f32(np.r_[below, above]), np.r_[below, above])
    vals = np.r_[below, np.full(12, 0.125), above]
    tgt = np.r_[np.zeros(start + 6, dtype=np.uint8), np.ones(6 + n_after, dtype=np.uint8)]
    # any input order that keeps the run's own order (the sort is stable): shuffle the positions, then sort the run's
    slot = rng.permutation(n)
    slot[start:start + 12] = np.sort(slot[start:start + 12])
    x, t = np.empty(n), np.empty(n, dtype=np.uint8)
    x[slot], t[slot] = vals, tgt
    mat = torch.from_numpy(x).to(DEV).reshape(1, n)
    trials = ev.TrialList(np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32), t)
    pos, neg = x[t == 1], x[t == 0]
    P, N = pos.size, neg.size
    assert P > N and N == start + 6
    tally = Tally()
    for p_target in (0.5, 0.05):
        res = ev.evaluate_trials(mat, trials, p_target=p_target)
        assert (res.frr, res.far, res.eer_th) == (6 / P, 0.0, 0.125)
        what = f"[run at {start}, n={n}, p={p_target}]"
        if n <= 10000:                                                       # (the walk is quadratic in n)
            tally.check(res, eer_ref.naive(pos, neg, p_target=p_target), pos, neg, eer_ref.naive_objectives_at, VAL_BAR,
                        p_target, what + " walk")
        tally.check(res, eer_ref.by_sort(pos, neg, p_target=p_target), pos, neg, eer_ref.by_sort_objectives_at, SORT_BAR,
                    p_target, what + " sort")
    tally.done()


@pytest.mark.parametrize("n_pos", [100, 4096])
def test_one_run_over_several_tiles(n_pos):
    """All 2 x 4096 + 1 scores equal: one candidate threshold, the last element of the third tile."""
    from xvector_amd import evaluate as ev
    n = 2 * 4096 + 1
    same = np.full(n, 0.75)
    mat, trials = scattered(same[:n_pos], same[n_pos:], n_pos)
    res = ev.evaluate_trials(mat, trials, p_target=0.05)
    ref = eer_ref.naive(same[:n_pos], same[n_pos:], p_target=0.05)
    assert (res.eer, res.far, res.frr, res.eer_th) == (0.5, 0.0, 1.0, 0.75) == (ref.eer, ref.far, ref.frr, ref.eer_th)
    assert abs(res.min_dcf - ref.min_dcf) <= VAL_BAR and res.min_dcf_th == 0.75
    assert (res.n_target, res.n_nontarget) == (n_pos, n - n_pos)


# ------------------------------------------------------------------ all pairs

@pytest.mark.parametrize("n_rows,n_cols,skip", [(64, 64, True), (64, 65, True), (1, 5000, False), (5000, 1, False),
                                                (1, 5000, True), (5000, 1, True), (65, 64, True)])
def test_all_pairs_with_void_tiles_and_row_strides(n_rows, n_cols, skip):
    """64 x 64 without its diagonal keeps 4032 of 4096 cells, 64 x 65 keeps 4096 of 4160: the last tile holds voids only.  The
    matrix is a view with ld = n_cols + 7 whose padding and skipped diagonal hold NaN."""
    from xvector_amd import evaluate as ev
    rng = np.random.default_rng(n_rows * 7 + n_cols)
    rl, cl = rng.integers(0, 5, n_rows), rng.integers(0, 5, n_cols)
    rl[0] = cl[-1] = 0                                                       # both kinds present off the diagonal
    cl[0] = 1
    self_set = n_rows == n_cols                                              # a set against itself: col_labels = None
    if self_set:
        cl = rl
    same = rl[:, None] == cl[None, :]
    wide = np.full((n_rows, n_cols + 7), np.nan)
    wide[:, :n_cols] = _f32(rng.normal(-1.5, 1.5, same.shape) + 2.5 * same)
    use = np.ones(same.shape, dtype=bool)
    if skip:
        np.fill_diagonal(use, False)
        np.fill_diagonal(wide[:, :n_cols], np.nan)
    host = wide[:, :n_cols]
    pos, neg = host[same & use], host[~same & use]
    assert pos.size and neg.size and pos.size + neg.size == n_rows * n_cols - (min(n_rows, n_cols) if skip else 0)
    dmat = torch.from_numpy(wide).to(DEV)[:, :n_cols]
    assert dmat.stride(0) == n_cols + 7
    tally = Tally()
    for p_target in (0.5, 0.05):
        res = ev.evaluate_all_pairs(dmat, rl, None if self_set else cl, skip_diagonal=skip, p_target=p_target)
        assert (res.n_target, res.n_nontarget) == (pos.size, neg.size)
        tally.check(res, eer_ref.by_sort(pos, neg, p_target=p_target), pos, neg, eer_ref.by_sort_objectives_at, SORT_BAR, p_target,
                    f"[all pairs {n_rows} x {n_cols} skip={skip} p={p_target}]")
        assert ev.evaluate_all_pairs(dmat, rl, None if self_set else cl, skip_diagonal=skip, p_target=p_target) == res
    tally.done()


# ------------------------------------------------------------------ workspace

@pytest.mark.parametrize("n", [4096, 4097])
def test_workspace_window_of_exactly_the_reported_size(n):
    """evaluate_trials and sorted_keys inside a 0xFF-filled window of xvec_eval_workspace_bytes(n) bytes in a guarded buffer;
    one byte less is refused before anything is launched."""
    from xvector_amd import evaluate as ev, hip
    pos, neg = eer_ref.draw(np.random.default_rng(n), n // 4, n - n // 4, 16)
    mat, trials = scattered(pos, neg, n)
    need = int(hip.lib.xvec_eval_workspace_bytes(n))
    assert need > 0
    first = ev.evaluate_trials(mat, trials, p_target=0.05)
    big, off = ss.window(need, DEV)
    assert ev.evaluate_trials(mat, trials, p_target=0.05, workspace=big[off:off + need]) == first
    torch.cuda.synchronize()
    assert ss.guards_intact(big, off, need)
    x = torch.from_numpy(np.r_[pos, neg]).to(DEV)
    bits = np.r_[np.ones(pos.size, dtype=np.uint8), np.zeros(neg.size, dtype=np.uint8)]
    want = ev.sorted_keys(x, bits)
    big, off = ss.window(need, DEV)
    got = ev.sorted_keys(x, bits, workspace=big[off:off + need])
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and ss.guards_intact(big, off, need)
    big, off = ss.window(need, DEV)
    with pytest.raises(hip.XvecError, match="workspace too small"):
        ev.evaluate_trials(mat, trials, p_target=0.05, workspace=big[off:off + need - 1])
    torch.cuda.synchronize()
    assert bool((big[off:off + need] == 0xFF).all()) and ss.guards_intact(big, off, need), "a refused call touched its workspace"
