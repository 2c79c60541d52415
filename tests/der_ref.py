"""The numpy restatement of include/xvec_der.h: the diarization error rate with the optimal speaker mapping.  Plain loops over
the turns, a uint64 mask per tick and side, integer counts; the optimum of the mapping comes from scipy's
linear_sum_assignment(maximize=True).  A plain module like vbx_ref.py; tests/test_der.py checks it against hand-computed cases
and a brute-force search, tests/test_der_gpu.py holds the device to it with ==."""
import itertools

import numpy as np
from scipy.optimize import linear_sum_assignment

MAX_SPEAKERS = 64
CHUNK_TICKS = 4096          # XVEC_DER_CHUNK_TICKS (tests/test_der.py ties the two)


def popcount(a):
    """Set bits of every element of a uint64 array."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def rasterise(turns, rec_len):
    """(masks: one uint64 [n_r] array per recording, ignored, boundaries: per recording the starts and ends of the valid
    turns as given)."""
    turns = np.asarray(turns, dtype=np.int64).reshape(-1, 4)
    masks = [np.zeros(int(n), dtype=np.uint64) for n in rec_len]
    bounds = [[] for _ in rec_len]
    ignored = 0
    for rec, start, end, spk in turns.tolist():
        if not 0 <= rec < len(rec_len) or not 0 <= spk < MAX_SPEAKERS or end <= start:
            ignored += 1
            continue
        n = int(rec_len[rec])
        lo, hi = max(start, 0), min(end, n)
        if lo < hi:
            masks[rec][lo:hi] |= np.uint64(1) << np.uint64(spk)
        bounds[rec] += [start, end]
    return masks, ignored, bounds


def best_correct(C):
    """The largest sum_i C[i][map(i)] over partial injective maps (entries are >= 0, so a full assignment reaches it)."""
    C = np.asarray(C, dtype=np.int64)
    rows, cols = linear_sum_assignment(C, maximize=True)
    return int(C[rows, cols].sum())


def brute_force_correct(C):
    """The same by trying every permutation of the speakers that occur (for a handful of speakers)."""
    C = np.asarray(C, dtype=np.int64)
    rows, cols = np.flatnonzero(C.any(axis=1)), np.flatnonzero(C.any(axis=0))
    k = max(len(rows), len(cols))
    sq = np.zeros((k, k), dtype=np.int64)
    sq[:len(rows), :len(cols)] = C[np.ix_(rows, cols)]
    return max((int(sum(sq[i, p[i]] for i in range(k))) for p in itertools.permutations(range(k))), default=0)


def check_map(C, mapping, correct):
    """What the header promises of a map: injective, reaches `correct`, reports no pair with C == 0."""
    C, mapping = np.asarray(C, dtype=np.int64), np.asarray(mapping, dtype=np.int64)
    assert mapping.shape == (MAX_SPEAKERS,) and ((mapping >= -1) & (mapping < MAX_SPEAKERS)).all()
    used = mapping[mapping >= 0]
    assert len(set(used.tolist())) == len(used), "the map is not injective"
    got = 0
    for i in np.flatnonzero(mapping >= 0):
        assert C[i, mapping[i]] > 0, f"the map reports the pair ({i}, {mapping[i]}), which never met"
        got += int(C[i, mapping[i]])
    assert got == int(correct), (got, int(correct))


def der(ref, hyp, rec_len, collar=0, skip_overlap=False):
    """A dict of per-recording int64 arrays scored / total / miss / fa / conf / correct, cooc [n_rec, 64, 64], der [n_rec + 1]
    float64 (the pooled value last) and ignored (reference, hypothesis)."""
    rec_len = [int(n) for n in rec_len]
    n_rec = len(rec_len)
    rm, r_ign, bounds = rasterise(ref, rec_len)
    hm, h_ign, _ = rasterise(hyp, rec_len)
    out = {k: np.zeros(n_rec, dtype=np.int64) for k in ("scored", "total", "miss", "fa", "conf", "correct")}
    cooc = np.zeros((n_rec, MAX_SPEAKERS, MAX_SPEAKERS), dtype=np.int64)
    for r in range(n_rec):
        n = rec_len[r]
        score = np.ones(n, dtype=bool)
        for b in bounds[r]:
            lo, hi = max(b - collar, 0), min(b + collar, n)
            if lo < hi:
                score[lo:hi] = False
        nref, nhyp = popcount(rm[r]), popcount(hm[r])
        if skip_overlap:
            score &= nref <= 1
        out["scored"][r] = score.sum()
        out["total"][r] = nref[score].sum()
        out["miss"][r] = np.maximum(nref - nhyp, 0)[score].sum()
        out["fa"][r] = np.maximum(nhyp - nref, 0)[score].sum()
        R, H = rm[r][score], hm[r][score]
        ref_spk = [i for i in range(MAX_SPEAKERS) if (R >> np.uint64(i) & np.uint64(1)).any()]
        hyp_spk = [j for j in range(MAX_SPEAKERS) if (H >> np.uint64(j) & np.uint64(1)).any()]
        for i in ref_spk:
            has_i = (R >> np.uint64(i) & np.uint64(1)).astype(bool)
            for j in hyp_spk:
                cooc[r, i, j] = ((H[has_i] >> np.uint64(j)) & np.uint64(1)).sum()
        out["correct"][r] = best_correct(cooc[r])
        out["conf"][r] = np.minimum(nref, nhyp)[score].sum() - out["correct"][r]
    err = out["miss"] + out["fa"] + out["conf"]
    rate = np.full(n_rec + 1, np.nan)
    for r in range(n_rec):
        if out["total"][r]:
            rate[r] = float(err[r]) / float(out["total"][r])
    if out["total"].sum():
        rate[n_rec] = float(err.sum()) / float(out["total"].sum())
    out.update(cooc=cooc, der=rate, ignored=np.array([r_ign, h_ign], dtype=np.int64))
    return out


def random_turns(rng, rec_len, n_turns, n_spk, max_len=None, slack=0):
    """Seeded random turns [n_turns, 4]: any recording, speakers below n_spk, starts and ends up to `slack` ticks outside."""
    rec = rng.integers(0, len(rec_len), n_turns)
    n = np.asarray(rec_len)[rec]
    start = rng.integers(-slack, n + slack, n_turns)
    length = rng.integers(1, (n if max_len is None else np.minimum(n, max_len)) + 1, n_turns)
    return np.stack([rec, start, start + length, rng.integers(0, n_spk, n_turns)], axis=1).astype(np.int64)


# ---------------------------------------------------------------- the cases of tests/test_der_gpu.py

def _t(*rows):
    return np.asarray(rows, dtype=np.int64).reshape(-1, 4)


EMPTY = np.zeros((0, 4), dtype=np.int64)
BATCH8 = (700, 1, CHUNK_TICKS + 37, 129, 2 * CHUNK_TICKS - 1, 64, 3000, 5)


def _random_case(seed, rec_len, n_ref, n_hyp, n_spk, max_len, slack):
    rng = np.random.default_rng(seed)
    return random_turns(rng, rec_len, n_ref, n_spk, max_len, slack), random_turns(rng, rec_len, n_hyp, n_spk, max_len, slack)


def gpu_cases():
    """{name: (ref, hyp, rec_len, collar, skip_overlap)}: the smallest shapes at which the kernels can still go wrong."""
    C = CHUNK_TICKS
    cases = {}
    lens = [1, C - 1, C, C + 1, 2 * C + 1]
    ref = [[r, 0, n, 0] for r, n in enumerate(lens)] + [[4, C, 2 * C, 2], [4, 2 * C, 2 * C + 1, 5], [3, C, C + 1, 1], [2, C - 1, C, 6]]
    hyp = [[r, 0, n, 1] for r, n in enumerate(lens)] + [[4, C - 1, C + 1, 3], [4, 0, 1, 5], [3, C - 1, C, 2], [1, C - 2, C - 1, 4]]
    cases["lengths_and_chunk_edges"] = (_t(*ref), _t(*hyp), lens, 0, False)
    cases["clipped_at_both_ends"] = (_t([0, -20, 30, 1], [0, 90, 500, 2], [1, -5, 60, 0], [0, 200, 300, 4], [0, -50, -10, 4]),
                                     _t([0, -1000, 1000, 1], [1, 40, 51, 3], [1, 50, 60, 2]), [100, 50], 0, False)
    edge = (0, 31, 32, 63)
    ref = [[0, 10 * k, 10 * k + 10, s] for k, s in enumerate(edge)] + [[0, 45, 47, s] for s in range(64)]
    hyp = [[0, 10 * k, 10 * k + 10, s] for k, s in enumerate(reversed(edge))] + [[0, 5, 35, 63], [0, 46, 48, 0]] + [[0, 46, 48, s] for s in range(64)]
    cases["word_halves_sign_bit_and_all_64"] = (_t(*ref), _t(*hyp), [50], 0, False)
    some = _t([0, 3, 40, 2], [0, 30, 90, 5], [1, 0, 20, 0])
    cases["empty_hypothesis"] = (some, EMPTY, [100, 20], 0, False)
    cases["empty_reference"] = (EMPTY, some, [100, 20], 0, False)
    cases["both_empty"] = (EMPTY, EMPTY, [7, 3], 0, False)
    cases["one_pair_over_70000_ticks"] = (_t([0, 0, 70000, 3]), _t([0, 0, 70000, 7]), [70000], 0, False)
    n = 300
    cases["alternating_pairs_every_tick"] = (_t(*[[0, t, t + 1, t % 3] for t in range(n)]),
                                             _t(*[[0, t, t + 1, 10 + t % 5] for t in range(n)]), [n], 0, False)
    lens = [500, 2 * C + 1, 90]
    ref, hyp = _random_case(11, lens, 30, 30, 6, 400, 20)
    cases["collar_1"] = (ref, hyp, lens, 1, False)
    cases["collar_swallows_a_recording"] = (_t([0, 10, 20, 0], [0, 15, 45, 1]), _t([0, 0, 50, 0], [1, 0, 30, 0]), [50, 30], 1000, False)
    cases["collar_zones_clipped_at_0_and_n"] = (_t([0, 0, 40, 0], [0, 40, 64, 1], [1, 0, 33, 2], [1, 1, 32, 3]),
                                                _t([0, 0, 64, 1], [1, 0, 33, 3]), [64, 33], 3, False)
    ref, hyp = _random_case(12, lens, 40, 40, 5, 600, 10)
    cases["skip_overlap"] = (ref, hyp, lens, 2, True)
    bad = [[-1, 0, 5, 0], [2, 0, 5, 0], [0, 0, 5, -1], [0, 0, 5, 64], [0, 5, 5, 0], [1, 9, 3, 0]]
    cases["invalid_turns_of_each_kind"] = (_t(*bad, [0, 2, 30, 1], [1, 0, 9, 0]), _t([0, 0, 25, 4], *bad[:5], [1, 3, 10, 2], bad[5]),
                                           [40, 10], 1, False)
    ref, hyp = _random_case(13, BATCH8, 120, 120, 7, 900, 15)
    cases["batch_of_eight"] = (ref, hyp, list(BATCH8), 2, False)
    return cases


def only_recording(turns, r):
    """The valid-or-not turns of recording r alone, renumbered to recording 0."""
    t = np.asarray(turns, dtype=np.int64).reshape(-1, 4)
    t = t[t[:, 0] == r].copy()
    t[:, 0] = 0
    return t


def assign_cases():
    """{name: C [64, 64] int64}: the crafted matrices of xvec_der_assign."""
    top = 2 ** 31 - 1
    rng = np.random.default_rng(2024)
    z = lambda: np.zeros((MAX_SPEAKERS, MAX_SPEAKERS), dtype=np.int64)
    cases = {}
    c = z()
    c[:2, :2] = [[5, 4], [4, 0]]
    cases["greedy_gives_5_optimum_8"] = c
    c = z()
    c[np.ix_([2, 40, 63], [0, 5, 17, 31, 32, 50, 63])] = rng.integers(1, 1000, (3, 7))
    cases["3_reference_x_7_hypothesis"] = c
    cases["7_reference_x_3_hypothesis"] = c.T.copy()
    cases["all_zeros"] = z()
    cases["all_entries_equal"] = np.full((MAX_SPEAKERS, MAX_SPEAKERS), 7, dtype=np.int64)
    c = z()
    c[np.arange(MAX_SPEAKERS), rng.permutation(MAX_SPEAKERS)] = top
    cases["permutation_times_2^31-1"] = c
    cases["random_full_range_a"] = rng.integers(0, top + 1, (MAX_SPEAKERS, MAX_SPEAKERS))
    cases["random_full_range_b"] = rng.integers(top - 1000, top + 1, (MAX_SPEAKERS, MAX_SPEAKERS))
    c = rng.integers(0, 500, (MAX_SPEAKERS, MAX_SPEAKERS))
    c[rng.random(c.shape) < 0.8] = 0
    cases["random_sparse"] = c
    c = z()                # rows 0 .. 62 take the diagonal (1001 each); row 63 has column 0 alone, and its 100 is worth moving every
    c[np.arange(63), np.arange(63)] = 1001         # other row one column on (1000 each) but no row is worth dropping
    c[np.arange(63), np.arange(1, 64)] = 1000
    c[63, 0] = 100
    cases["path_through_every_row"] = c
    return cases
