"""CPU-only checks of DER scoring (include/xvec_der.h): the numpy restatement tests/der_ref.py against hand-computed cases, a
per-tick restatement with Python sets and a brute-force search over all maps; that it handles every case the GPU test relies on;
read_rttm against write_rttm; the host-only plan (csrc/der_plan.h) through its dump program; and the C ABI's argument errors
(each returns before the library touches a device)."""
import ctypes
import io
import math

import numpy as np
import pytest

import der_ref
from scipy.optimize import linear_sum_assignment
from hipcc_support import header_constants, host_program, needs_host_cxx

P = 0x1000          # a pointer that is never followed: every call here fails its argument checks first
CHUNK = der_ref.CHUNK_TICKS


def _t(*rows):
    return np.asarray(rows, dtype=np.int64).reshape(-1, 4)


# ---------------------------------------------------------------- the restatement

def _counts(o, r=0):
    return tuple(int(o[k][r]) for k in ("scored", "total", "miss", "fa", "conf", "correct"))


def test_oracle_on_hand_computed_cases():
    # a miss: the hypothesis stops four ticks early
    o = der_ref.der(_t([0, 0, 10, 0]), _t([0, 0, 6, 0]), [10])
    assert _counts(o) == (10, 10, 4, 0, 0, 6) and o["der"][0] == 4 / 10 and o["der"][1] == 4 / 10
    # a false alarm: it goes on four ticks too long
    o = der_ref.der(_t([0, 0, 6, 0]), _t([0, 0, 10, 0]), [10])
    assert _counts(o) == (10, 6, 0, 4, 0, 6) and o["der"][0] == 4 / 6
    # a confusion: X covers A and the first four ticks of B; A -> X (10), B -> Y (6), the four ticks of B under X are confused
    ref, hyp = _t([0, 0, 10, 0], [0, 10, 20, 1]), _t([0, 0, 14, 0], [0, 14, 20, 1])
    o = der_ref.der(ref, hyp, [20])
    assert _counts(o) == (20, 20, 0, 0, 4, 16) and o["der"][0] == 4 / 20
    assert o["cooc"][0, :2, :2].tolist() == [[10, 0], [4, 6]] and o["cooc"].sum() == 20
    # overlap on both sides: ticks 0-3 A|X, 4-5 AB|X (a miss each), 6-7 AB|XY, 8-9 A|XY (a false alarm each)
    ref, hyp = _t([0, 0, 10, 0], [0, 4, 8, 1]), _t([0, 0, 10, 0], [0, 6, 10, 1])
    o = der_ref.der(ref, hyp, [10])
    assert _counts(o) == (10, 14, 2, 2, 0, 12) and o["der"][0] == 4 / 14
    assert o["cooc"][0, :2, :2].tolist() == [[10, 4], [4, 2]]
    # ... and with skip_overlap ticks 4-7 leave: 0-3 A|X, 8-9 A|XY
    o = der_ref.der(ref, hyp, [10], skip_overlap=True)
    assert _counts(o) == (6, 6, 0, 2, 0, 6) and o["der"][0] == 2 / 6 and o["cooc"][0, 0, :2].tolist() == [6, 2]
    # a collar that removes a boundary error: the hypothesis changes speaker two ticks late
    ref, hyp = _t([0, 0, 10, 0], [0, 10, 20, 1]), _t([0, 0, 12, 0], [0, 12, 20, 1])
    o = der_ref.der(ref, hyp, [20])
    assert _counts(o) == (20, 20, 0, 0, 2, 18) and o["der"][0] == 2 / 20
    o = der_ref.der(ref, hyp, [20], collar=2)      # unscored: 0-1, 8-11, 18-19
    assert _counts(o) == (12, 12, 0, 0, 0, 12) and o["der"][0] == 0.0
    # two recordings pool by summed errors over summed totals; a recording without reference speech is NaN
    o = der_ref.der(_t([0, 0, 10, 0]), _t([0, 0, 6, 0], [1, 0, 5, 0]), [10, 5])
    assert o["der"][0] == 0.4 and math.isnan(o["der"][1]) and o["der"][2] == (4 + 5) / 10 and o["fa"].tolist() == [0, 5]
    # touching turns of one speaker are not merged: the collar takes the seam
    o = der_ref.der(_t([0, 0, 10, 0], [0, 10, 20, 0]), _t([0, 0, 20, 0]), [20], collar=1)
    assert int(o["scored"][0]) == 20 - 1 - 2 - 1


def _by_sets(ref, hyp, rec_len, collar, skip_overlap):
    """The definition once more, tick by tick with Python sets (valid turns only)."""
    out = []
    for r, n in enumerate(rec_len):
        R, H, un = [set() for _ in range(n)], [set() for _ in range(n)], [False] * n
        for side, turns in ((R, ref), (H, hyp)):
            for rec, s, e, k in turns.tolist():
                if rec != r:
                    continue
                for t in range(max(s, 0), min(e, n)):
                    side[t].add(k)
                if side is R:
                    for b in (s, e):
                        for t in range(max(b - collar, 0), min(b + collar, n)):
                            un[t] = True
        scored = total = miss = fa = both = 0
        C = np.zeros((64, 64), dtype=np.int64)
        for t in range(n):
            if un[t] or (skip_overlap and len(R[t]) > 1):
                continue
            scored += 1
            total += len(R[t])
            miss += max(len(R[t]) - len(H[t]), 0)
            fa += max(len(H[t]) - len(R[t]), 0)
            both += min(len(R[t]), len(H[t]))
            for i in R[t]:
                for j in H[t]:
                    C[i, j] += 1
        out.append((scored, total, miss, fa, both, C))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_oracle_against_sets_and_a_brute_force_search_over_all_maps(seed):
    rng = np.random.default_rng(100 + seed)
    lens = [int(v) for v in rng.integers(1, 80, 3)]
    n_spk = 2 + seed % 4                             # 2 .. 5 speakers a side
    ref = der_ref.random_turns(rng, lens, 12, n_spk, 30, 5)
    hyp = der_ref.random_turns(rng, lens, 12, n_spk, 30, 5)
    collar, skip = seed % 3, bool(seed % 2)
    o = der_ref.der(ref, hyp, lens, collar, skip)
    for r, (scored, total, miss, fa, both, C) in enumerate(_by_sets(ref, hyp, lens, collar, skip)):
        best = der_ref.brute_force_correct(C)
        assert np.array_equal(o["cooc"][r], C)
        assert _counts(o, r) == (scored, total, miss, fa, both - best, best), (seed, r)


def test_oracle_handles_every_case_of_the_gpu_test():
    cases = der_ref.gpu_cases()
    want = {"lengths_and_chunk_edges", "clipped_at_both_ends", "word_halves_sign_bit_and_all_64", "empty_hypothesis", "empty_reference",
            "both_empty", "one_pair_over_70000_ticks", "alternating_pairs_every_tick", "collar_1", "collar_swallows_a_recording",
            "collar_zones_clipped_at_0_and_n", "skip_overlap", "invalid_turns_of_each_kind", "batch_of_eight"}
    assert set(cases) == want
    out = {k: der_ref.der(*v) for k, v in cases.items()}
    for name, o in out.items():
        err = o["miss"] + o["fa"] + o["conf"]
        assert (o["conf"] >= 0).all() and (o["correct"] >= 0).all() and (o["scored"] <= np.asarray(cases[name][2])).all(), name
        assert all(math.isnan(d) == (t == 0) and (t == 0 or d == e / t) for d, e, t in zip(o["der"], err, o["total"])), name
    assert cases["lengths_and_chunk_edges"][2] == [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
    o = out["lengths_and_chunk_edges"]
    assert o["scored"].tolist() == cases["lengths_and_chunk_edges"][2] and o["cooc"][4, 2, 3] == 1 and o["cooc"][4, 0, 1] == 2 * CHUNK + 1
    o = out["word_halves_sign_bit_and_all_64"]
    assert (o["cooc"][0] > 0).all() and o["cooc"][0, 63, 63] > 0 and o["cooc"][0, 0, 63] >= 10        # tick 46 has all 64 x 64 pairs
    o = out["empty_hypothesis"]
    assert np.array_equal(o["miss"], o["total"]) and o["total"].tolist() == [97, 20] and o["der"].tolist() == [1.0, 1.0, 1.0]
    o = out["empty_reference"]
    assert np.isnan(o["der"]).all() and o["fa"].tolist() == [97, 20] and not o["total"].any()
    o = out["both_empty"]
    assert np.isnan(o["der"]).all() and o["scored"].tolist() == [7, 3] and not (o["fa"].any() or o["miss"].any())
    o = out["one_pair_over_70000_ticks"]
    assert o["cooc"][0, 3, 7] == 70000 > 0xffff and o["cooc"].sum() == 70000 and o["der"][0] == 0.0 and 70000 > 16 * CHUNK
    o = out["alternating_pairs_every_tick"]
    assert (o["cooc"][0] > 0).sum() == 15 and o["total"][0] == 300
    o = out["collar_swallows_a_recording"]
    assert o["scored"].tolist() == [0, 30] and o["fa"].tolist() == [0, 30] and np.isnan(o["der"]).all()
    o = out["collar_zones_clipped_at_0_and_n"]
    assert o["scored"].tolist() == [64 - 3 - 6 - 3, 33 - 4 - 4]
    o = out["invalid_turns_of_each_kind"]
    assert o["ignored"].tolist() == [6, 6]
    ref, hyp, lens, collar, skip = cases["invalid_turns_of_each_kind"]
    valid = lambda t: t[(t[:, 0] >= 0) & (t[:, 0] < 2) & (t[:, 3] >= 0) & (t[:, 3] < 64) & (t[:, 2] > t[:, 1])]
    clean = der_ref.der(valid(ref), valid(hyp), lens, collar, skip)
    assert all(np.array_equal(o[k], clean[k], equal_nan=True) for k in o if k != "ignored") and not clean["ignored"].any()
    # a recording alone is its part of the batch
    ref, hyp, lens, collar, skip = cases["batch_of_eight"]
    o = out["batch_of_eight"]
    assert len(set(lens)) == 8 and (o["total"] > 0).sum() >= 5
    for r, n in enumerate(lens):
        alone = der_ref.der(der_ref.only_recording(ref, r), der_ref.only_recording(hyp, r), [n], collar, skip)
        assert np.array_equal(alone["cooc"][0], o["cooc"][r]) and np.array_equal(alone["der"][0], o["der"][r], equal_nan=True)


def test_oracle_handles_every_assign_case():
    cases = der_ref.assign_cases()
    top = 2 ** 31 - 1
    assert all(c.shape == (64, 64) and c.min() >= 0 and c.max() <= top for c in cases.values())
    best = {k: der_ref.best_correct(c) for k, c in cases.items()}
    assert best["greedy_gives_5_optimum_8"] == 8 and best["all_zeros"] == 0 and best["all_entries_equal"] == 64 * 7
    assert best["permutation_times_2^31-1"] == 64 * top > 2 ** 32
    c = cases["3_reference_x_7_hypothesis"]
    assert best["3_reference_x_7_hypothesis"] == best["7_reference_x_3_hypothesis"] == der_ref.brute_force_correct(c)
    assert (c.any(axis=1).sum(), c.any(axis=0).sum()) == (3, 7)
    assert best["random_full_range_a"] > 2 ** 36 and cases["random_full_range_a"].max() > 2 ** 30
    # the path case: without row 63 the diagonal is best; row 63's 100 pays for shifting every other row one column on, and
    # no smaller change reaches the optimum: the only map that does uses every row and every column
    c = cases["path_through_every_row"]
    assert best["path_through_every_row"] == 100 + 63 * 1000 and der_ref.best_correct(c[:63]) == 63 * 1001
    rows, cols = linear_sum_assignment(c, maximize=True)
    assert cols.tolist() == list(range(1, 64)) + [0]
    assert all(der_ref.best_correct(np.delete(c, r, axis=0)) < best["path_through_every_row"] for r in (0, 30, 62))
    # check_map refuses what the header forbids
    m = np.full(64, -1)
    der_ref.check_map(cases["all_zeros"], m, 0)
    m[:2] = [1, 0]
    der_ref.check_map(cases["greedy_gives_5_optimum_8"], m, 8)
    with pytest.raises(AssertionError, match="never met"):
        der_ref.check_map(cases["greedy_gives_5_optimum_8"], np.concatenate([[0, 1], m[2:]]), 5)
    with pytest.raises(AssertionError, match="injective"):
        der_ref.check_map(cases["all_entries_equal"], np.zeros(64, dtype=np.int64), 7)


# ---------------------------------------------------------------- RTTM

@pytest.mark.parametrize("frame_shift", [0.01, 0.0125])
def test_read_rttm_inverts_write_rttm(frame_shift, tmp_path):
    from xvector_amd import der
    from xvector_amd.diarize import write_rttm
    rng = np.random.default_rng(5)
    rows = []
    for rec in range(3):
        t, n_spk = 0, 0
        for _ in range(40):
            t += int(rng.integers(0, 50))
            length = int(rng.integers(1, 700))
            spk = int(rng.integers(0, n_spk + 1))          # a new speaker is the next number: order of first appearance
            n_spk = max(n_spk, spk + 1)
            rows.append([rec, t, t + length, spk])
            t += length - int(rng.integers(0, min(length, 20)))           # turns may overlap
    t = np.asarray(rows, dtype=np.int64)
    names = ["rec_a", "rec-b", "c"]
    path = tmp_path / "t.rttm"
    write_rttm(t, names, str(path), frame_shift=frame_shift)
    back, rec_names, spk_names = der.read_rttm(str(path), frame_shift=frame_shift)
    assert back.dtype == np.int64 and np.array_equal(back, t) and rec_names == names
    assert [len(s) for s in spk_names] == [int(t[t[:, 0] == r, 3].max()) + 1 for r in range(3)] and spk_names[0][0] == "spk0"
    # an open file, other line types skipped, and recordings numbered by `names`
    text = "SPKR-INFO rec-b 1 <NA> <NA> <NA> unknown spk0 <NA> <NA>\n\n" + path.read_text()
    back2, rec2, _ = der.read_rttm(io.StringIO(text), frame_shift=frame_shift, names=["c", "rec_a", "rec-b", "never"])
    assert rec2 == ["c", "rec_a", "rec-b", "never"] and np.array_equal(back2[:, 1:], t[:, 1:])
    assert np.array_equal(back2[:, 0], np.asarray([1, 2, 0])[t[:, 0]])
    with pytest.raises(ValueError, match="not among"):
        der.read_rttm(str(path), names=["rec_a"])


def test_read_rttm_refuses_a_65th_speaker():
    from xvector_amd import der
    line = "SPEAKER {} 1 {:.3f} 0.500 <NA> <NA> s{} <NA> <NA>\n"
    ok = "".join(line.format("a", 0.5 * k, k) for k in range(64)) + "".join(line.format("b", 0.5 * k, k) for k in range(3))
    t, recs, spk = der.read_rttm(io.StringIO(ok))
    assert t.shape == (67, 4) and t[63].tolist() == [0, 3150, 3200, 63] and [len(s) for s in spk] == [64, 3]
    with pytest.raises(ValueError, match="speaker 65 of 'a'"):
        der.read_rttm(io.StringIO(ok + line.format("a", 40.0, 64)))
    assert der.read_rttm(io.StringIO(""))[0].shape == (0, 4)


# ---------------------------------------------------------------- the host-only plan

@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return host_program("der_plan_dump", tmp_path_factory.mktemp("der_plan"))


def _a256(n):
    return -(-n // 256) * 256


PLAN_RECORDINGS = ([1], [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1], [3000] * 64, [360000] * 16, list(der_ref.BATCH8), [5, 1, 1, 70000])


@needs_host_cxx
def test_plan_layout_is_the_restated_one_and_what_the_library_reports(plan):
    from xvector_amd import hip
    for counts in PLAN_RECORDINGS:
        v = [int(x) for x in plan(["layout " + " ".join(map(str, counts))])[0].split()[1:]]
        n_rec, N = len(counts), sum(counts)
        want, at = [], 0
        for nbytes in (8 * (n_rec + 1), 4 * (n_rec + 1), 8 * N, 8 * N, 4 * (N // 32 + 1), 8 * 4 * n_rec, 8 * 2, 8 * 64 * 64 * n_rec):
            want.append(at)
            at += _a256(nbytes)
        assert v == want + [want[2], at], counts            # zero_from: everything behind rec_start and blk_start
        rs = (ctypes.c_int64 * (n_rec + 1))(*np.concatenate([[0], np.cumsum(counts)]).tolist())
        assert hip.lib.xvec_der_workspace_bytes(rs, n_rec, 40, 0) == at


@needs_host_cxx
def test_plan_block_to_chunk_map_and_launches(plan):
    from xvector_amd import der
    threads = der.THREADS
    assert CHUNK == der.CHUNK_TICKS == threads * der.WAVE_ROWS
    for counts in PLAN_RECORDINGS:
        want = [(r, k, k * CHUNK, min(CHUNK, n - k * CHUNK)) for r, n in enumerate(counts) for k in range(-(-n // CHUNK))]
        if len(want) <= 64:
            got = plan(["blocks " + " ".join(map(str, counts))])[0].split()
            assert got[0] == "blocks" and int(got[1]) == len(want)
            assert [tuple(int(x) for x in g.split(":")) for g in got[2:]] == want, counts
        # every tick of every recording is in exactly one block
        assert [sum(w[3] for w in want if w[0] == r) for r in range(len(counts))] == list(counts)
        for m_ref, m_hyp in ((0, 0), (1, 0), (3, 1), (40, 41), (2560, 2560)):
            got = plan([f"launch {m_ref} {m_hyp} " + " ".join(map(str, counts))])[0]
            assert got == f"launch {-(-(m_ref + m_hyp) // 4) + 1} {threads} {len(want)} {threads} {len(counts)} 64 1 {threads}"


@needs_host_cxx
def test_plan_refusals_one_text_each(plan):
    got = plan(["check 3 1 4", "check 1", "check 3 0 4", "start 0 5 4", "start 1 4", "start 0", "nullstart 2", "nullstart 0",
                f"check {2 ** 31 - 1}", f"check 5 {2 ** 31 - 5}", f"check {2 ** 30} {2 ** 30} 1",
                "counts 0 0", "counts 5 7", "counts -1 0", "counts 0 -3", f"counts {2 ** 31} 0", f"counts 0 {2 ** 31 - 1}",
                "collar 0", "collar 25", "collar -1",
                "turns 0 0 ref", "turns 1 4 ref", "turns 0 4 ref", "turns 0 2 hyp"])
    assert got[:2] == ["ok", "ok"]
    empty = "refused recording 1 is empty or rec_start decreases: every recording needs a tick"
    assert got[2] == empty and got[3] == empty
    assert got[4] == "refused rec_start must begin at 0 (got 1)" and got[5] == "refused n_rec = 0: need at least one recording"
    assert got[6] == "refused null pointer: rec_start" and got[7] == "refused n_rec = 0: need at least one recording"
    assert got[8] == "ok"
    assert got[9] == f"refused {2 ** 31} ticks up to recording 1: the total must stay below 2^31"
    assert got[10] == got[9]                         # the first recording that crosses the bound is named
    assert got[11:13] == ["ok", "ok"]
    assert got[13] == "refused m_ref = -1 must not be negative" and got[14] == "refused m_hyp = -3 must not be negative"
    assert got[15] == f"refused {2 ** 31} and 0 turns: a side may have 2^31 - 1 at most" and got[16] == "ok"
    assert got[17:19] == ["ok", "ok"] and got[19] == "refused collar = -1 must not be negative"
    assert got[20:22] == ["ok", "ok"]
    assert got[22] == "refused null pointer: ref_turns with m_ref = 4" and got[23] == "refused null pointer: hyp_turns with m_hyp = 2"


# ---------------------------------------------------------------- the header, the module and the C ABI without a device

def test_module_restates_the_header_constants_and_refuses_the_cpu():
    import torch
    import xvector_amd
    from xvector_amd import der
    consts = header_constants("xvec_der.h", "XVEC_DER_")
    assert consts == {"MAX_SPEAKERS": der.MAX_SPEAKERS, "CHUNK_TICKS": der.CHUNK_TICKS, "WAVE_ROWS": der.WAVE_ROWS, "THREADS": der.THREADS}
    assert consts["MAX_SPEAKERS"] == 64 == der_ref.MAX_SPEAKERS and consts["CHUNK_TICKS"] == der_ref.CHUNK_TICKS
    exports = {"xvec_der_last_error", "xvec_der_workspace_bytes", "xvec_der_cooccurrence", "xvec_der_assign", "xvec_der_score"}
    assert exports <= set(xvector_amd.hip.EXPORTS) and all(hasattr(xvector_amd.hip.lib, n) for n in exports)
    turns = _t([0, 0, 5, 0])
    with pytest.raises(RuntimeError, match="HIP device only"):
        der.der(turns, turns, [10], device="cpu")
    with pytest.raises(RuntimeError, match="HIP device only"):
        der.assign(torch.zeros(64, 64, dtype=torch.int64))
    assert xvector_amd.der is der and xvector_amd.DerResult is der.DerResult and xvector_amd.read_rttm is der.read_rttm
    assert {"der", "DerResult", "read_rttm"} <= set(xvector_amd.__all__)
    assert der.DerResult._fields == ("scored", "total", "miss", "fa", "conf", "der", "overall", "mapping", "ignored", "cooccurrence")
    with pytest.raises(ValueError, match="rec_len"):
        der.workspace_bytes([10, 0])
    assert der.workspace_bytes([2 ** 30, 2 ** 30]) == 0 and der.workspace_bytes([10, 20]) % 256 == 0


def _start(*v):
    return (ctypes.c_int64 * len(v))(*v)


GOOD = dict(ref=P, m_ref=3, hyp=P, m_hyp=2, start=None, n_rec=2, collar=0, skip=0, counts=P, map=P, der=P, ignored=P, cooc=P, ws=P,
            ws_bytes=None)


def _need(hip):
    return hip.lib.xvec_der_workspace_bytes(_start(0, 4, 9), 2, 3, 2)


def _score(hip, **kw):
    a = {**GOOD, "start": _start(0, 4, 9), **kw}
    if a["ws_bytes"] is None:
        a["ws_bytes"] = _need(hip)
    return hip.lib.xvec_der_score(a["ref"], a["m_ref"], a["hyp"], a["m_hyp"], a["start"], a["n_rec"], a["collar"], a["skip"], a["counts"],
                                  a["map"], a["der"], a["ignored"], a["cooc"], a["ws"], a["ws_bytes"], None)


def _cooc(hip, **kw):
    a = {**GOOD, "start": _start(0, 4, 9), **kw}
    if a["ws_bytes"] is None:
        a["ws_bytes"] = _need(hip)
    return hip.lib.xvec_der_cooccurrence(a["ref"], a["m_ref"], a["hyp"], a["m_hyp"], a["start"], a["n_rec"], a["collar"], a["skip"],
                                         a["counts"], a["cooc"], a["ignored"], a["ws"], a["ws_bytes"], None)


def test_c_abi_argument_errors_return_before_any_device_call():
    from xvector_amd import hip
    lib, err = hip.lib, lambda: hip.lib.xvec_der_last_error().decode()
    shared = [
        (dict(n_rec=0), "n_rec = 0: need at least one recording"),
        (dict(start=None), "null pointer: rec_start"),
        (dict(start=_start(2, 4, 9)), "rec_start must begin at 0 (got 2)"),
        (dict(start=_start(0, 0, 9)), "recording 0 is empty or rec_start decreases: every recording needs a tick"),
        (dict(start=_start(0, 9, 4)), "recording 1 is empty or rec_start decreases: every recording needs a tick"),
        (dict(start=_start(0, 4, 2 ** 31)), f"{2 ** 31} ticks up to recording 1: the total must stay below 2^31"),
        (dict(m_ref=-1), "m_ref = -1 must not be negative"),
        (dict(m_hyp=-2), "m_hyp = -2 must not be negative"),
        (dict(collar=-1), "collar = -1 must not be negative"),
        (dict(ref=None), "null pointer: ref_turns with m_ref = 3"),
        (dict(hyp=None), "null pointer: hyp_turns with m_hyp = 2"),
    ]
    for kwargs, text in shared:
        for call in (_score, _cooc):
            assert call(hip, **kwargs) == hip.ERR_ARG and err() == text, kwargs
    for k in ("counts", "map", "der", "ignored"):
        assert _score(hip, **{k: None}) == hip.ERR_ARG and err() == "null pointer: counts / map / der / ignored"
    for k in ("counts", "cooc", "ignored"):
        assert _cooc(hip, **{k: None}) == hip.ERR_ARG and err() == "null pointer: counts / cooc / ignored"
    # an empty side may be a null pointer, and cooc is optional in the fused call: the next refusal is the workspace's
    assert _score(hip, ref=None, m_ref=0, hyp=None, m_hyp=0, cooc=None, ws=None) == hip.ERR_ARG and err() == "null pointer: workspace"
    # xvec_der_assign
    assert lib.xvec_der_assign(P, 0, P, P, None) == hip.ERR_ARG and err() == "n_rec = 0: need at least one recording"
    for args in ((None, 1, P, P), (P, 1, None, P), (P, 1, P, None)):
        assert lib.xvec_der_assign(*args, None) == hip.ERR_ARG and err() == "null pointer: cooc / map / correct"
    # the size query answers 0 for what the entry points refuse
    good = _start(0, 4, 9)
    for args in ((good, 0, 1, 1), (None, 2, 1, 1), (_start(1, 4, 9), 2, 1, 1), (_start(0, 4, 4), 2, 1, 1), (_start(0, 4, 2 ** 31), 2, 1, 1),
                 (good, 2, -1, 1), (good, 2, 1, -1), (good, 2, 2 ** 31, 1)):
        assert lib.xvec_der_workspace_bytes(*args) == 0
    assert lib.xvec_der_workspace_bytes(good, 2, 0, 0) == lib.xvec_der_workspace_bytes(good, 2, 1000, 1000) >= 2 * 9 * 8 + 2 * 64 * 64 * 8


def test_workspace_refusals_through_the_der_pairs():
    """Every (void*, _wsb_der) pair of the binding is this unit's and is held here: a null and a one-byte-short workspace."""
    from xvector_amd import hip
    C = ctypes
    takes = {n for n, (_, a) in hip._SIGS.items() if any(x is hip._wsb_der and a[i - 1] is C.c_void_p for i, x in enumerate(a))}
    assert takes == {"xvec_der_cooccurrence", "xvec_der_score"} and issubclass(hip._wsb_der, hip._wsb_vbx) and hip._wsb_der is not hip._wsb_vbx
    need = _need(hip)
    assert need % 256 == 0
    for call in (_score, _cooc):
        assert call(hip, ws=None) == hip.ERR_ARG and hip.lib.xvec_der_last_error().decode() == "null pointer: workspace"
        assert call(hip, ws_bytes=need - 1) == hip.ERR_WORKSPACE
        assert hip.lib.xvec_der_last_error().decode() == f"workspace too small: {need - 1} < {need} bytes"
        assert call(hip, ws_bytes=0) == hip.ERR_WORKSPACE


def test_der_error_channel_is_its_own():
    from xvector_amd import hip
    lib = hip.lib
    assert lib.xvec_ahc_cluster(P, 9, _start(0, 4, 9), 2, 0.0, -2, None, P, P, None, None, None, P, 1 << 20, None) == hip.ERR_ARG
    assert _score(hip, collar=-7) == hip.ERR_ARG
    assert lib.xvec_der_last_error().decode() == "collar = -7 must not be negative"
    assert lib.xvec_diar_last_error().decode() == "max_clusters = -2 must not be negative (0 = no limit)"
