"""DER scoring on the device (csrc/der.hip, include/xvec_der.h) against tests/der_ref.py, through the C ABI and the module.

Everything is integer arithmetic, and der is one fp64 division of two exact integers: every output is compared with ==
(der by its bits).  The map is held to what the header promises (injective, reaches the optimum that scipy finds, reports no
pair that never met), not to one of several optimal maps.  The cases live in der_ref.gpu_cases() / assign_cases();
tests/test_der.py checks on the CPU that the oracle handles each of them.  One oracle run per case is shared by the tests."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import der_ref
import score_support as ss

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = der_ref.gpu_cases()
ASSIGN = der_ref.assign_cases()
COUNTS = ("scored", "total", "miss", "fa", "conf")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _i64(v):
    return (ctypes.c_int64 * len(v))(*[int(x) for x in v])


@functools.lru_cache(maxsize=None)
def _ref(name):
    return der_ref.der(*CASES[name])


def _dev_turns(t):
    t = np.asarray(t, dtype=np.int64).reshape(-1, 4)
    return torch.from_numpy(t.astype(np.int32)).to(DEV) if len(t) else None


def _score(ref, hyp, rec_len, collar=0, skip_overlap=False, ws=None, fill_ws=None, want_cooc=True):
    """xvec_der_score on host turns: a dict of numpy arrays.  Outputs start from a pattern that no result has."""
    from xvector_amd import hip
    n_rec = len(rec_len)
    rd, hd = _dev_turns(ref), _dev_turns(hyp)
    m_ref, m_hyp = (0 if rd is None else rd.shape[0]), (0 if hd is None else hd.shape[0])
    rs = _i64(np.concatenate([[0], np.cumsum(rec_len)]))
    need = int(hip.lib.xvec_der_workspace_bytes(rs, n_rec, m_ref, m_hyp))
    assert need > 0 and need % 256 == 0
    if ws is None:
        wst = torch.empty(need, dtype=torch.uint8, device=DEV)
        if fill_ws is not None:
            wst.fill_(fill_ws)
        ws = wst.data_ptr()
    counts = torch.full((n_rec, 5), -7, dtype=torch.int64, device=DEV)
    mapping = torch.full((n_rec, 64), -7, dtype=torch.int32, device=DEV)
    rate = torch.full((n_rec + 1,), 7.5, dtype=torch.float64, device=DEV)
    ign = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    cooc = torch.full((n_rec, 64, 64), -7, dtype=torch.int64, device=DEV) if want_cooc else None
    before = [None if t is None else t.clone() for t in (rd, hd)]
    rc = hip.lib.xvec_der_score(None if rd is None else rd.data_ptr(), m_ref, None if hd is None else hd.data_ptr(), m_hyp, rs, n_rec,
                                collar, int(skip_overlap), counts.data_ptr(), mapping.data_ptr(), rate.data_ptr(), ign.data_ptr(),
                                None if cooc is None else cooc.data_ptr(), ws, need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_der_last_error()
    torch.cuda.synchronize()
    assert all(b is None or torch.equal(b, t) for b, t in zip(before, (rd, hd))), "the turns were written to"
    c = counts.cpu().numpy()
    out = {k: c[:, i] for i, k in enumerate(COUNTS)}
    out.update(map=mapping.cpu().numpy(), der=rate.cpu().numpy(), ignored=ign.cpu().numpy(), cooc=None if cooc is None else cooc.cpu().numpy())
    return out


def _assert_equals_oracle(got, want, what):
    for k in COUNTS + ("ignored", "cooc"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k] if k != "cooc" else None, want[k] if k != "cooc" else None)
    assert np.array_equal(_bits(got["der"]), _bits(want["der"])), (what, got["der"], want["der"])
    for r in range(len(want["total"])):
        der_ref.check_map(want["cooc"][r], got["map"][r], want["correct"][r])


def _same(a, b, what):
    for k in COUNTS + ("ignored", "cooc", "map"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert np.array_equal(_bits(a["der"]), _bits(b["der"])), what


# ---------------------------------------------------------------- the fused call against the oracle

@pytest.mark.parametrize("name", list(CASES))
def test_score_equals_the_oracle(name):
    ref, hyp, rec_len, collar, skip = CASES[name]
    got = _score(ref, hyp, rec_len, collar, skip)
    want = _ref(name)
    print(f"[der] {name}: scored {got['scored'].tolist()} total {got['total'].tolist()} miss {got['miss'].tolist()} fa {got['fa'].tolist()} "
          f"conf {got['conf'].tolist()} der {got['der'].tolist()} ignored {got['ignored'].tolist()}")
    _assert_equals_oracle(got, want, name)


def test_what_the_cases_are_there_for():
    got = _score(*CASES["empty_hypothesis"])
    assert np.array_equal(got["miss"], got["total"]) and got["total"].sum() > 0 and (got["map"] == -1).all()
    got = _score(*CASES["empty_reference"])
    assert np.isnan(got["der"]).all() and got["fa"].tolist() == [97, 20] and (got["map"] == -1).all()
    got = _score(*CASES["both_empty"])
    assert np.isnan(got["der"]).all() and got["scored"].tolist() == [7, 3] and not got["cooc"].any()
    got = _score(*CASES["one_pair_over_70000_ticks"])
    assert got["cooc"][0, 3, 7] == 70000 and got["cooc"].sum() == 70000 and got["map"][0, 3] == 7 and got["der"][0] == 0.0
    got = _score(*CASES["word_halves_sign_bit_and_all_64"])
    assert (got["cooc"][0] > 0).all()
    got = _score(*CASES["collar_swallows_a_recording"])
    assert got["scored"].tolist() == [0, 30] and np.isnan(got["der"]).all()


@pytest.mark.parametrize("collar", [0, 1, 7, 100000])
def test_collars_on_one_set_of_turns(collar):
    ref, hyp, rec_len, _, _ = CASES["collar_1"]
    _assert_equals_oracle(_score(ref, hyp, rec_len, collar), der_ref.der(ref, hyp, rec_len, collar), f"collar {collar}")


def test_cooccurrence_call_equals_the_fused_call():
    from xvector_amd import hip
    ref, hyp, rec_len, collar, skip = CASES["skip_overlap"]
    want = _ref("skip_overlap")
    n_rec = len(rec_len)
    rd, hd = _dev_turns(ref), _dev_turns(hyp)
    rs = _i64(np.concatenate([[0], np.cumsum(rec_len)]))
    need = int(hip.lib.xvec_der_workspace_bytes(rs, n_rec, len(ref), len(hyp)))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    counts = torch.full((n_rec, 4), -7, dtype=torch.int64, device=DEV)
    cooc = torch.full((n_rec, 64, 64), -7, dtype=torch.int64, device=DEV)
    ign = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    rc = hip.lib.xvec_der_cooccurrence(rd.data_ptr(), len(ref), hd.data_ptr(), len(hyp), rs, n_rec, collar, int(skip), counts.data_ptr(),
                                       cooc.data_ptr(), ign.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_der_last_error()
    c = counts.cpu().numpy()
    for i, k in enumerate(COUNTS[:4]):
        assert np.array_equal(c[:, i], want[k]), k
    assert np.array_equal(cooc.cpu().numpy(), want["cooc"]) and ign.cpu().tolist() == want["ignored"].tolist()


# ---------------------------------------------------------------- exactness

def test_each_recording_alone_equals_itself_in_the_batch_at_either_end():
    ref, hyp, rec_len, collar, skip = CASES["batch_of_eight"]
    batch = _score(ref, hyp, rec_len, collar, skip)
    _assert_equals_oracle(batch, _ref("batch_of_eight"), "batch")
    n = len(rec_len)

    def renumbered(t, order):                     # the batch with its recordings in another order
        new = np.empty(n, dtype=np.int64)
        new[np.asarray(order)] = np.arange(n)
        t = t.copy()
        t[:, 0] = new[t[:, 0]]
        return t

    rolled = list(range(1, n)) + [0]              # the first recording last ...
    back = [n - 1] + list(range(n - 1))           # ... and the last one first
    for order in (rolled, back, list(reversed(range(n)))):
        got = _score(renumbered(ref, order), renumbered(hyp, order), [rec_len[r] for r in order], collar, skip)
        for at, r in enumerate(order):
            for k in COUNTS + ("cooc", "map"):
                assert np.array_equal(got[k][at], batch[k][r]), (order, r, k)
            assert _bits(got["der"][at]) == _bits(batch["der"][r])
        assert _bits(got["der"][n]) == _bits(batch["der"][n])
    for r in range(n):
        alone = _score(der_ref.only_recording(ref, r), der_ref.only_recording(hyp, r), [rec_len[r]], collar, skip)
        for k in COUNTS + ("cooc", "map"):
            assert np.array_equal(alone[k][0], batch[k][r]), (r, k)
        assert _bits(alone["der"][0]) == _bits(batch["der"][r]) == _bits(alone["der"][1])


def test_two_runs_and_a_poisoned_workspace_give_the_same_bits():
    ref, hyp, rec_len, collar, skip = CASES["batch_of_eight"]
    a = _score(ref, hyp, rec_len, collar, skip)
    b = _score(ref, hyp, rec_len, collar, skip)
    c = _score(ref, hyp, rec_len, collar, skip, fill_ws=0xFF)
    _same(a, b, "two runs")
    _same(a, c, "a workspace of 0xFF bytes")
    d = _score(ref, hyp, rec_len, collar, skip, want_cooc=False)
    assert d["cooc"] is None and all(np.array_equal(a[k], d[k]) for k in COUNTS + ("map",))
    # the order of the turns cannot show
    rng = np.random.default_rng(3)
    _same(a, _score(ref[rng.permutation(len(ref))], hyp[rng.permutation(len(hyp))], rec_len, collar, skip), "turns in another order")


def test_inside_a_workspace_window_of_the_reported_size():
    from xvector_amd import hip
    ref, hyp, rec_len, collar, skip = CASES["lengths_and_chunk_edges"]
    need = int(hip.lib.xvec_der_workspace_bytes(_i64(np.concatenate([[0], np.cumsum(rec_len)])), len(rec_len), len(ref), len(hyp)))
    big, off = ss.window(need, DEV)                  # the window holds 0xFF bytes: nothing is read unwritten
    got = _score(ref, hyp, rec_len, 3, skip, ws=big.data_ptr() + off)
    assert ss.guards_intact(big, off, need)
    _assert_equals_oracle(got, der_ref.der(ref, hyp, rec_len, 3, skip), "window")


# ---------------------------------------------------------------- the solver alone

def _assign(mats):
    from xvector_amd import hip
    c = torch.from_numpy(np.ascontiguousarray(np.stack(mats), dtype=np.int64)).to(DEV)
    before = c.clone()
    mapping = torch.full((len(mats), 64), -7, dtype=torch.int32, device=DEV)
    correct = torch.full((len(mats),), -7, dtype=torch.int64, device=DEV)
    rc = hip.lib.xvec_der_assign(c.data_ptr(), len(mats), mapping.data_ptr(), correct.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_der_last_error()
    torch.cuda.synchronize()
    assert torch.equal(c, before)
    return mapping.cpu().numpy(), correct.cpu().numpy()


def test_assign_on_crafted_matrices():
    names = list(ASSIGN)
    mapping, correct = _assign([ASSIGN[k] for k in names])
    for k, m, c in zip(names, mapping, correct):
        want = der_ref.best_correct(ASSIGN[k])
        print(f"[der] assign {k}: correct {int(c)} (scipy {want}), {int((m >= 0).sum())} pairs")
        assert int(c) == want, k
        der_ref.check_map(ASSIGN[k], m, c)
    by = dict(zip(names, mapping))
    assert by["greedy_gives_5_optimum_8"][:2].tolist() == [1, 0] and (by["all_zeros"] == -1).all()
    assert sorted(by["all_entries_equal"].tolist()) == list(range(64))
    assert np.array_equal(by["permutation_times_2^31-1"], ASSIGN["permutation_times_2^31-1"].argmax(axis=1))
    assert by["path_through_every_row"].tolist() == list(range(1, 64)) + [0]
    assert (by["3_reference_x_7_hypothesis"] >= 0).sum() == 3 and (by["7_reference_x_3_hypothesis"] >= 0).sum() == 3
    # a pure function of the matrix: alone, in another place of the batch, and run again
    again, _ = _assign([ASSIGN[k] for k in reversed(names)])
    assert np.array_equal(again[::-1], mapping)
    for k in ("all_entries_equal", "random_full_range_a", "random_sparse"):
        alone, c1 = _assign([ASSIGN[k]])
        assert np.array_equal(alone[0], by[k]) and int(c1[0]) == int(correct[names.index(k)])


def test_assign_terminates_on_entries_outside_the_range_and_touches_no_other_recording():
    good = ASSIGN["random_sparse"]
    bad = np.full((64, 64), -1, dtype=np.int64)
    bad[::2] = np.iinfo(np.int64).min
    bad[5, 5] = np.iinfo(np.int64).max
    mapping, correct = _assign([good, bad, good])
    want = der_ref.best_correct(good)
    assert int(correct[0]) == int(correct[2]) == want and np.array_equal(mapping[0], mapping[2])
    der_ref.check_map(good, mapping[0], want)
    assert ((mapping[1] >= -1) & (mapping[1] < 64)).all()


# ---------------------------------------------------------------- the module

def test_module_call_equals_the_c_abi():
    from xvector_amd import der
    ref, hyp, rec_len, collar, skip = CASES["batch_of_eight"]
    want = _ref("batch_of_eight")
    ws = torch.empty(der.workspace_bytes(rec_len), dtype=torch.uint8, device=DEV)
    res = der.der(ref, hyp, rec_len, collar=collar, skip_overlap=skip, return_cooccurrence=True, workspace=ws)
    assert isinstance(res, der.DerResult) and res.ignored == (0, 0) and all(t.is_cuda for t in res[:8]) and res.cooccurrence.is_cuda
    got = dict(scored=res.scored, total=res.total, miss=res.miss, fa=res.fa, conf=res.conf, cooc=res.cooccurrence, map=res.mapping)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    got.update(der=np.concatenate([res.der.cpu().numpy(), [float(res.overall)]]), ignored=np.asarray(res.ignored))
    _assert_equals_oracle(got, want, "module")
    # any integer dtype, numpy or torch, on the host or the device
    for conv in (lambda t: t.astype(np.int16), lambda t: torch.from_numpy(t), lambda t: torch.from_numpy(t.astype(np.int32)).to(DEV)):
        small = der.der(conv(ref), conv(hyp), torch.tensor(rec_len), collar=collar)
        assert torch.equal(small.total, res.total) and torch.equal(small.conf, res.conf) and small.cooccurrence is None
    # strict
    ref, hyp, rec_len, collar, skip = CASES["invalid_turns_of_each_kind"]
    with pytest.raises(ValueError, match="6 reference and 6 hypothesis turns are invalid"):
        der.der(ref, hyp, rec_len, collar=collar)
    loose = der.der(ref, hyp, rec_len, collar=collar, strict=False)
    assert loose.ignored == (6, 6) and loose.miss.cpu().tolist() == _ref("invalid_turns_of_each_kind")["miss"].tolist()
    # values beyond int32 stay invalid or clipped, they do not wrap
    wide = np.array([[0, 0, 2 ** 40, 1], [2 ** 32, 0, 5, 0], [0, 0, 5, 2 ** 32]], dtype=np.int64)
    res = der.der(wide, wide[:1], [30], strict=False)
    assert res.ignored == (2, 0) and int(res.total[0]) == 30 and float(res.overall) == 0.0
    # empty sides
    res = der.der(np.zeros((0, 4), dtype=np.int64), hyp[:1], rec_len)
    assert torch.isnan(res.der).all() and torch.isnan(res.overall)
    with pytest.raises(ValueError, match="m, 4"):
        der.der(np.zeros((3, 3), dtype=np.int64), hyp, rec_len)
    with pytest.raises(ValueError, match="integers"):
        der.der(ref.astype(np.float64), hyp, rec_len)
    # assign
    mats = torch.from_numpy(np.stack([ASSIGN["greedy_gives_5_optimum_8"], ASSIGN["random_sparse"]])).to(DEV)
    mapping, correct = der.assign(mats)
    assert correct.cpu().tolist() == [8, der_ref.best_correct(ASSIGN["random_sparse"])] and mapping.shape == (2, 64)
    one_map, one = der.assign(mats[0].to(torch.int32))
    assert int(one) == 8 and torch.equal(one_map, mapping[0])


def test_turns_through_rttm_score_zero_against_themselves(tmp_path):
    from xvector_amd import der
    from xvector_amd.diarize import write_rttm
    t = np.array([[0, 0, 120, 0], [0, 100, 260, 1], [0, 260, 300, 0], [1, 5, 80, 0]], dtype=np.int64)
    path = str(tmp_path / "ref.rttm")
    write_rttm(t, ["a", "b"], path)
    back, names, _ = der.read_rttm(path)
    res = der.der(back, t, [300, 80], collar=25)
    assert names == ["a", "b"] and float(res.overall) == 0.0 and res.mapping[0, :2].cpu().tolist() == [0, 1]
    swapped = t.copy()
    swapped[:3, 3] = 1 - swapped[:3, 3]            # speaker names carry no meaning: the mapping undoes the swap
    res = der.der(back, swapped, [300, 80])
    assert float(res.overall) == 0.0 and res.mapping[0, :2].cpu().tolist() == [1, 0]
