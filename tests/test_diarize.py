"""CPU-only checks of diarization's clustering (include/xvec_diar.h): the numpy restatement tests/diar_ref.py against
scipy.cluster.hierarchy.linkage on planted-speaker scores, the host-only plan (csrc/diar_plan.h) through its dump program, the
C ABI's argument errors (each returns before the library touches a device), `turns` / `write_rttm` on hand-written cases and the
module's constants against the header.

The bound on a merge score, 4 n 2^-53 max|S|.  A merge score is a chain of at most n - 1 nested updates
(n_i s_ik + n_j s_jk) / (n_i + n_j) of cells of S.  The sizes are exact, so an update is a convex combination that rounds three
times at the scale of max|S| (the two products' errors are weighted by n_i / (n_i + n_j) and n_j / (n_i + n_j), which add to 1,
and count as one; the sum and the quotient round once each): 3 (n - 1) 2^-53 max|S| < 4 n 2^-53 max|S| at the deepest chain.
scipy evaluates the same expression per update, so the two sides agree far inside it: 4e-14 against 3e-11 at n = 513."""
import ctypes
import io

import numpy as np
import pytest

import diar_ref
from scipy.cluster import hierarchy
from hipcc_support import header_constants, host_program, needs_host_cxx

P = 0x1000          # a pointer that is never followed: every call here fails its argument checks first
INF, NAN = float("inf"), float("nan")


def _canonical(flat):
    """Labels renumbered in the order of first appearance."""
    _, first, inverse = np.unique(flat, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inverse.reshape(-1)]


# ---------------------------------------------------------------- the restatement against scipy

@pytest.mark.parametrize("n", [2, 3, 65, 200, 513])
def test_restatement_equals_scipy_average_linkage(n):
    S, _ = diar_ref.planted(n, speakers=4 + n % 2, seed=n)
    iu = np.triu_indices(n, 1)
    Z = hierarchy.linkage(-S[iu], "average")          # condensed distances in row-major upper-triangle order
    heights = -Z[:, 2]
    bound = 4 * n * 2.0 ** -53 * np.abs(S[iu]).max()
    labels, count, mi, mj, ms = diar_ref.ahc(S, threshold=-INF)
    assert count == 1 and (labels == 0).all() and (mi[:n - 1] >= 0).all() and (mi[:n - 1] < mj[:n - 1]).all()
    assert mi[n - 1] == -1 and mj[n - 1] == -1 and np.isnan(ms[n - 1])
    err = np.abs(np.sort(ms[:n - 1]) - np.sort(heights)).max()
    print(f"[diar] n = {n}: merge scores against scipy {err:.2e}, bound {bound:.2e}")
    assert err <= bound
    Zs = Z.copy()
    shift = Zs[:, 2].min()
    Zs[:, 2] -= shift                                 # fcluster refuses negative heights
    for k in (1, 2, 4):
        got = diar_ref.ahc(S, want=k)
        want = hierarchy.fcluster(Zs, t=k, criterion="maxclust")
        assert got[1] == min(k, n) == len(set(want.tolist()))
        assert np.array_equal(got[0], _canonical(want)), (n, k)
        assert (got[2] >= 0).sum() == n - got[1]
    # thresholds: above every height, below every height, and in the middle of the widest gap between two
    # heights; each further than the bound from every height
    h = np.sort(heights)
    thresholds = [h[-1] + 1.0, h[0] - 1.0]
    if n > 2:
        gap = int(np.argmax(np.diff(h)))
        thresholds.append(0.5 * (h[gap] + h[gap + 1]))
    for thr in thresholds:
        assert np.abs(heights - thr).min() > bound, (n, thr)
        got = diar_ref.ahc(S, threshold=thr)
        want = hierarchy.fcluster(Zs, t=-thr - shift, criterion="distance")
        assert np.array_equal(got[0], _canonical(want)), (n, thr)
        assert got[1] == 1 + int((heights < thr).sum())


def test_restatement_rules_on_hand_written_blocks():
    # ties: an all-equal block merges in index order, (0, 1), (0, 2), ...
    out = diar_ref.ahc(np.full((5, 5), 2.5), threshold=-INF)
    assert out[2].tolist() == [0, 0, 0, 0, -1] and out[3].tolist() == [1, 2, 3, 4, -1] and (out[4][:4] == 2.5).all()
    # only the upper triangle is read; -0.0 ties with +0.0 (the lower pair wins), NaN is never selected
    S = np.array([[NAN, -0.0, NAN, -1.0],
                  [9.0, NAN, 0.0, NAN],
                  [9.0, 9.0, NAN, NAN],
                  [9.0, 9.0, 9.0, NAN]])
    labels, count, mi, mj, ms = diar_ref.ahc(S, threshold=-INF)
    assert (mi[0], mj[0]) == (0, 1) and np.signbit(ms[0])
    # (0,1) merged: s(0,2) = (NaN + 0.0) / 2 = NaN, s(0,3) = (-1 + NaN) / 2 = NaN, s(2,3) = NaN: nothing selectable is left
    assert count == 3 and labels.tolist() == [0, 0, 1, 2] and mi[1] == -1
    # the stop rules
    S, _ = diar_ref.planted(12, 2, seed=3)
    assert diar_ref.ahc(S, threshold=INF)[1] == 12 and diar_ref.ahc(S, threshold=INF, max_clusters=5)[1] == 5
    assert diar_ref.ahc(S, want=12)[1] == 12 and diar_ref.ahc(S, want=40)[1] == 12 and diar_ref.ahc(S, want=1)[1] == 1
    assert diar_ref.ahc(S, threshold=-INF, want=3)[1] == 3         # a wanted count overrides the threshold
    inf_block = np.full((3, 3), -INF)
    assert diar_ref.ahc(inf_block, threshold=-INF)[1] == 1 and diar_ref.ahc(inf_block, threshold=-1e300)[1] == 3


# ---------------------------------------------------------------- the host-only plan

@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return host_program("diar_plan_dump", tmp_path_factory.mktemp("diar_plan"))


@needs_host_cxx
def test_plan_layout_is_aligned_dense_and_what_the_library_reports(plan):
    from xvector_amd import hip
    for counts in ([1], [2], [37] * 64, [3, 64, 1, 65, 300, 1], [2048], [5, 6, 7]):
        v = [int(x) for x in plan(["layout " + " ".join(map(str, counts))])[0].split()[1:]]
        rec_start, want, mat_off, best_v, best_i, mats, total = v[:7]
        offs = v[7:]
        n_rec, N = len(counts), sum(counts)
        assert all(o % 256 == 0 for o in v), counts
        assert rec_start == 0 and want >= 8 * (n_rec + 1) and mat_off >= want + 4 * n_rec and best_v >= mat_off + 8 * n_rec
        assert best_i >= best_v + 8 * N and mats >= best_i + 4 * N and offs[0] == mats
        for r, n in enumerate(counts):                # each matrix holds n * n doubles before the next starts
            end = offs[r + 1] if r + 1 < n_rec else total
            assert 0 <= end - offs[r] - 8 * n * n < 256, (counts, r)
        rs = (ctypes.c_int64 * (n_rec + 1))(*np.concatenate([[0], np.cumsum(counts)]).tolist())
        assert hip.lib.xvec_ahc_workspace_bytes(rs, n_rec) == total


@needs_host_cxx
def test_plan_refusals_block_sizes_and_groups(plan):
    from xvector_amd import diarize
    small, large, cap = diarize.THREADS_SMALL, diarize.THREADS_LARGE, diarize.MAX_SEGMENTS
    got = plan(["check 3 1 4", f"check {cap}", f"check 3 {cap + 1}", "check 3 0 4", "start 1 4", "start 0 4 3 9", "start 0",
                "check" + " 2048" * (2 ** 20 + 1),
                "want 0 1 5", "want 2 -1", f"threads 1", f"threads {small}", f"threads {small + 1}", f"threads {cap}",
                "groups 3 4 5", "groups 300 400", f"groups 1 {small + 1} {small} 500 2 9 1", f"groups 100 7 8 300"])
    assert got[:3] == ["ok", "ok", f"refused recording 1 has {cap + 1} segments, more than XVEC_DIAR_MAX_SEGMENTS = {cap}"]
    assert got[3] == "refused recording 1 is empty or rec_start decreases: every recording needs a segment"
    assert got[4] == "refused rec_start must begin at 0 (got 1)"
    assert got[5] == "refused recording 1 is empty or rec_start decreases: every recording needs a segment"
    assert got[6] == "refused n_rec = 0: need at least one recording"
    assert got[7] == f"refused {2 ** 31} segments up to recording {2 ** 20 - 1}: the total must stay below 2^31"
    assert got[8:10] == ["ok", "refused want[1] = -1 must not be negative (0 = stop by threshold)"]
    assert got[10:14] == [f"threads {small}", f"threads {small}", f"threads {large}", f"threads {large}"]
    assert got[14] == f"groups 0 3 {small}" and got[15] == f"groups 0 2 {large}"
    assert got[16] == f"groups 0 7 {small} 1 3 {large}"          # the hulls: small 0 .. 6, large 1 .. 3
    assert got[17] == f"groups 1 2 {small} 0 4 {large}"


# ---------------------------------------------------------------- the header, the module and the C ABI without a device

def test_module_restates_the_header_constants_and_refuses_the_cpu():
    import torch
    import xvector_amd
    from xvector_amd import diarize
    consts = header_constants("xvec_diar.h", "XVEC_DIAR_")
    assert consts == {"MAX_SEGMENTS": diarize.MAX_SEGMENTS, "THREADS_SMALL": diarize.THREADS_SMALL,
                      "THREADS_LARGE": diarize.THREADS_LARGE, "RESCAN_WIDTH": diarize.RESCAN_WIDTH}
    assert diarize.MAX_SEGMENTS >= 2048 and diarize.THREADS_SMALL == diarize.RESCAN_WIDTH == 64
    with pytest.raises(RuntimeError, match="HIP device only"):
        diarize.cluster(torch.zeros(4, 4, dtype=torch.float64), [0, 4], threshold=0.0)
    with pytest.raises(RuntimeError, match="HIP device only"):
        diarize.Diarizer(None, "cosine", threshold=0.0, device="cpu")
    assert xvector_amd.Diarizer is diarize.Diarizer and xvector_amd.cluster is diarize.cluster
    assert xvector_amd.turns is diarize.turns and xvector_amd.write_rttm is diarize.write_rttm
    assert {"xvec_diar_last_error", "xvec_ahc_workspace_bytes", "xvec_ahc_cluster"} <= set(xvector_amd.hip.EXPORTS)


def _start(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _want(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_c_abi_argument_errors_return_before_any_device_call():
    from xvector_amd import hip
    lib, err = hip.lib, lambda: hip.lib.xvec_diar_last_error().decode()
    good = dict(S=P, ld=9, start=_start(0, 4, 9), n_rec=2, thr=0.0, maxc=0, want=None, labels=P, counts=P, mi=None, mj=None,
                ms=None, ws=P, ws_bytes=None)

    def call(**kw):
        a = {**good, **kw}
        if a["ws_bytes"] is None:
            a["ws_bytes"] = lib.xvec_ahc_workspace_bytes(a["start"], a["n_rec"])
        return lib.xvec_ahc_cluster(*[a[k] for k in ("S", "ld", "start", "n_rec", "thr", "maxc", "want", "labels", "counts", "mi",
                                                     "mj", "ms", "ws", "ws_bytes")], None)

    need = lib.xvec_ahc_workspace_bytes(good["start"], 2)
    assert need % 256 == 0 and need >= 8 * (16 + 25) + 12 * 9 + 8 * 3 + 4 * 2 + 8 * 2
    cases = [
        (dict(n_rec=0), hip.ERR_ARG, "n_rec = 0: need at least one recording"),
        (dict(n_rec=-3), hip.ERR_ARG, "n_rec = -3: need at least one recording"),
        (dict(start=None), hip.ERR_ARG, "null pointer: rec_start"),
        (dict(start=_start(2, 4, 9)), hip.ERR_ARG, "rec_start must begin at 0 (got 2)"),
        (dict(start=_start(0, 0, 9)), hip.ERR_ARG, "recording 0 is empty or rec_start decreases: every recording needs a segment"),
        (dict(start=_start(0, 9, 4)), hip.ERR_ARG, "recording 1 is empty or rec_start decreases: every recording needs a segment"),
        (dict(start=_start(0, 4, 2053), ld=4000), hip.ERR_ARG, "recording 1 has 2049 segments, more than XVEC_DIAR_MAX_SEGMENTS = 2048"),
        (dict(thr=NAN), hip.ERR_ARG, "threshold is NaN (+inf never merges by score, -inf always)"),
        (dict(maxc=-1), hip.ERR_ARG, "max_clusters = -1 must not be negative (0 = no limit)"),
        (dict(want=_want(2, -7)), hip.ERR_ARG, "want[1] = -7 must not be negative (0 = stop by threshold)"),
        (dict(ld=8), hip.ERR_ARG, "ld = 8 is smaller than the 9 segments"),
        (dict(S=None), hip.ERR_ARG, "null pointer: S / labels / n_clusters"),
        (dict(labels=None), hip.ERR_ARG, "null pointer: S / labels / n_clusters"),
        (dict(counts=None), hip.ERR_ARG, "null pointer: S / labels / n_clusters"),
        (dict(mi=P), hip.ERR_ARG, "merge_i, merge_j and merge_score: all three or none"),
        (dict(mi=P, mj=P), hip.ERR_ARG, "merge_i, merge_j and merge_score: all three or none"),
        (dict(ms=P), hip.ERR_ARG, "merge_i, merge_j and merge_score: all three or none"),
        (dict(ws=None), hip.ERR_ARG, "null pointer: workspace"),
        (dict(ws_bytes=need - 1), hip.ERR_WORKSPACE, f"workspace too small: {need - 1} < {need} bytes"),
    ]
    for kwargs, code, text in cases:
        assert call(**kwargs) == code, kwargs
        assert err() == text, kwargs
    # the size query answers 0 for what the entry point refuses
    for start, n_rec in ((good["start"], 0), (None, 2), (_start(1, 4, 9), 2), (_start(0, 0, 9), 2), (_start(0, 4, 2053), 2)):
        assert lib.xvec_ahc_workspace_bytes(start, n_rec) == 0
    assert lib.xvec_ahc_workspace_bytes(_start(0, 2048), 1) >= 8 * 2048 * 2048


def test_diar_error_channel_is_its_own():
    from xvector_amd import hip
    lib = hip.lib
    assert lib.xvec_identify_topk(P, 8, 4, 8, 99, 0.0, P, P, None, P, 4096, None) == hip.ERR_ARG
    assert lib.xvec_ahc_cluster(P, 9, _start(0, 4, 9), 2, 0.0, -2, None, P, P, None, None, None, P, 1 << 20, None) == hip.ERR_ARG
    assert lib.xvec_diar_last_error().decode() == "max_clusters = -2 must not be negative (0 = no limit)"
    assert lib.xvec_ident_last_error().decode() == "k = 99 must lie in 1 .. 16"


def test_cluster_refuses_bad_arguments_before_the_device():
    import torch
    from xvector_amd import diarize
    with pytest.raises(ValueError, match="rec_start must rise"):
        diarize._rec_start([0, 3, 3, 5], 5, "cluster")
    with pytest.raises(ValueError, match="rec_start must rise"):
        diarize._rec_start([0, 4], 5, "cluster")
    assert diarize._rec_start([0, 2, 5], 5, "cluster").dtype == np.int64
    with pytest.raises(RuntimeError, match="no CPU path"):
        diarize._matrix(torch.zeros(3, 3, dtype=torch.float64), "cluster")


# ---------------------------------------------------------------- turns and RTTM

def test_turns_split_overlaps_leave_gaps_and_merge_equal_labels():
    from xvector_amd.diarize import turns
    # overlap split: [0, 100) and [50, 150) share [50, 100): cut at (50 + 0 + 100) // 2 = 75
    assert turns([(0, 0, 100), (0, 50, 100)], [0, 1]).tolist() == [[0, 0, 75, 0], [0, 75, 150, 1]]
    # an odd overlap rounds down: [0, 15) and [10, 25): (10 + 0 + 15) // 2 = 12
    assert turns([(0, 0, 15), (0, 10, 15)], [1, 0]).tolist() == [[0, 0, 12, 1], [0, 12, 25, 0]]
    # equal labels merge over the cut; a change of speaker and back gives three turns
    w = [(0, 0, 100), (0, 50, 100), (0, 100, 100), (0, 150, 100)]
    assert turns(w, [0, 0, 0, 0]).tolist() == [[0, 0, 250, 0]]
    assert turns(w, [0, 1, 1, 0]).tolist() == [[0, 0, 75, 0], [0, 75, 175, 1], [0, 175, 250, 0]]
    # a gap belongs to nobody, also between equal labels; windows that touch merge
    assert turns([(0, 0, 100), (0, 120, 100)], [2, 2]).tolist() == [[0, 0, 100, 2], [0, 120, 220, 2]]
    assert turns([(0, 0, 100), (0, 100, 100)], [2, 2]).tolist() == [[0, 0, 200, 2]]
    # a single window; two recordings never merge, and recording 1 starts again at its own frames
    assert turns([(3, 40, 60)], [0]).tolist() == [[3, 40, 100, 0]]
    two = turns(np.array([(0, 0, 100), (0, 50, 100), (1, 0, 100), (1, 50, 80)], dtype=np.int32), np.array([0, 0, 0, 1], dtype=np.int32))
    assert two.dtype == np.int64 and two.tolist() == [[0, 0, 150, 0], [1, 0, 75, 0], [1, 75, 130, 1]]
    assert turns(np.zeros((0, 3), dtype=np.int32), []).shape == (0, 4)
    with pytest.raises(ValueError, match="grouped by recording"):
        turns([(1, 0, 100), (0, 0, 100)], [0, 0])
    with pytest.raises(ValueError, match="grouped by recording"):
        turns([(0, 50, 100), (0, 0, 100)], [0, 0])
    with pytest.raises(ValueError, match="labels"):
        turns([(0, 0, 100)], [0, 1])


def test_write_rttm_lines(tmp_path):
    from xvector_amd.diarize import write_rttm
    t = np.array([[0, 0, 75, 0], [0, 75, 175, 1], [1, 12, 1345, 0]])
    want = ("SPEAKER recA 1 0.000 0.750 <NA> <NA> spk0 <NA> <NA>\n"
            "SPEAKER recA 1 0.750 1.000 <NA> <NA> spk1 <NA> <NA>\n"
            "SPEAKER recB 1 0.120 13.330 <NA> <NA> spk0 <NA> <NA>\n")
    buf = io.StringIO()
    write_rttm(t, ["recA", "recB"], buf)
    assert buf.getvalue() == want
    path = str(tmp_path / "out.rttm")
    write_rttm(t, {0: "recA", 1: "recB"}, path)
    assert open(path).read() == want
    buf = io.StringIO()
    write_rttm(t[:1], ["r"], buf, frame_shift=0.0125)
    assert buf.getvalue() == "SPEAKER r 1 0.000 0.938 <NA> <NA> spk0 <NA> <NA>\n"


def test_diarizer_groups_recordings_into_calls():
    from xvector_amd.diarize import Diarizer
    d = Diarizer.__new__(Diarizer)
    d.max_score_rows = 100
    rs = lambda counts: np.concatenate([[0], np.cumsum(counts)])
    assert d.calls(rs([30, 30, 30, 30])) == [(0, 3), (3, 4)]
    assert d.calls(rs([100])) == [(0, 1)] and d.calls(rs([50, 50])) == [(0, 2)] and d.calls(rs([50, 51])) == [(0, 1), (1, 2)]
    assert d.calls(rs([300, 10, 10, 200, 1])) == [(0, 1), (1, 3), (3, 4), (4, 5)]      # a recording over the bound is its own call
