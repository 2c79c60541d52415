"""Average-linkage clustering on the device (csrc/diar.hip, include/xvec_diar.h) against tests/diar_ref.py, through the C ABI.
Labels, cluster counts and the (i, j) of every merge must be EQUAL and the merge scores bit-equal: the update is four separately
rounded operations on both sides, and the tie and NaN rules leave no choice.  Segment counts sit around the exported block
sizes (a single wave up to THREADS_SMALL segments, THREADS_LARGE threads beyond, a row walked in strides of either) and the
rescan width."""
import ctypes

import numpy as np
import pytest
import torch

import diar_ref
import score_support as ss

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
SMALL, LARGE = 64, 256          # tests/test_diarize.py ties xvector_amd.diarize's copies to the header
SIZES = [1, 2, 3, SMALL - 1, SMALL, SMALL + 1, LARGE - 1, LARGE, LARGE + 1, 2 * LARGE + 1]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _i64(v):
    return (ctypes.c_int64 * len(v))(*[int(x) for x in v])


def _i32(v):
    return (ctypes.c_int32 * len(v))(*[int(x) for x in v])


def _starts(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _call(S, rec_start, threshold=INF, max_clusters=0, want=None, merges=True, ld=None, ws=None):
    """xvec_ahc_cluster on the device matrix S (a tensor whose row stride is `ld`): (labels, n_clusters, merge_i, merge_j,
    merge_score) as numpy arrays (the last three None without `merges`)."""
    from xvector_amd import hip
    n_rec, N = len(rec_start) - 1, int(rec_start[-1])
    rs = _i64(rec_start)
    need = int(hip.lib.xvec_ahc_workspace_bytes(rs, n_rec))
    assert need > 0 and need % 256 == 0
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        ws_ptr = ws.data_ptr()
    else:
        ws_ptr = ws
    labels = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((n_rec,), -7, dtype=torch.int32, device=DEV)
    mi = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    mj = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    ms = torch.full((N,), 7.5, dtype=torch.float64, device=DEV)
    w = None if want is None else _i32(want)
    rc = hip.lib.xvec_ahc_cluster(S.data_ptr(), S.stride(0) if ld is None else ld, rs, n_rec, threshold, max_clusters, w,
                                  labels.data_ptr(), counts.data_ptr(), *([m.data_ptr() for m in (mi, mj, ms)] if merges else [None] * 3),
                                  ws_ptr, need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_diar_last_error()
    torch.cuda.synchronize()
    out = [labels.cpu().numpy(), counts.cpu().numpy()]
    return (*out, mi.cpu().numpy(), mj.cpu().numpy(), ms.cpu().numpy()) if merges else (*out, None, None, None)


def _assert_same(got, ref, what):
    assert np.array_equal(got[0], ref[0]), (what, "labels")
    assert np.array_equal(got[1], ref[1]), (what, "n_clusters", got[1], ref[1])
    assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]), (what, "merge pairs")
    done = ref[2] >= 0
    assert np.isnan(got[4][~done]).all() and np.array_equal(_bits(got[4][done]), _bits(ref[4][done])), (what, "merge scores")


_PLANTED = {}


def _planted(n):
    """(host scores, device scores, the full merge list of the reference) of a planted-speaker block, computed once."""
    if n not in _PLANTED:
        S, _ = diar_ref.planted(n, speakers=4 + n % 2, seed=1000 + n)
        _PLANTED[n] = (S, torch.from_numpy(S).to(DEV), diar_ref.ahc_batch(S, [0, n], threshold=-INF))
    return _PLANTED[n]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


# ---------------------------------------------------------------- segment counts

@pytest.mark.parametrize("n", SIZES)
def test_one_recording_equals_the_reference_at_every_size(n):
    host, dev, full = _planted(n)
    before = dev.clone()
    got = _call(dev, [0, n], threshold=-INF)
    _assert_same(got, full, f"n = {n}, everything merges")
    assert got[1][0] == 1 and (got[2][:n - 1] >= 0).all() and got[2][n - 1] == -1 and got[3][n - 1] == -1 and np.isnan(got[4][n - 1])
    again = _call(dev, [0, n], threshold=-INF)                      # run to run
    _assert_same(again, got, f"n = {n}, second run")
    assert torch.equal(dev, before)                                 # S is not modified
    if n > 1:
        thr = float(np.median(full[4][:n - 1]))                     # a merge score itself: best >= threshold still merges
        ref = diar_ref.ahc_batch(host, [0, n], threshold=thr)
        assert ref[1][0] <= (n + 1) // 2 + 1
        _assert_same(_call(dev, [0, n], threshold=thr), ref, f"n = {n}, threshold {thr}")
    only = _call(dev, [0, n], threshold=-INF, merges=False)         # without the merge outputs
    assert np.array_equal(only[0], full[0]) and np.array_equal(only[1], full[1])


# ---------------------------------------------------------------- batching and layout

BATCH = [5, SMALL, 1, SMALL + 1, 300, 37, 1]          # both block sizes mixed; a single segment in the middle and at the end


def test_batch_with_a_row_stride_an_odd_base_and_nan_around_the_blocks():
    rs = _starts(BATCH)
    N = int(rs[-1])
    ld = N + 3
    buf = torch.full((N * ld + 2,), NAN, dtype=torch.float64, device=DEV)
    off = 1 if buf.data_ptr() % 16 == 0 else 0
    S = buf[off:off + N * ld].view(N, ld)
    assert S.data_ptr() % 16 == 8                    # 8 bytes is all that is asked
    blocks = []
    for r, n in enumerate(BATCH):
        host = diar_ref.planted(n, 3, seed=50 + r)[0]
        blocks.append(host)
        a = int(rs[r])
        S[a:a + n, a:a + n] = torch.triu(_dev(host), 1) + torch.tril(torch.full((n, n), NAN, dtype=torch.float64, device=DEV))
    # (everything but the cells above the diagonal inside a block is NaN now: the diagonal, the lower triangle, the rest)
    want = [0, 2, 0, 0, 3, 0, 5]
    thr = 2.0
    ref = [diar_ref.ahc_batch(b, [0, b.shape[0]], threshold=thr, want=[w]) for b, w in zip(blocks, want)]
    cat = lambda k: np.concatenate([x[k] for x in ref])
    ref_all = (cat(0), cat(1), cat(2), cat(3), cat(4))
    got = _call(S, rs, threshold=thr, want=want, ld=ld)
    _assert_same(got, ref_all, "batch")
    assert got[1][2] == 1 and got[1][6] == 1 and got[2][rs[2]] == -1 and got[2][rs[6]] == -1      # the single segments
    # every recording alone (dense, 16-byte aligned, finite values around the triangle) gives the same bits
    for r, (b, w) in enumerate(zip(blocks, want)):
        alone = _call(_dev(b), [0, b.shape[0]], threshold=thr, want=[w])
        a, e = int(rs[r]), int(rs[r + 1])
        _assert_same(alone, tuple(x[r:r + 1] if k == 1 else x[a:e] for k, x in enumerate(got)), f"recording {r} alone")
    # and in another place of another batch
    order = [4, 0, 6, 3]
    rs2 = _starts([BATCH[r] for r in order])
    S2 = torch.zeros((int(rs2[-1]), int(rs2[-1])), dtype=torch.float64, device=DEV)
    for q, r in enumerate(order):
        a = int(rs2[q])
        S2[a:a + BATCH[r], a:a + BATCH[r]] = _dev(blocks[r])
    got2 = _call(S2, rs2, threshold=thr, want=[want[r] for r in order])
    for q, r in enumerate(order):
        a, e, a2, e2 = int(rs[r]), int(rs[r + 1]), int(rs2[q]), int(rs2[q + 1])
        _assert_same(tuple(x[q:q + 1] if k == 1 else x[a2:e2] for k, x in enumerate(got2)),
                     tuple(x[r:r + 1] if k == 1 else x[a:e] for k, x in enumerate(got)), f"recording {r} moved")


# ---------------------------------------------------------------- score values

@pytest.mark.parametrize("n", [5, SMALL + 6, LARGE + 3])
def test_exact_ties_merge_in_index_order(n):
    got = _call(_dev(np.full((n, n), 2.5)), [0, n], threshold=-INF)
    assert got[2][:n - 1].tolist() == [0] * (n - 1) and got[3][:n - 1].tolist() == list(range(1, n))
    assert (got[4][:n - 1] == 2.5).all() and (got[0] == 0).all()
    # duplicated rows: small integer vectors, every second one a copy of its predecessor, so that products and sums are exact
    x = np.random.default_rng(n).integers(-3, 4, (n, 6)).astype(np.float64)
    x[1::2] = x[0:n - 1:2][: x[1::2].shape[0]]
    S = x @ x.T
    for kw in (dict(threshold=-INF), dict(threshold=float(np.median(S))), dict(want=[3])):
        _assert_same(_call(_dev(S), [0, n], **kw), diar_ref.ahc_batch(S, [0, n], **kw), f"duplicates n = {n} {kw}")
    zeros = np.where(np.random.default_rng(1).random((n, n)) < 0.5, -0.0, 0.0)       # the two zeros tie
    _assert_same(_call(_dev(zeros), [0, n], threshold=0.0), diar_ref.ahc_batch(zeros, [0, n], threshold=0.0), "zeros")


@pytest.mark.parametrize("n", [7, SMALL + 1, LARGE + 45])
def test_nan_inf_and_large_cells(n):
    rng = np.random.default_rng(n)
    base = diar_ref.planted(n, 3, seed=n)[0]
    # NaN cells inside the upper triangle: never selected, and they spread by the update until only NaN pairs remain
    S = base.copy()
    S[rng.random((n, n)) < 0.02] = NAN
    ref = diar_ref.ahc_batch(S, [0, n], threshold=-INF)
    got = _call(_dev(S), [0, n], threshold=-INF)
    _assert_same(got, ref, f"NaN cells n = {n}")
    # two groups with nothing but NaN between them: the merging stops at two clusters whatever the threshold
    half = n // 2
    S = base.copy()
    S[:half, half:] = NAN
    got = _call(_dev(S), [0, n], threshold=-INF)
    _assert_same(got, diar_ref.ahc_batch(S, [0, n], threshold=-INF), f"NaN wall n = {n}")
    assert got[1][0] == 2 and got[0].tolist() == [0] * half + [1] * (n - half) and (got[2] >= 0).sum() == n - 2
    allnan = _call(_dev(np.full((n, n), NAN)), [0, n], threshold=-INF)
    assert allnan[1][0] == n and allnan[0].tolist() == list(range(n)) and (allnan[2] == -1).all() and np.isnan(allnan[4]).all()
    # +-inf are ordinary values (inf - inf in an update gives a NaN cell), +-900 are nothing special
    S = base.copy()
    pick = rng.random((n, n))
    S[pick < 0.03] = INF
    S[(pick >= 0.03) & (pick < 0.06)] = -INF
    S[(pick >= 0.06) & (pick < 0.12)] = 900.0
    S[(pick >= 0.12) & (pick < 0.18)] = -900.0
    for thr in (-INF, 0.0, INF):
        _assert_same(_call(_dev(S), [0, n], threshold=thr), diar_ref.ahc_batch(S, [0, n], threshold=thr), f"inf cells n = {n}, {thr}")
    S = np.full((n, n), -INF)
    assert _call(_dev(S), [0, n], threshold=-INF)[1][0] == 1 and _call(_dev(S), [0, n], threshold=-1e300)[1][0] == n


# ---------------------------------------------------------------- the stop rule

def test_stop_rules():
    counts = [SMALL - 4, SMALL + 9, 12, LARGE + 1]
    rs = _starts(counts)
    N = int(rs[-1])
    S = np.zeros((N, N))
    for r, n in enumerate(counts):
        S[rs[r]:rs[r + 1], rs[r]:rs[r + 1]] = diar_ref.planted(n, 4, seed=70 + r)[0]
    dev = _dev(S)
    nothing = _call(dev, rs, threshold=INF)
    assert nothing[1].tolist() == counts and (nothing[2] == -1).all() and np.isnan(nothing[4]).all()
    assert nothing[0].tolist() == [s for n in counts for s in range(n)]
    everything = _call(dev, rs, threshold=-INF)
    assert everything[1].tolist() == [1] * 4 and (everything[0] == 0).all()
    for kw in (dict(threshold=INF, want=[1, counts[1], counts[2] + 5, 2]),          # want at 1, at n_r, above n_r
               dict(threshold=-INF, want=[0, 7, 0, counts[3]]),                     # 0: the threshold decides
               dict(threshold=INF, max_clusters=9),                                 # merges below the threshold, down to 9
               dict(threshold=6.0, max_clusters=3),
               dict(threshold=6.0, max_clusters=3, want=[0, 0, 5, 1]),
               dict(threshold=6.0)):
        ref = diar_ref.ahc_batch(S, rs, **kw)
        _assert_same(_call(dev, rs, **kw), ref, str(kw))
    assert _call(dev, rs, threshold=INF, want=[1, counts[1], counts[2] + 5, 2])[1].tolist() == [1, counts[1], counts[2], 2]
    assert _call(dev, rs, threshold=INF, max_clusters=9)[1].tolist() == [9] * 4
    by_score = _call(dev, rs, threshold=6.0)[1]
    assert (by_score > 3).any()                      # ... so that max_clusters = 3 forced merges under the threshold above
    assert (_call(dev, rs, threshold=6.0, max_clusters=3)[1] <= 3).all()


# ---------------------------------------------------------------- resources

def test_inside_a_workspace_window_of_the_reported_size():
    from xvector_amd import hip
    rs = _starts(BATCH)
    N = int(rs[-1])
    S = np.zeros((N, N))
    for r, n in enumerate(BATCH):
        S[rs[r]:rs[r + 1], rs[r]:rs[r + 1]] = diar_ref.planted(n, 3, seed=50 + r)[0]
    need = int(hip.lib.xvec_ahc_workspace_bytes(_i64(rs), len(BATCH)))
    assert need >= 8 * sum(n * n for n in BATCH) + 12 * N
    big, off = ss.window(need, DEV)                  # the window holds 0xFF bytes (NaN as float64): nothing is read unwritten
    got = _call(_dev(S), rs, threshold=1.0, ws=big.data_ptr() + off)
    assert ss.guards_intact(big, off, need)
    _assert_same(got, diar_ref.ahc_batch(S, rs, threshold=1.0), "window")


def test_runs_under_graph_capture():
    from xvector_amd import hip
    counts = [40, SMALL + 30, 1]
    rs_np = _starts(counts)
    N = int(rs_np[-1])
    hosts = []
    for seed in (1, 2):
        S = np.zeros((N, N))
        for r, n in enumerate(counts):
            S[rs_np[r]:rs_np[r + 1], rs_np[r]:rs_np[r + 1]] = diar_ref.planted(n, 3, seed=10 * seed + r)[0]
        hosts.append(S)
    rs, want = _i64(rs_np), _i32([0, 3, 0])          # host arrays the graph reads at every replay: kept alive to the end
    need = int(hip.lib.xvec_ahc_workspace_bytes(rs, len(counts)))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    static = _dev(hosts[0])
    labels = torch.zeros(N, dtype=torch.int32, device=DEV)
    n_clusters = torch.zeros(len(counts), dtype=torch.int32, device=DEV)
    mi, mj = torch.zeros(N, dtype=torch.int32, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
    ms = torch.zeros(N, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = hip.lib.xvec_ahc_cluster(static.data_ptr(), N, rs, len(counts), 1.5, 0, want, labels.data_ptr(), n_clusters.data_ptr(),
                                      mi.data_ptr(), mj.data_ptr(), ms.data_ptr(), ws.data_ptr(), need,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_diar_last_error()
    for S in hosts:
        static.copy_(_dev(S))
        g.replay()
        torch.cuda.synchronize()
        got = tuple(t.cpu().numpy() for t in (labels, n_clusters, mi, mj, ms))
        _assert_same(got, diar_ref.ahc_batch(S, rs_np, threshold=1.5, want=[0, 3, 0]), "replay")


# ---------------------------------------------------------------- the module and the chain

def test_cluster_module_call_equals_the_abi():
    from xvector_amd import diarize
    host, dev, full = _planted(SMALL + 1)
    n = SMALL + 1
    cl = diarize.cluster(dev, [0, n], threshold=-INF, return_merges=True)
    assert cl.labels.dtype == torch.int32 and cl.n_clusters.dtype == torch.int32 and cl.labels.is_cuda
    _assert_same((cl.labels.cpu().numpy(), cl.n_clusters.cpu().numpy(), *[m.cpu().numpy() for m in cl.merges]), full, "module")
    two = diarize.cluster(dev, [0, n], n_speakers=2)
    assert two.merges is None and int(two.n_clusters[0]) == 2
    assert np.array_equal(two.labels.cpu().numpy(), diar_ref.ahc_batch(host, [0, n], want=[2])[0])
    capped = diarize.cluster(dev, [0, n], threshold=INF, max_speakers=4)
    assert int(capped.n_clusters[0]) == 4
    cols = dev.t().contiguous().t()                  # a column-major view is made contiguous, not misread
    assert torch.equal(diarize.cluster(cols, [0, n], n_speakers=2).labels, two.labels)
    with pytest.raises(ValueError, match="threshold, n_speakers"):
        diarize.cluster(dev, [0, n])
    with pytest.raises(ValueError, match="rec_start must rise"):
        diarize.cluster(dev, [0, n - 1], threshold=0.0)
    with pytest.raises(ValueError, match="square"):
        diarize.cluster(dev[:, :5], [0, n], threshold=0.0)


def test_diarizer_equals_its_pieces_on_two_alternating_speakers(synth):
    import xvector_amd as xa
    from xvector_amd import diarize
    from xvector_amd.scoring import cosine_scores
    cin, hid, xv, nc = 24, 72, 16, 3
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in
          synth.make_state_dict(706, input_size=cin, hidden_size=hid, num_classes=nc, x_vector_size=xv).items()}
    model = xa.XVectorModel(input_size=cin, hidden_size=hid, num_classes=nc, x_vector_size=xv)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    # three recordings; two speakers (a shift of every coefficient, of opposite sign) taking turns of 120 frames
    rng = np.random.default_rng(5)
    lengths = [960, 700, 400]
    x = synth.make_mfcc(3, max(lengths), seed=8)
    shift = rng.standard_normal(cin).astype(np.float32) * 1.5
    who = (np.arange(max(lengths)) // 120) % 2
    x += np.where(who[None, :, None] == 0, shift, -shift)
    xd = torch.from_numpy(x).to(DEV)
    win, hop = 60, 30
    d = diarize.Diarizer(model, "cosine", win=win, hop=hop, max_score_rows=40, device=DEV)
    res = d.diarize(xd, lengths=lengths, n_speakers=2)
    vecs, windows = model.extract_windows(xd, win, hop, lengths=lengths)
    assert np.array_equal(res.windows, windows) and res.labels.shape == (len(windows),) and res.labels.dtype == np.int32
    counts = [int((windows[:, 0] == u).sum()) for u in range(3)]
    rs = _starts(counts)
    calls = d.calls(rs)
    assert calls == [(0, 1), (1, 3)] and counts == [(n - win) // hop + 1 for n in lengths]
    for a, b in calls:                               # the scores of every call, computed here, through cluster and the reference
        lo, hi = int(rs[a]), int(rs[b])
        S = cosine_scores(vecs[lo:hi].double(), device=DEV)
        cl = diarize.cluster(S, rs[a:b + 1] - lo, n_speakers=2)
        assert np.array_equal(res.labels[lo:hi], cl.labels.cpu().numpy())
        assert np.array_equal(res.labels[lo:hi], diar_ref.ahc_batch(S.cpu().numpy(), rs[a:b + 1] - lo, want=[2] * (b - a))[0])
    assert res.n_clusters.tolist() == [2, 2, 2]
    # the turns cover the windows: per recording from its first window's start to its last window's end, without a hole
    # (hop < win: consecutive windows overlap), speakers alternating
    t = res.turns
    for u in range(3):
        tu, wu = t[t[:, 0] == u], windows[windows[:, 0] == u]
        assert tu[0, 1] == wu[0, 1] and tu[-1, 2] == wu[-1, 1] + wu[-1, 2]
        assert (tu[1:, 1] == tu[:-1, 2]).all() and (tu[1:, 3] != tu[:-1, 3]).all() and set(tu[:, 3].tolist()) <= {0, 1}
    by_threshold = diarize.Diarizer(model, "cosine", win=win, hop=hop, threshold=2.0, device=DEV).diarize(xd, lengths=lengths)
    assert by_threshold.n_clusters.tolist() == counts            # no cosine reaches 2: nothing merges
