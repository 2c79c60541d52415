"""CPU checks of the segments surface (sliding windows and segments of recordings): the window lists against hand-written
answers, the call planner's invariants on seeded random cases and one case by hand, the host refusals of extract_segments
(raised before the device is looked at), the C ABI's argument errors, and the new kernels' resources."""
import ctypes

import numpy as np
import pytest
import torch

from hipcc_support import kernel_resources, needs_hipcc


def _rows(*rows):
    return np.asarray(rows, dtype=np.int32).reshape(-1, 3)


# ------------------------------------------------------------------------------- sliding_windows
def test_sliding_windows_hand_written_answers():
    from xvector_amd import sliding_windows as sw
    assert sw([40], 40, 13).dtype == np.int32
    # T == win: the one full window, no tail with or without min_tail
    assert np.array_equal(sw([40], 40, 13), _rows((0, 0, 40)))
    assert np.array_equal(sw([40], 40, 13, min_tail=15), _rows((0, 0, 40)))
    # T == win - 1: nothing without min_tail, the whole recording as the single (tail) window with it
    assert sw([39], 40, 13).shape == (0, 3)
    assert np.array_equal(sw([39], 40, 13, min_tail=16), _rows((0, 0, 39)))
    assert sw([39], 40, 13, min_tail=40).shape == (0, 3)
    # (T - win) % hop == 0: the last full window ends on the last frame, no tail
    assert np.array_equal(sw([66], 40, 13, min_tail=15), _rows((0, 0, 40), (0, 13, 40), (0, 26, 40)))
    # one frame more: frames remain, the tail [3 * 13, 67) has 28 frames
    assert np.array_equal(sw([67], 40, 13, min_tail=15), _rows((0, 0, 40), (0, 13, 40), (0, 26, 40), (0, 39, 28)))
    assert np.array_equal(sw([67], 40, 13), _rows((0, 0, 40), (0, 13, 40), (0, 26, 40)))
    # a remainder below min_tail is dropped: T = 90, full windows at 0, 30, 60 (end 90)? no: 60 + 40 > 90 -> 0, 30; tail [60, 90)
    assert np.array_equal(sw([90], 40, 30, min_tail=31), _rows((0, 0, 40), (0, 30, 40)))
    assert np.array_equal(sw([90], 40, 30, min_tail=30), _rows((0, 0, 40), (0, 30, 40), (0, 60, 30)))
    # hop > win: the frames between windows are skipped, and a tail that would start past the end does not exist
    assert np.array_equal(sw([150], 40, 100, min_tail=15), _rows((0, 0, 40), (0, 100, 40)))
    # several recordings, ordered by utterance, then start
    assert np.array_equal(sw([47, 20, 55], 40, 13, min_tail=16),
                          _rows((0, 0, 40), (0, 13, 34), (1, 0, 20), (2, 0, 40), (2, 13, 40), (2, 26, 29)))
    assert np.array_equal(sw(torch.tensor([47, 20]), 40, 13), _rows((0, 0, 40)))


@pytest.mark.parametrize("kw", [dict(win=14, hop=1), dict(win=40, hop=0), dict(win=40, hop=-3),
                                dict(win=40, hop=13, min_tail=14), dict(win=40, hop=13, min_tail=0)])
def test_sliding_windows_refusals(kw):
    from xvector_amd import sliding_windows
    with pytest.raises(ValueError):
        sliding_windows([100], **kw)


# ------------------------------------------------------------------------------- the call planner
def _check_plan(seg, calls, max_frames):
    seen = []
    for c in calls:
        assert c.frames <= max_frames and c.frames == sum(hi - lo for _, lo, hi in c.pieces)
        assert len(c.pieces) >= 1 and len(c.segs) >= 1
        for k, (u, lo, hi) in enumerate(c.pieces):
            mine = c.segs[c.segs[:, 1] == k]
            assert len(mine), "a piece without segments"
            g = seg[mine[:, 0]]
            assert (g[:, 0] == u).all()
            assert np.array_equal(g[:, 1], mine[:, 2] + lo) and np.array_equal(g[:, 2], mine[:, 3])      # local = global - lo
            assert (mine[:, 2] >= 0).all() and (mine[:, 2] + mine[:, 3] <= hi - lo).all()                 # inside its piece
            assert lo == g[:, 1].min() and hi == (g[:, 1] + g[:, 2]).max()                                # the hull of its run
            assert (np.diff(g[:, 1]) >= 0).all()                                                          # in start order
        seen += c.segs[:, 0].tolist()
    assert sorted(seen) == list(range(len(seg))), "every segment exactly once"
    # the pieces of one recording are consecutive runs of its segments in start order
    last = {}
    for c in calls:
        for k, (u, lo, hi) in enumerate(c.pieces):
            first_start = seg[c.segs[c.segs[:, 1] == k][:, 0], 1].min()
            assert first_start >= last.get(u, -1)
            last[u] = seg[c.segs[c.segs[:, 1] == k][:, 0], 1].max()


@pytest.mark.parametrize("seed", range(8))
def test_planner_random_cases(seed):
    from xvector_amd import plan_segment_calls
    rng = np.random.default_rng(seed)
    n_rec = int(rng.integers(1, 7))
    lens = rng.integers(15, 3000, n_rec)
    max_frames = int(rng.integers(200, 1500))
    n = int(rng.integers(1, 60))
    utt = rng.integers(0, n_rec, n)
    ln = np.minimum(rng.integers(15, min(max_frames, 400) + 1, n), lens[utt])
    st = (rng.random(n) * (lens[utt] - ln + 1)).astype(np.int64)
    seg = np.stack([utt, st, ln], 1).astype(np.int64)
    if seed % 2:                        # duplicates and a shuffled order
        seg = np.concatenate([seg, seg[:3]])[rng.permutation(n + min(3, n))]
    calls = plan_segment_calls(seg, max_frames)
    _check_plan(seg, calls, max_frames)
    small = plan_segment_calls(seg, max_frames, max_pieces=1)
    _check_plan(seg, small, max_frames)
    assert all(len(c.pieces) == 1 for c in small)
    few = plan_segment_calls(seg, max_frames, max_segments=4)
    _check_plan(seg, few, max_frames)
    assert all(len(c.segs) <= 4 for c in few)


def test_planner_bounds_the_segments_of_a_call():
    """Dense and repeated segments over few frames: the segment count cuts the pieces and the calls, not the frames."""
    from xvector_amd import plan_segment_calls
    from xvector_amd.model import MAX_SEGMENTS_PER_CALL
    assert MAX_SEGMENTS_PER_CALL == 65535 * 16                   # ceil(M / 16) on grid.y in the segment layers' direct form
    seg = np.asarray([(0, s, 20) for s in range(10)] + [(0, 3, 20)] * 3 + [(1, 0, 15)], dtype=np.int64)      # hop 1, duplicates
    calls = plan_segment_calls(seg, 1000, max_segments=4)
    _check_plan(seg, calls, 1000)
    assert [len(c.segs) for c in calls] == [4, 4, 4, 2]
    assert [c.pieces for c in calls] == [[(0, 0, 23)], [(0, 3, 24)], [(0, 5, 28)], [(0, 9, 29), (1, 0, 15)]]
    assert [len(c.segs) for c in plan_segment_calls(seg, 1000)] == [14]
    one = plan_segment_calls(seg, 1000, max_segments=1)
    _check_plan(seg, one, 1000)
    assert len(one) == 14
    with pytest.raises(ValueError, match="max_segments"):
        plan_segment_calls(seg, 1000, max_segments=0)


def test_planner_2000_frames_by_hand():
    from xvector_amd import plan_segment_calls, sliding_windows
    seg = sliding_windows([2000], 300, 75, min_tail=20)
    assert len(seg) == 24 and tuple(seg[-1]) == (0, 1725, 275) and tuple(seg[-2]) == (0, 1650, 300)
    calls = plan_segment_calls(seg, 600)
    # five windows at hop 75 span 4 * 75 + 300 = 600 frames: pieces start every 375 frames
    assert [c.pieces for c in calls] == [[(0, 0, 600)], [(0, 375, 975)], [(0, 750, 1350)], [(0, 1125, 1725)], [(0, 1500, 2000)]]
    assert [len(c.segs) for c in calls] == [5, 5, 5, 5, 4]
    assert calls[1].segs.tolist() == [[5 + i, 0, 75 * i, 300] for i in range(5)]
    assert calls[4].segs.tolist() == [[20, 0, 0, 300], [21, 0, 75, 300], [22, 0, 150, 300], [23, 0, 225, 275]]
    _check_plan(seg.astype(np.int64), calls, 600)
    # everything in one call when it fits, and two recordings share a call
    assert [c.pieces for c in plan_segment_calls(seg, 2000)] == [[(0, 0, 2000)]]
    two = plan_segment_calls([(1, 10, 50), (0, 5, 20), (1, 100, 30)], 1000)
    assert [c.pieces for c in two] == [[(0, 5, 25), (1, 10, 130)]]
    assert two[0].segs.tolist() == [[1, 0, 0, 20], [0, 1, 0, 50], [2, 1, 90, 30]]
    with pytest.raises(ValueError, match="max_frames"):
        plan_segment_calls([(0, 0, 601)], 600)


# ------------------------------------------------------------------------------- host refusals of extract_segments
@pytest.mark.parametrize("segments, kw, what", [
    ([(0, 0, 40, 1)], {}, "integer array"),               # wrong shape
    (np.zeros((0, 3), dtype=np.int64), {}, "integer array"),
    ([0, 0, 40], {}, "integer array"),
    ([(0.0, 0.0, 40.0)], {}, "integer array"),
    ([(2, 0, 40)], {}, "outside the batch"),
    ([(-1, 0, 40)], {}, "outside the batch"),
    ([(0, 0, 14)], {}, "at least 15"),
    ([(0, 61, 40)], {}, "leaves its recording"),
    ([(0, -1, 40)], {}, "leaves its recording"),
    ([(1, 11, 40)], dict(lengths=[100, 50]), "leaves its recording"),
    ([(0, 0, 40)], dict(lengths=[100, 14]), "at least 15"),
    ([(0, 0, 40)], dict(lengths=[100, 101]), "lengths"),
    ([(0, 0, 40)], dict(logits=True, pooled=True), "exclude"),
])
def test_extract_segments_refuses_on_the_host(segments, kw, what):
    """A CPU tensor would be refused with a RuntimeError as soon as the device is looked at: the segment checks come first."""
    import xvector_amd as xa
    m = xa.XVectorModel()
    x = torch.zeros(2, 100, 24)
    with pytest.raises(ValueError, match=what):
        m.extract_segments(x, segments, **kw)


def test_extract_segments_packed_refusals_and_the_device_check():
    import xvector_amd as xa
    m = xa.XVectorModel()
    rows = torch.zeros(150, 24)
    with pytest.raises(ValueError, match="leaves its recording"):
        m.extract_segments(rows, [(1, 20, 40)], offsets=[0, 100, 150])
    with pytest.raises(ValueError, match="packed input"):
        m.extract_segments(rows, [(0, 0, 40)], offsets=[0, 100, 151])
    with pytest.raises(ValueError, match="channels"):
        m.extract_segments(torch.zeros(2, 100, 23), [(0, 0, 40)])
    with pytest.raises(RuntimeError, match="HIP device"):       # valid segments: only now the device is looked at
        m.extract_segments(rows, [(1, 10, 40)], offsets=[0, 100, 150])
    with pytest.raises(ValueError):
        m.extract_windows(torch.zeros(2, 30, 24), 40, 13)       # no recording holds a window
    with pytest.raises(RuntimeError, match="HIP device"):
        m.extract_windows(torch.zeros(2, 100, 24), 40, 13)


def test_window_records_names_windows(monkeypatch):
    import xvector_amd as xa
    from xvector_amd import extract
    m = xa.XVectorModel()
    monkeypatch.setattr(m, "extract_segments", lambda x, seg, **kw: torch.arange(len(seg) * 2.0).reshape(-1, 2))
    rec = extract.window_records(m, torch.zeros(2, 60, 24), ["a", "b"], torch.tensor([7, 9]), 40, 13, lengths=[60, 47], min_tail=16)
    assert [r[0] for r in rec] == ["a@0+40", "a@13+40", "a@26+34", "b@0+40", "b@13+34"]
    assert [r[1] for r in rec] == [7, 7, 7, 9, 9]
    assert rec[3][2].dtype == np.float64 and rec[3][2].tolist() == [6.0, 7.0]


# ------------------------------------------------------------------------------- C ABI without a GPU
def test_c_abi_argument_errors_without_gpu():
    from xvector_amd import hip
    lib = hip.lib
    for name in ("xvec_forward_segments", "xvec_stat_pool_segments", "xvec_segments_workspace_bytes"):
        assert name in hip.EXPORTS and hasattr(lib, name)
    assert lib.xvec_segments_workspace_bytes(None, 1000, 2, 10) == 0
    assert lib.xvec_forward_segments(None, None, None, 1, None, None, None, 1, hip.MODE_XVEC6, hip.F32, None, None, 0,
                                     None) == hip.ERR_ARG
    assert "null" in hip.last_error()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert lib.xvec_stat_pool_segments(None, 0, 4, 4, 4, None, None, 1, None, None, None, None) == hip.ERR_ARG
    assert "null" in hip.last_error()
    # (host memory stands in for the pointers: these are refused before anything is launched)
    assert lib.xvec_stat_pool_segments(p, 2, 4, 4, 4, p, p, 1, None, None, p, None) == hip.ERR_ARG      # unknown element type
    assert lib.xvec_stat_pool_segments(p, 0, 4, 3, 4, p, p, 1, None, None, p, None) == hip.ERR_ARG      # ldy < C
    assert lib.xvec_stat_pool_segments(p, 0, 0, 4, 4, p, p, 1, None, None, p, None) == hip.ERR_ARG      # no rows
    assert lib.xvec_stat_pool_segments(p, 0, 4, 4, 4, p, p, 0, None, None, p, None) == hip.ERR_ARG      # no segments
    assert lib.xvec_stat_pool_segments(p, 0, 4, 4, 4, p, p, 1, p, None, p, None) == hip.ERR_ARG         # scale without shift
    assert "together" in hip.last_error()


def test_which_pooling_variant_runs_is_host_arithmetic():
    """xvec_stat_pool_segments_vector: 16-byte loads need a 16-byte base, a row stride of whole vectors and C rounded up to the
    vector inside ldy; anything else is the element-wise variant.  No pointer is dereferenced."""
    from xvector_amd import hip
    v = hip.lib.xvec_stat_pool_segments_vector
    base = 0x10000
    for elem, es, vec in ((0, 4, 4), (1, 2, 8)):
        assert v(base, elem, 1536, 1500) == 1 and v(base, elem, 256, 256) == 1
        assert v(base + 4, elem, 256, 256) == 0 and v(base + 8, elem, 256, 256) == 0          # the base
        assert v(base + 16, elem, 256, 256) == 1
        assert v(base, elem, 7, 7) == 0 and v(base, elem, 256 + vec // 2, 256) == 0            # the row stride
        assert v(base, elem, 2 * vec, 2 * vec) == 1 and v(base, elem, 2 * vec, 2 * vec - 1) == 1
        assert v(base, elem, vec, vec) == 1                                                    # C = 4 fp32: one vector
        assert v(None, elem, 8, 8) == -1 and v(base, elem, 4, 8) == -1 and v(base, elem, 8, 0) == -1
    assert v(base, 0, 260, 260) == 1 and v(base, 1, 260, 260) == 0        # 260 = 65 fp32 vectors, but 32.5 bf16 vectors a row
    assert v(base, 1, 264, 260) == 1                                      # C rounds up to 264 inside ldy
    assert v(base, 2, 8, 8) == -1


# ------------------------------------------------------------------------------- kernel resources
KERNELS = ("pool_segments_kernelILb0ELi4E", "pool_segments_kernelILb0ELi1E", "pool_segments_kernelILb1ELi8E",
           "pool_segments_kernelILb1ELi1E", "segment_rows_kernel")


@needs_hipcc
def test_segment_kernels_use_no_scratch():
    kernels = kernel_resources("pool_segments.hip")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for want in KERNELS:
        name = [k for k in kernels if want in k]
        assert len(name) == 1, (want, sorted(kernels))
        r = kernels[name[0]]
        assert r["scratch"] == 0 and r.get("spill", 0) == 0, (want, r)
        assert r["vgprs"] <= 128, (want, r)               # four blocks of four waves per CU and more
    # LDS: the sums of three waves, two planes, 64 lanes x VEC floats
    for want, vec in (("ILb0ELi4E", 4), ("ILb0ELi1E", 1), ("ILb1ELi8E", 8), ("ILb1ELi1E", 1)):
        r = kernels[[k for k in kernels if want in k][0]]
        assert r["lds"] == 2 * 3 * 64 * vec * 4, (want, r)
