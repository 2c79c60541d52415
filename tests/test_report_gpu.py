"""The trial report on the GPU (csrc/report.hip through xvector_amd.report) against the numpy restatement tests/report_ref.py.

Every comparison is bit for bit (NaN equal to NaN): the arithmetic is integer counts, comparisons and fp64 operations that round
correctly.  The images are written into buffers filled with 0xA5 at chosen byte offsets, and the bytes around them must come
back unchanged.  The shapes are small: 4096 cells make a tile of the image pass, 4096 trials a block of the curve's scan and 16
a thread's share of it, so a few thousand elements reach every path but one: the one-block scans carry their totals across
chunks of 256 blocks, which takes a million trials (a few tests at 256 * 4096 and either side)."""
import numpy as np
import pytest
import torch

import eer_ref
import report_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
U8, F32 = np.uint8, np.float32
TORCH = {U8: torch.uint8, F32: torch.float32}


def device_matrix(host, pad=0):
    """The matrix on the device with row stride n_cols + pad, its base one element into its buffer."""
    r, c = host.shape
    buf = torch.full((r * (c + pad) + 1,), float("nan"), dtype=torch.float64, device=DEV)
    s = buf[1:].view(r, c + pad)[:, :c]
    s.copy_(torch.from_numpy(host))
    return s


def raw_images(s, trials, e_th, m_th, dtype, which=63, offset=0):
    """xvec_report_images through the C ABI, every selected image `offset` bytes into a 16-byte aligned window of a buffer of
    0xA5: {name: host array in the stored shape}, after checking that the bytes around each image are untouched."""
    from xvector_amd import hip, report
    m = report.trial_map(trials, s.shape, s.device)
    rec = report._range_record(s)
    r, c = s.shape
    es = np.dtype(dtype).itemsize
    bufs, ptrs, shapes = [], [], []
    for i, name in enumerate(report.IMAGE_NAMES):
        shape = report._image_shape(i, r, c)
        nbytes = int(np.prod(shape)) * es
        buf = torch.full((GUARD + 16 + nbytes + GUARD + 16,), 0xA5, dtype=torch.uint8, device=DEV)
        start = (-buf.data_ptr()) % 16 + GUARD + offset
        bufs.append((buf, start, nbytes))
        shapes.append(shape)
        ptrs.append(buf.data_ptr() + start if which >> i & 1 else None)
    rc = hip.lib.xvec_report_images(s.data_ptr(), s.stride(0), r, c, m.data_ptr(), m.stride(0), rec.data_ptr(), float(e_th),
                                    float(m_th), which, 0 if dtype == U8 else 1, *ptrs,
                                    torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == 0, hip.lib.xvec_report_last_error().decode()
    out = {}
    for i, name in enumerate(report.IMAGE_NAMES):
        buf, start, nbytes = bufs[i]
        host = buf.cpu().numpy()
        if which >> i & 1:
            assert (host[:start] == 0xA5).all() and (host[start + nbytes:] == 0xA5).all(), (name, offset, "guard bytes")
            out[name] = host[start:start + nbytes].copy().view(dtype).reshape(shapes[i])
        else:
            assert (host == 0xA5).all(), (name, "not selected")
    return out


def expected(host, trials, e_th, m_th, dtype):
    """{name: array in the stored shape} by the restatement."""
    pos, neg, _ = report_ref.masks(trials.row_idx, trials.col_idx, trials.is_target, host.shape)
    ref = {n: report_ref.as_dtype(v, dtype) for n, v in report_ref.images(host, pos, neg, e_th, m_th).items()}
    ref["score_matrix"] = ref["score_matrix"][0]
    return ref


def check_images(got, ref, what):
    for name, img in got.items():
        if not report_ref.same(img, ref[name]):
            bad = np.argwhere(~((img == ref[name]) | (np.isnan(img.astype(np.float64)) & np.isnan(ref[name].astype(np.float64)))))
            first = tuple(bad[0])
            raise AssertionError(f"{what} {name}: {len(bad)} cells differ, first {first}: got {img[first]!r} want {ref[name][first]!r}")


def case(r, c, seed):
    """(host matrix, TrialList, eer threshold, minDCF threshold): a third of the cells named, one by a target and a non-target
    trial; the second threshold is exactly a named cell's score."""
    from xvector_amd.evaluate import TrialList
    rng = np.random.default_rng(seed)
    host = rng.normal(0.0, 10.0, (r, c))
    n = max(1, r * c // 3)
    cells = rng.permutation(r * c)[:n]
    tgt = rng.integers(0, 2, n)
    cells, tgt = np.r_[cells, cells[0]], np.r_[tgt, 1 - tgt[0]]
    return host, TrialList(cells // c, cells % c, tgt), float(np.median(host)), float(host.reshape(-1)[cells[n // 2]])


SHAPES = [(1, 1), (2, 3), (5, 16), (7, 59), (3, 64), (3, 65), (2, 127), (2, 129), (65, 11), (33, 257)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_images_at_every_shape_stride_type_and_offset(shape):
    r, c = shape
    host, trials, e_th, m_th = case(r, c, 100 * r + c)
    for dtype in (U8, F32):
        ref = expected(host, trials, e_th, m_th, dtype)
        step = 1 if dtype == U8 else 4
        offsets = range(0, 16, step) if shape == (5, 16) else (0, 5 * step % 16, 11 * step % 16)
        for pad in (0, 3):
            s = device_matrix(host, pad)
            for offset in offsets if pad == 0 else (3 * step,):
                check_images(raw_images(s, trials, e_th, m_th, dtype, offset=offset), ref, f"{shape} {dtype.__name__} pad {pad} offset {offset}")


def test_images_across_tiles_of_the_image_pass():
    """More columns than a tile (4096) in one row, and rows of a narrow matrix that end a tile of several rows."""
    for r, c in ((2, 4099), (700, 7)):
        host, trials, e_th, m_th = case(r, c, r + c)
        s = device_matrix(host, 1)
        for dtype, offset in ((U8, 9), (F32, 4)):
            check_images(raw_images(s, trials, e_th, m_th, dtype, offset=offset), expected(host, trials, e_th, m_th, dtype), f"{r}x{c}")


def test_the_same_cell_gives_the_same_bytes_whatever_is_selected():
    host, trials, e_th, m_th = case(7, 59, 5)
    s = device_matrix(host, 2)
    for dtype in (U8, F32):
        every = raw_images(s, trials, e_th, m_th, dtype, which=63, offset=4)
        check_images(every, expected(host, trials, e_th, m_th, dtype), "all")
        for which in (1, 2, 4, 8, 16, 32, 9, 36, 62):
            some = raw_images(s, trials, e_th, m_th, dtype, which=which, offset=12)
            assert len(some) == bin(which).count("1")
            for name, img in some.items():
                assert report_ref.same(img, every[name]), (which, name)


def test_special_cells_and_thresholds():
    from xvector_amd.evaluate import TrialList
    nan, inf = float("nan"), float("inf")
    host = np.array([[1.5, nan, 3.0, inf, -inf, 0.25, -2.0],
                     [nan, 4.0, inf, -inf, 7.5, -0.5, 6.0],
                     [2.0, 2.5, -1.0, 0.0, -0.0, 9.0, 3.0]])
    # named: a NaN, both infinities, the cell (0, 2) = 3.0 by a target and a non-target trial (K = 2), ordinary cells; unnamed: the others
    rows, cols, tgt = [0, 0, 0, 0, 0, 1, 1, 2, 2, 2], [1, 3, 4, 2, 2, 1, 4, 0, 5, 6], [1, 0, 1, 1, 0, 1, 0, 0, 1, 1]
    trials = TrialList(rows, cols, tgt)
    s = device_matrix(host, 1)
    four = 4.0
    thresholds = [4.5,                                              # between S = 3 and 2 S = 6 of the K = 2 cell
                  four, np.nextafter(four, -inf), np.nextafter(four, inf),      # exactly a cell's score and one step either side
                  6.0, np.nextafter(6.0, -inf), np.nextafter(6.0, inf),         # ... and the same around 2 S of the K = 2 cell
                  inf, -inf, nan, 0.0]
    for dtype in (U8, F32):
        for k, t in enumerate(thresholds):
            u = thresholds[(k + 3) % len(thresholds)]
            check_images(raw_images(s, trials, t, u, dtype, offset=4), expected(host, trials, t, u, dtype), f"thresholds {t} {u}")
    from xvector_amd import report
    assert report.score_range(s) == (-2.0, 9.0, 6)
    # the images through the module: the score matrix comes back as an expanded view of one plane
    imgs = report.score_images(s, trials, 4.5, 4.0)
    assert imgs["score_matrix"].shape == (3, 3, 7) and imgs["score_matrix"].stride(0) == 0
    ref = expected(host, trials, 4.5, 4.0, U8)
    assert np.array_equal(imgs["score_matrix"].cpu().numpy(), np.broadcast_to(ref["score_matrix"], (3, 3, 7)))
    for name in report.IMAGE_NAMES[1:]:
        assert imgs[name].is_contiguous() and np.array_equal(imgs[name].cpu().numpy(), ref[name]), name


def test_images_from_a_map_into_given_tensors():
    from xvector_amd import report
    host, trials, e_th, m_th = case(7, 59, 8)
    s = device_matrix(host, 3)
    plain = report.score_images(s, trials, e_th, m_th, dtype=torch.float32)
    m = report.trial_map(trials, s.shape, DEV)
    which = report.SCORE_MATRIX | report.FALSE
    out = {"score_matrix": torch.full((7, 59), -1.0, dtype=torch.float32, device=DEV),
           "false_prediction_eer_min_dcf": torch.full((3, 7, 123), -1.0, dtype=torch.float32, device=DEV)}
    got = report.score_images(s, m, e_th, m_th, dtype=torch.float32, which=which, out=out)
    assert sorted(got) == sorted(out) and got["false_prediction_eer_min_dcf"] is out["false_prediction_eer_min_dcf"]
    assert got["score_matrix"].data_ptr() == out["score_matrix"].data_ptr() and got["score_matrix"].shape == (3, 7, 59)
    for name in got:
        assert report_ref.same(got[name].cpu().numpy(), plain[name].cpu().numpy()), name
    for bad in ({"score_matrix": torch.empty((3, 7, 59), dtype=torch.float32, device=DEV)},
                {"score_matrix": torch.empty((7, 59), dtype=torch.uint8, device=DEV)}):
        with pytest.raises(ValueError, match="out\\['score_matrix'\\]"):
            report.score_images(s, m, e_th, m_th, dtype=torch.float32, which=which, out=bad)
    with pytest.raises(ValueError, match="TrialList or the uint8 map"):
        report.score_images(s, m[:, :58], e_th, m_th)
    with pytest.raises(ValueError, match="which"):
        report.score_images(s, m, e_th, m_th, which=64)


def test_constant_matrix_zero_trials_and_bad_indices():
    from xvector_amd import report
    from xvector_amd.evaluate import TrialList
    host = np.full((4, 9), 2.75)
    trials = TrialList([0, 3], [1, 8], [1, 0])
    for dtype in (U8, F32):                                         # 0 / 0 in every cell, as numpy
        got = raw_images(device_matrix(host), trials, 1.0, 3.0, dtype)
        check_images(got, expected(host, trials, 1.0, 3.0, dtype), "constant")
    assert np.isnan(raw_images(device_matrix(host), trials, 1.0, 3.0, F32)["score_matrix"]).all()
    host, _, e_th, m_th = case(5, 16, 1)
    none = TrialList([], [], [])
    m, bad = report.trial_map(none, host.shape, DEV, return_bad=True)
    assert bad == 0 and not m.any()
    for dtype in (U8, F32):
        check_images(raw_images(device_matrix(host), none, e_th, m_th, dtype), expected(host, none, e_th, m_th, dtype), "no trials")
    rows, cols, tgt = [0, 5, -1, 2, 4, 0, 2 ** 31 - 1], [3, 0, 2, 16, -1, 15, 2 ** 31 - 1], [1, 1, 0, 0, 1, 0, 1]
    some = TrialList(rows, cols, tgt)
    m, bad = report.trial_map(some, host.shape, DEV, return_bad=True)
    pos, neg, want_bad = report_ref.masks(rows, cols, tgt, host.shape)
    assert bad == want_bad == 5
    assert np.array_equal(m.cpu().numpy(), (pos + 2 * neg).astype(np.uint8))
    check_images(raw_images(device_matrix(host), some, e_th, m_th, U8), expected(host, some, e_th, m_th, U8), "bad indices")


class _Plda:
    pass


class _Recorder:
    def __init__(self):
        self.calls = []

    def add_image(self, name, image, step):
        self.calls.append((name, image, step))


def test_against_the_reference_s_own_masks_and_through_the_stat_object(tmp_path):
    import pandas as pd
    from xvector_amd import report
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
    with pytest.raises(RuntimeError, match="test_plda first"):
        obj.score_images()
    obj.test_plda(plda, path)
    for call in (obj.score_images, lambda: obj.write_images(_Recorder())):
        with pytest.raises(RuntimeError, match="calc_eer_mindcf first"):
            call()
    assert len(obj.det_curve().tp) > 1                              # the curve needs no thresholds
    obj.calc_eer_mindcf()
    m = report.trial_map(obj._trials, (60, 60), DEV).cpu().numpy()
    assert np.array_equal(m & 1, g["positive_scores_mask"].astype(np.uint8))         # the reference's own masks
    assert np.array_equal(m >> 1, g["negative_scores_mask"].astype(np.uint8))
    host = obj._scoremat.cpu().numpy()
    for dtype in (U8, F32):
        ref = {n: report_ref.as_dtype(v, dtype)
               for n, v in report_ref.images(host, g["positive_scores_mask"], g["negative_scores_mask"], obj.eer_th, obj.min_dcf_th).items()}
        imgs = obj.score_images(dtype=TORCH[dtype])
        assert list(imgs) == list(report.IMAGE_NAMES)
        for name in report.IMAGE_NAMES:
            assert report_ref.same(imgs[name].cpu().numpy(), ref[name]), (name, dtype)
    rec = _Recorder()
    obj.write_images(rec, step=3)
    assert [c[0] for c in rec.calls] == list(report.IMAGE_NAMES) and all(c[2] == 3 for c in rec.calls)
    assert [tuple(c[1].shape) for c in rec.calls] == [(3, 60, 60)] * 3 + [(3, 60, 125)] * 3
    assert all(c[1].device.type == "cpu" and c[1].dtype == torch.uint8 for c in rec.calls)
    det = obj.det_curve()
    assert det.eer() == (obj.eer, obj.eer_th) and det.min_dcf() == (obj.min_dcf, obj.min_dcf_th)
    with pytest.raises(NotImplementedError):
        obj.plot_images(None)


# ---------------------------------------------------------------- the DET curve

def listed(scores, tgt, width=64):
    """The scores in the cells of a [rows, width] device matrix (row stride width + 1, NaN elsewhere) and the TrialList that
    names them in order."""
    from xvector_amd.evaluate import TrialList
    n = len(scores)
    rows = -(-n // width)
    host = np.full((rows, width), np.nan)
    host.reshape(-1)[:n] = scores
    return host, device_matrix(host, 1), TrialList(np.arange(n) // width, np.arange(n) % width, tgt)


def check_curve(det, host, trials, grid, what):
    s, t, n_nan, n_bad = report_ref.select(host, trials.row_idx, trials.col_idx, trials.is_target)
    thr, tp, nn, n_pos, n_neg = report_ref.det_points(s, t)
    assert (det.n_target, det.n_nontarget, det.n_nan, det.n_bad_index) == (n_pos, n_neg, n_nan, n_bad), what
    thr, tp, nn = report_ref.thin(thr, tp, nn, n_pos, n_neg, grid)
    assert det.thresholds.dtype == np.float32 and det.tp.dtype == np.int64 and det.nn.dtype == np.int64
    assert np.array_equal(det.thresholds.view(np.uint32), thr.view(np.uint32)), what
    assert np.array_equal(det.tp, tp) and np.array_equal(det.nn, nn), what
    if grid:
        assert len(det.tp) <= 2 * grid + 2, what


SIZES = [1, 2, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193]


@pytest.mark.parametrize("n", SIZES)
def test_curve_at_the_scan_s_block_and_chunk_sizes(n):
    from xvector_amd import report
    rng = np.random.default_rng(n)
    scores = rng.integers(-n // 3 - 1, n // 3 + 2, n) / 8.0         # ties: three trials per distinct score on average
    tgt = rng.integers(0, 2, n)
    host, s, trials = listed(scores, tgt)
    for grid in (0, 4):
        check_curve(report.det_curve(s, trials, grid), host, trials, grid, f"n {n} grid {grid}")
    # ... and as a plain vector with the target flags alone
    vec = torch.from_numpy(scores).to(DEV)
    det = report.det_curve(vec, tgt)
    assert np.array_equal(det.tp, report.det_curve(s, trials).tp) and len(det.tp) == len(np.unique(scores))


# The one-block scans (report_det_scan_kernel, report_det_keep_scan_kernel) walk the per-block sums 256 blocks at a time and
# carry the totals from one such chunk to the next: 256 * 4096 trials fill the first chunk exactly.
CHUNK_TRIALS = 256 * 4096


@pytest.mark.parametrize("n", [CHUNK_TRIALS - 1, CHUNK_TRIALS, CHUNK_TRIALS + 1])
def test_curve_across_the_chunks_of_the_one_block_scans(n):
    from xvector_amd import report
    rng = np.random.default_rng(n)
    tgt = rng.integers(0, 2, n)
    # runs of 100 equal scores, shuffled: the run 1048500 .. 1048599 of the sorted order spans the chunk's edge;
    # all distinct (exact in fp32): more points than a chunk of the keep pass holds, so its carry is used as well
    for name, scores in (("runs", (rng.permutation(n) // 100).astype(np.float64)), ("distinct", rng.permutation(n) / 4.0 - 1000.0)):
        host, s, trials = listed(scores, tgt, width=1024)
        for grid in (0, 1000):
            det = report.det_curve(s, trials, grid)
            check_curve(det, host, trials, grid, f"n {n} {name} grid {grid}")
            assert det.tp[-1] == det.n_target and det.nn[-1] == det.n_nontarget
        if name == "distinct":
            assert len(report.det_curve(s, trials).tp) == n > CHUNK_TRIALS - 2


def test_curve_of_all_pairs_across_the_chunks_of_the_one_block_scans():
    from xvector_amd import report
    from xvector_amd.evaluate import TrialList
    rng = np.random.default_rng(12)
    r, c = 1025, 1024                                               # 1 049 600 cells: 257 blocks
    rows, cols = rng.integers(0, 50, r), rng.integers(0, 50, c)
    host = np.round(rng.normal(0.0, 300.0, (r, c)) * 8.0) / 8.0
    host[3, 3] = host[1000, 17] = np.nan
    s = device_matrix(host, 1)
    i, j = np.divmod(np.arange(r * c), c)
    for skip in (True, False):
        keep = i != j if skip else np.ones(r * c, bool)
        trials = TrialList(i[keep], j[keep], rows[i[keep]] == cols[j[keep]])
        for grid in (0, 1000):
            det = report.det_curve_all_pairs(s, rows, cols, skip_diagonal=skip, grid=grid)
            check_curve(det, host, trials, grid, f"all pairs skip {skip} grid {grid}")
        assert det.n_nan == (1 if skip else 2)


PATTERNS = ["equal", "distinct", "runs", "zeros", "left_out", "targets_only"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("grid", [0, 1, 4, 1000])
def test_curve_score_patterns_and_grids(pattern, grid):
    from xvector_amd import report
    from xvector_amd.evaluate import TrialList
    rng = np.random.default_rng(len(pattern))
    n = 9000
    tgt = rng.integers(0, 2, n)
    if pattern == "equal":
        scores = np.full(n, 1.25)
    elif pattern == "distinct":
        scores = rng.permutation(n) / 4.0 - 1000.0
    elif pattern == "runs":                                         # runs of 100 equal scores: 4000 .. 4099 and 8100 .. 8199 span block edges
        scores = (np.arange(n) // 100).astype(np.float64)
    elif pattern == "zeros":                                        # -0.0 and +0.0 share a key
        scores = np.where(rng.integers(0, 2, n) == 1, -0.0, 0.0) * 1.0
        scores[::7] = rng.normal(0.0, 1.0, len(scores[::7]))
    elif pattern == "left_out":
        scores = rng.integers(-50, 50, n) / 2.0
        scores[rng.permutation(n)[:300]] = np.nan
    else:
        scores, tgt = rng.integers(-50, 50, n) / 2.0, np.ones(n, dtype=np.int64)
    host, s, trials = listed(scores, tgt)
    if pattern == "left_out":                                       # ... and 200 trials that point outside the matrix
        rows, cols = trials.row_idx.copy(), trials.col_idx.copy()
        out = rng.permutation(n)[:200]
        rows[out[:100]], cols[out[100:]] = host.shape[0] + out[:100], -1 - out[100:]
        trials = TrialList(rows, cols, tgt)
    det = report.det_curve(s, trials, grid)
    check_curve(det, host, trials, grid, f"{pattern} grid {grid}")
    assert len(det.tp) >= 1 and det.tp[-1] == det.n_target and det.nn[-1] == det.n_nontarget      # the last point holds every trial kept
    if pattern == "equal":
        assert len(det.tp) == 1
    if pattern == "zeros":
        assert (det.thresholds.view(np.uint32) != 0x80000000).all()                               # one key: -0.0 reads +0.0
    if pattern == "left_out":
        assert (det.n_nan, det.n_bad_index) == (int(np.isnan(scores[np.setdiff1d(np.arange(n), out)]).sum()), 200)
    if pattern == "targets_only":                                   # the counts stand, the rate without a class is NaN (include/xvec_eval.h)
        assert det.n_nontarget == 0 and np.isnan(det.far).all() and det.frr[-1] == 1.0
    else:
        assert (np.diff(det.frr) >= 0).all() and (np.diff(det.far) <= 0).all()                    # both rates monotone, thinned or not


@pytest.mark.parametrize("skip_diagonal", [True, False])
def test_curve_of_all_pairs(skip_diagonal):
    from xvector_amd import report
    from xvector_amd.evaluate import TrialList
    rng = np.random.default_rng(11)
    n = 67
    labels = rng.integers(0, 9, n)
    host = np.round(rng.normal(0.0, 3.0, (n, n)) * 4.0) / 4.0
    host[5, 9] = host[40, 2] = np.nan
    host[7, 7] = np.nan                                             # on the diagonal: counted only when the diagonal is kept
    s = device_matrix(host, 2)
    r, c = np.divmod(np.arange(n * n), n)
    keep = r != c if skip_diagonal else np.ones(n * n, bool)
    trials = TrialList(r[keep], c[keep], labels[r[keep]] == labels[c[keep]])
    for grid in (0, 4, 1000):
        det = report.det_curve_all_pairs(s, labels, skip_diagonal=skip_diagonal, grid=grid)
        check_curve(det, host, trials, grid, f"all pairs grid {grid}")
        assert det.n_nan == (2 if skip_diagonal else 3)
    two = report.det_curve_all_pairs(s[:, :40], labels, labels[:40], skip_diagonal=False)      # two sets: rows against other columns
    check_curve(two, host[:, :40], TrialList(*np.divmod(np.arange(n * 40), 40), (labels[:, None] == labels[None, :40]).reshape(-1)), 0, "two sets")


def test_curve_reproduces_the_evaluator_s_operating_points():
    from xvector_amd import evaluate as ev, report
    for seed, (n_pos, n_neg, levels) in enumerate(((40, 60, 0), (700, 2300, 64), (3000, 34720, 16))):
        pos, neg = eer_ref.draw(np.random.default_rng(seed), n_pos, n_neg, levels or None)
        host, s, trials = listed(np.r_[pos, neg], np.r_[np.ones(n_pos, int), np.zeros(n_neg, int)], width=411)
        det = report.det_curve(s, trials)
        # costs and a prior that are powers of two: every product of the evaluator's cost is exact, so its sum rounds once
        # whether or not the device fuses it, and numpy's fp64 repeats it
        for c_miss, c_fa in ((1.0, 1.0), (4.0, 1.0)):
            res = ev.evaluate_trials(s, trials, c_miss, c_fa, 0.5)
            assert det.eer() == (res.eer, res.eer_th), (seed, det.eer(), res)
            assert det.min_dcf(c_miss, c_fa, 0.5) == (res.min_dcf, res.min_dcf_th), (seed, det.min_dcf(c_miss, c_fa, 0.5), res)
        thin = report.det_curve(s, trials, grid=50)
        assert thin.thresholds[0] == det.thresholds[0] and thin.thresholds[-1] == det.thresholds[-1]      # first and last stay
        assert len(thin.tp) <= 102 and (np.diff(thin.frr) >= 0).all() and (np.diff(thin.far) <= 0).all()
        rep = report.trial_report(s, trials, grid=50, which=report.GROUND_TRUTH)
        assert rep.result == ev.evaluate_trials(s, trials) and list(rep.images) == ["ground_truth"]
        assert np.array_equal(rep.det.tp, thin.tp)


def test_repeatable_on_any_stream_with_an_exact_and_a_poisoned_workspace():
    from xvector_amd import hip, report
    rng = np.random.default_rng(4)
    n = 9000
    scores, tgt = rng.integers(-400, 400, n) / 4.0, rng.integers(0, 2, n)
    host, s, trials = listed(scores, tgt)
    first = report.det_curve(s, trials, 16)
    need = int(hip.lib.xvec_report_det_workspace_bytes(n))
    same = lambda d: all(np.array_equal(getattr(d, f), getattr(first, f)) for f in ("thresholds", "tp", "nn")) and d.n_target == first.n_target
    assert same(report.det_curve(s, trials, 16))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)           # exactly the reported size, poisoned
    assert same(report.det_curve(s, trials, 16, workspace=ws))
    ws.fill_(0x5A)
    images = report.score_images(s, trials, 1.0, 2.0)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        assert same(report.det_curve(s, trials, 16, workspace=ws))
        again = report.score_images(s, trials, 1.0, 2.0)
    stream.synchronize()
    for name, img in images.items():
        assert torch.equal(img, again[name]), name
    # the range's workspace: exactly the reported size, poisoned
    rws = torch.full((int(hip.lib.xvec_report_range_workspace_bytes()),), 0xFF, dtype=torch.uint8, device=DEV)
    rec = torch.empty(3, dtype=torch.float64, device=DEV)
    assert hip.lib.xvec_report_range(s.data_ptr(), s.stride(0), s.shape[0], s.shape[1], rec.data_ptr(), rws.data_ptr(), rws.numel(),
                                     torch.cuda.current_stream(DEV).cuda_stream) == 0
    assert rec[:2].tolist() == [np.nanmin(host), np.nanmax(host)] and report.score_range(s)[2] == int(np.isnan(host).sum())
