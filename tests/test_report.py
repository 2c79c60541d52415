"""CPU-only checks of the trial report (include/xvec_report.h, xvector_amd.report): the numpy restatement tests/report_ref.py
on cases worked by hand; the host-only plan (csrc/report_plan.h) through its dump program -- the tiling of the image pass, the
map from a wide image's column to its panel at both panel edges and in the gap, the split of a row's piece into ragged ends
and aligned body, the thinning rule, the workspace layout, the argument checks; the exports, the module's constants, and what
the entry points answer to bad arguments and to a null or short workspace (each returns before the library touches a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import report_ref
from conftest import ROOT
from hipcc_support import header_constants, host_program, needs_host_cxx

P, Q = 0x1000, 0x2000      # pointers that are never followed


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return host_program("report_plan_dump", tmp_path_factory.mktemp("report_plan"))


# ---------------------------------------------------------------- the restatement, by hand

def test_restatement_on_a_case_worked_by_hand():
    S = np.array([[1.0, 3.0, 5.0], [2.0, np.nan, -3.0]])
    # cell (0, 1): a target; (0, 2): a target and a non-target (K = 2); (1, 2): a non-target; (5, 0): outside
    pos, neg, bad = report_ref.masks([0, 0, 0, 5], [1, 2, 2, 0], [1, 1, 0, 1], S.shape)
    neg[1, 2] = 1
    assert bad == 1 and pos.tolist() == [[0, 1, 1], [0, 0, 0]] and neg.tolist() == [[0, 0, 1], [0, 0, 1]]
    assert report_ref.finite_range(S) == (-3.0, 5.0)
    img = report_ref.images(S, pos, neg, 4.0, 12.0)
    norm = img["score_matrix"][0]
    assert norm[0].tolist() == [0.5, 0.75, 1.0] and norm[1, 0] == 0.625 and np.isnan(norm[1, 1]) and norm[1, 2] == 0.0
    assert [img[n].shape for n in report_ref.NAMES] == [(3, 2, 3)] * 3 + [(3, 2, 11)] * 3
    pred = img["prediction_eer_min_dcf"]
    # left panel, t = 4: cv = [3, 10 (= 2 * 5), -3]: the target at 3 is rejected, the K = 2 cell accepted with the value 2
    assert pred[1, :, :3].tolist() == [[0, 0, 2], [0, 0, 0]] and pred[0, :, :3].tolist() == [[0, 1, 0], [0, 0, 1]]
    # right panel, t = 12 lies above every cv: everything is rejected, the K = 2 cell with the value 2
    assert pred[1, :, -3:].tolist() == [[0, 0, 0], [0, 0, 0]] and pred[0, :, -3:].tolist() == [[0, 1, 2], [0, 0, 1]]
    assert (pred[:, :, 3:8] == 1).all() and (pred[2, :, :3] == 0).all() and (pred[2, :, -3:] == 0).all()
    cor, fal = img["correct_prediction_eer_min_dcf"], img["false_prediction_eer_min_dcf"]
    assert cor[1, :, :3].tolist() == [[0, 0, 2], [0, 0, 0]] and cor[0, :, :3].tolist() == [[0, 0, 0], [0, 0, 1]]
    assert fal[1, :, :3].tolist() == [[0, 0, 2], [0, 0, 0]] and fal[0, :, :3].tolist() == [[0, 1, 0], [0, 0, 0]]
    assert report_ref.to_u8(np.array([0.0, 0.5, 1.0, 2.0, -1.0, np.nan, np.inf, -np.inf, 0.999])).tolist() == [
        0, 127, 255, 255, 0, 0, 255, 0, 254]
    gts = report_ref.as_dtype(img["ground_truth_scores"], np.float32)
    assert gts[1, 0].tolist() == [0.0, 0.75, 1.0] and np.isnan(gts[1, 1, 1]) and gts[0, 1, 2] == 0.0
    # a constant matrix: 0 / 0 everywhere, as numpy
    assert np.isnan(report_ref.normalised(np.full((2, 2), 7.0))).all()


def test_curve_restatement_on_a_case_worked_by_hand():
    thr, tp, nn, n_pos, n_neg = report_ref.det_points([1.0, 2.0, 2.0, -0.0, 0.0, 3.0], [0, 1, 0, 1, 0, 1])
    assert thr.dtype == np.float32 and thr.tolist() == [0.0, 1.0, 2.0, 3.0]
    assert tp.tolist() == [1, 1, 2, 3] and nn.tolist() == [1, 2, 3, 3] and (n_pos, n_neg) == (3, 3)
    s, t, n_nan, n_bad = report_ref.select(np.array([[1.0, np.nan]]), [0, 0, 0, 1], [0, 1, 2, 0], [1, 0, 1, 0])
    assert s.tolist() == [1.0] and t.tolist() == [True] and (n_nan, n_bad) == (1, 2)
    # ten points, P = N = 10, tp = nn = 1 .. 10: with grid 2 the steps of floor(2 tp / 10) are at tp = 5 and 10, those of
    # floor(2 (10 - nn) / 10) at nn = 1 (2 -> 1), 6 (1 -> 0): the points 0, 4, 5, 9
    k = np.arange(1, 11)
    assert report_ref.thin(k.astype(np.float32), k, k, 10, 10, 2)[1].tolist() == [1, 5, 6, 10]
    assert report_ref.thin(k.astype(np.float32), k, k, 10, 10, 0)[1].tolist() == k.tolist()
    assert len(report_ref.thin(k.astype(np.float32), k, k, 10, 10, 1)[0]) <= 4


# ---------------------------------------------------------------- the host-only plan

@needs_host_cxx
def test_plan_constants_are_the_headers_and_the_modules(plan):
    from xvector_amd import report
    consts = header_constants("xvec_report.h", "XVEC_REPORT_")
    threads, tile, range_blocks, range_tile, det_items, det_tile, gap, chunk, max_planes = (int(v) for v in plan(["const"])[0].split()[1:])
    assert (threads, tile, range_blocks, det_items, det_tile, gap) == (consts["THREADS"], consts["TILE"], consts["RANGE_BLOCKS"],
                                                                       consts["DET_ITEMS"], consts["DET_TILE"], consts["GAP"])
    assert (report.THREADS, report.TILE, report.RANGE_BLOCKS, report.DET_ITEMS, report.DET_TILE, report.GAP) == (
        threads, tile, range_blocks, det_items, det_tile, gap)
    assert det_tile == threads * det_items and range_tile == 4 * threads and chunk == 16 and max_planes == 1 + 3 + 3 + 18
    assert (report.U8, report.F32) == (consts["U8"], consts["F32"]) == (0, 1)
    bits = [consts[n] for n in ("SCORE_MATRIX", "GROUND_TRUTH", "GROUND_TRUTH_SCORES", "PREDICTION", "CORRECT", "FALSE")]
    assert bits == [1, 2, 4, 8, 16, 32] == [report.SCORE_MATRIX, report.GROUND_TRUTH, report.GROUND_TRUTH_SCORES, report.PREDICTION,
                                            report.CORRECT, report.FALSE]
    assert consts["ALL"] == report.ALL == 63 and report.IMAGE_NAMES == report_ref.NAMES and report_ref.GAP == gap


@needs_host_cxx
def test_tiles_cover_the_matrix(plan):
    shapes = [(1, 1), (2, 3), (65, 11), (33, 257), (7, 4095), (7, 4096), (7, 4097), (3, 2049), (4874, 4874), (1, 2 ** 31 - 1),
              (2 ** 31 - 1, 1), (100000, 3)]
    for (r, c), line in zip(shapes, plan([f"tiles {r} {c}" for r, c in shapes])):
        tr, tc, rt, ctl, total = (int(v) for v in line.split()[1:])
        assert tr * tc <= 4096 and tc == min(c, 4096) and tr == (4096 // c if c < 4096 else 1) and tr >= 1, (r, c, line)
        assert (rt - 1) * tr < r <= rt * tr and (ctl - 1) * tc < c <= ctl * tc and total == rt * ctl, (r, c, line)
        assert tr == 1 or ctl == 1                                   # a tile of several rows holds them whole


@needs_host_cxx
@pytest.mark.parametrize("c", [1, 3, 11, 64, 65])
def test_wide_columns_map_to_their_panels(plan, c):
    ws = list(range(2 * c + 5))
    got = [tuple(int(v) for v in line.split()[1:]) for line in plan([f"wide {c} {w}" for w in ws])]
    for w, (panel, cell, first) in zip(ws, got):
        assert first + cell == w                                     # the panel's first column plus the cell is the column
        if w < c:
            assert (panel, cell) == (0, w)
        elif w < c + 5:
            assert (panel, cell) == (1, w - c)
        else:
            assert (panel, cell) == (2, w - c - 5)
    # both edges of both panels and the whole gap, spelt out
    assert got[0] == (0, 0, 0) and got[c - 1] == (0, c - 1, 0)
    assert [g[:2] for g in got[c:c + 5]] == [(1, k) for k in range(5)]
    assert got[c + 5] == (2, 0, c + 5) and got[2 * c + 4] == (2, c - 1, c + 5)


@needs_host_cxx
def test_pieces_split_into_ragged_ends_and_an_aligned_body(plan):
    asked = [(a, a + n) for a in range(4096, 4096 + 33) for n in list(range(0, 50)) + [4874, 9753]]
    for (a, b), line in zip(asked, plan([f"piece {a} {b}" for a, b in asked])):
        body, tail = (int(v) for v in line.split()[1:])
        assert a <= body <= tail <= b, (a, b, line)
        assert body - a < 16 and b - tail < 16, (a, b, line)         # the ends are shorter than a piece
        if tail > body:
            assert body % 16 == 0 and tail % 16 == 0, (a, b, line)   # the body is whole aligned pieces
        else:
            assert b - a < 31, (a, b, line)                          # no body: the piece holds no aligned 16 bytes
        assert (tail - body) // 16 == max(0, b // 16 - -(-a // 16)), (a, b, line)      # ... and every one it holds is in the body


@needs_host_cxx
def test_thinning_rule_on_hand_made_counts(plan):
    assert plan(["step 5 10 2", "step 4 10 2", "step 10 10 2", "step 3 0 7", f"step {2 ** 31 - 1} {2 ** 31 - 1} {2 ** 31 - 1}",
                 f"step {2 ** 31 - 2} {2 ** 31 - 1} {2 ** 31 - 1}"]) == [
        "step 1", "step 0", "step 2", "step 0", f"step {2 ** 31 - 1}", f"step {2 ** 31 - 2}"]
    rng = np.random.default_rng(3)
    for n_pos, n_neg, grid in ((10, 10, 2), (7, 0, 4), (0, 9, 4), (37, 91, 1), (37, 91, 4), (37, 91, 1000), (500, 300, 16)):
        tgt = np.r_[np.ones(n_pos, bool), np.zeros(n_neg, bool)]
        s = rng.integers(0, 40, n_pos + n_neg).astype(np.float64)
        thr, tp, nn, P_, N_ = report_ref.det_points(s, tgt)
        asked = [f"keep {tp[k]} {nn[k]} {tp[k - 1] if k else 0} {nn[k - 1] if k else 0} {P_} {N_} {grid} {int(k == 0)} {int(k == len(thr) - 1)}"
                 for k in range(len(thr))]
        kept = [k for k, line in enumerate(plan(asked)) if line == "keep 1"]
        want = report_ref.thin(thr, tp, nn, P_, N_, grid)
        assert thr[kept].tolist() == want[0].tolist() and len(kept) <= 2 * grid + 2, (n_pos, n_neg, grid)
        assert kept[0] == 0 and kept[-1] == len(thr) - 1
    assert plan(["keep 3 3 3 2 10 10 0 0 0", "keep 3 3 3 3 10 10 5 0 0"]) == ["keep 1", "keep 0"]      # grid 0 keeps everything


def _counts():
    return sorted({1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 37720, 4096 * 256 - 1, 4096 * 256,
                   4096 * 256 + 1, 4874 * 4874, 2 ** 31 - 1})


@needs_host_cxx
def test_workspace_regions_are_aligned_disjoint_and_hold_the_sort_window(plan):
    from xvector_amd import hip
    ns = _counts()
    ev = [hip.lib.xvec_eval_workspace_bytes(n) for n in ns]
    for n, e, line in zip(ns, ev, plan([f"layout {n} {e}" for n, e in zip(ns, ev)])):
        v = [int(t) for t in line.split()[1:]]
        offs, total, blocks = v[:12], v[12], v[13]
        assert e > 0 and blocks == -(-n // 4096)
        sizes = [256, e, 4 * n, n, 4 * n, 4 * n, n, 12 * blocks, 4 * blocks, 4 * n, 4 * n, 4 * n]
        assert offs[0] == 0 and all(o % 256 == 0 for o in offs), (n, line)
        for k in range(len(offs) - 1):
            assert offs[k] + sizes[k] <= offs[k + 1] < offs[k] + sizes[k] + 256, (n, k, line)
        assert offs[2] - offs[1] == e                                         # the sort's window is exactly what it asks for
        assert offs[-1] + sizes[-1] <= total < offs[-1] + sizes[-1] + 256, (n, line)
        assert hip.lib.xvec_report_det_workspace_bytes(n) == total, n
    for bad in (0, -1, 2 ** 31, 2 ** 40):
        assert hip.lib.xvec_report_det_workspace_bytes(bad) == 0, bad
    assert plan(["layout 0 256", "layout 10 0"]) == ["layout" + " 0" * 14] * 2
    shapes = [(1, 1), (1, 1024), (1, 1025), (1023, 1024), (1024, 1024), (1025, 7), (4874, 4874), (2 ** 31 - 1, 2 ** 31 - 1)]
    for (r, c), line in zip(shapes, plan([f"range {r} {c}" for r, c in shapes])):
        col_tiles, blocks, nbytes = (int(v) for v in line.split()[1:])
        assert col_tiles == -(-c // 1024) and blocks == min(r * col_tiles, 1024) and nbytes == 1024 * 24, (r, c, line)
    assert hip.lib.xvec_report_range_workspace_bytes() == 1024 * 24


@needs_host_cxx
def test_argument_checks_of_the_plan(plan):
    asked = ["tmap 4 1 3 4 4 0", "tmap 0 0 3 4 4 0", "tmap 4 0 3 4 4 0", "tmap -1 1 3 4 4 0", f"tmap {2 ** 31} 1 3 4 4 0", "tmap 4 1 0 4 4 0",
             "tmap 4 1 3 5 4 0", "tmap 4 1 3 4 6 0", "tmap 4 1 3 4 4 2", "tmap 4 1 3 5 8 0",
             "images 4 3 4 4 63 0 -1 3", "images 4 3 4 4 63 1 -1 4", "images 4 3 4 4 63 1 -1 3", "images 3 3 4 4 63 0 -1 0",
             "images 4 3 4 3 63 0 -1 0", "images 4 3 4 6 63 0 -1 0", "images 4 3 4 4 0 0 -1 0", "images 4 3 4 4 64 0 -1 0",
             "images 4 3 4 4 63 2 -1 0", "images 4 3 4 4 63 -1 -1 0", "images 4 3 4 4 63 0 4 0", "images 4 3 4 4 47 0 4 0",
             "images 4 -3 4 4 63 0 -1 0", f"images {2 ** 31 - 1} {2 ** 31 - 1} {2 ** 31 - 1} {2 ** 31} 1 0 -1 0",
             "curve 0 1 0 0", "curve 1000 1 5 1", "curve -1 1 0 0", f"curve {2 ** 31} 1 0 0", "curve 0 0 0 0", "curve 0 1 -1 1",
             "curve 0 1 5 0",
             "trials 4 1 4 0 4", "trials 4 1 4 0 0", "trials 4 1 3 0 4", f"trials 4 1 4 0 {2 ** 31}", "trials 3 2 4 1 9", "trials 4 2 4 0 3",
             "pairs 4 3 4", "pairs 65536 65536 65536", "pairs 4 0 4"]
    got = plan(asked)
    verdict = {a: g.split()[0] for a, g in zip(asked, got)}
    ok = {"tmap 4 1 3 4 4 0", "tmap 0 0 3 4 4 0", "tmap 4 1 3 5 8 0", "images 4 3 4 4 63 0 -1 3", "images 4 3 4 4 63 1 -1 4",
          "images 4 3 4 4 47 0 4 0", "curve 0 1 0 0", "curve 1000 1 5 1", "trials 4 1 4 0 4", "pairs 4 3 4"}
    large = {f"tmap {2 ** 31} 1 3 4 4 0", f"images {2 ** 31 - 1} {2 ** 31 - 1} {2 ** 31 - 1} {2 ** 31} 1 0 -1 0",
             f"trials 4 1 4 0 {2 ** 31}", "pairs 65536 65536 65536"}
    for a, g in zip(asked, got):
        assert verdict[a] == ("ok" if a in ok else "toolarge" if a in large else "refused"), (a, g)
    text = dict(zip(asked, got))
    assert "ld_map = 6" in text["tmap 4 1 3 4 6 0"] and "4-byte aligned" in text["tmap 4 1 3 4 4 2"]
    assert "which = 0x40" in text["images 4 3 4 4 64 0 -1 0"] and "dtype = 2" in text["images 4 3 4 4 63 2 -1 0"]
    assert "correct_prediction is selected" in text["images 4 3 4 4 63 0 4 0"]
    assert "float32 image must be 4-byte aligned" in text["images 4 3 4 4 63 1 -1 3"]


# ---------------------------------------------------------------- the header, the module and the C ABI without a device

EXPORTS = {"xvec_report_last_error", "xvec_report_trial_map", "xvec_report_range_workspace_bytes", "xvec_report_range",
           "xvec_report_images", "xvec_report_det_workspace_bytes", "xvec_report_det", "xvec_report_det_all_pairs"}


def _header_signatures():
    """{function: (return type, [parameter type, ...])} of include/xvec_report.h."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xvec_report.h")).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\n([a-z_0-9 ]+?\**)\s*(xvec_report_\w+)\s*\(([^)]*)\)\s*;", src):
        types = []
        for prm in (p.strip() for p in params.split(",")):
            if prm != "void":
                types.append(re.sub(r"\s*\w+$", "", prm).replace("const ", "").strip())
        out[name] = (ret.replace("const ", "").strip(), types)
    return out


def test_exports_and_python_signatures_match_the_header():
    import xvector_amd
    from xvector_amd import evaluate, hip, report
    sigs = _header_signatures()
    assert set(sigs) == EXPORTS <= set(hip.EXPORTS) and all(hasattr(hip.lib, n) for n in EXPORTS)
    ctype = {"int64_t": {C.c_int64}, "int32_t": {C.c_int32}, "uint32_t": {C.c_uint32}, "double": {C.c_double},
             "size_t": {C.c_size_t, hip._wsb_report}, "xvec_stream": {C.c_void_p}}
    for name, (ret, types) in sigs.items():
        res, args = hip._SIGS[name]
        assert res is {"char*": C.c_char_p, "size_t": C.c_size_t, "int": C.c_int}[ret], name
        assert len(args) == len(types), name
        for a, t in zip(args, types):
            assert a in (ctype[t] if t in ctype else {C.c_void_p}) and (t in ctype or t.endswith("*")), (name, t, a)
    assert C.sizeof(hip._wsb_report) == C.sizeof(C.c_size_t) and issubclass(hip._wsb_report, hip._wsb)
    assert (C.sizeof(report._Range), C.sizeof(report._Header)) == (24, 40)
    for name in ("DetCurve", "TrialReport", "trial_map", "score_range", "score_images", "det_curve", "det_curve_all_pairs",
                 "trial_report"):
        assert getattr(xvector_amd, name) is getattr(report, name) and name in xvector_amd.__all__
    for name in ("score_images", "det_curve", "write_images", "plot_images"):
        assert callable(getattr(evaluate.plda_score_stat_object, name))
    import torch
    cpu = torch.zeros(3, 3, dtype=torch.float64)
    trials = xvector_amd.TrialList([0, 1], [1, 2], [1, 0])
    for call in (lambda: report.score_images(cpu, trials, 0.0, 0.0), lambda: report.score_range(cpu),
                 lambda: report.det_curve(cpu, trials), lambda: report.det_curve_all_pairs(cpu, [0, 0, 1]),
                 lambda: report.trial_report(cpu, trials), lambda: report.trial_map(trials, (3, 3), "cpu")):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()


def test_det_curve_rates_and_operating_points_from_the_points():
    from xvector_amd.report import DetCurve
    thr, tp, nn, n_pos, n_neg = report_ref.det_points([1.0, 2.0, 2.0, 0.0, 0.0, 3.0, 4.0], [0, 1, 0, 1, 0, 1, 0])
    det = DetCurve(thr, tp, nn, n_pos, n_neg, 0, 0)
    assert det.frr.tolist() == [1 / 3, 1 / 3, 2 / 3, 1.0, 1.0] and det.far.tolist() == [0.75, 0.5, 0.25, 0.25, 0.0]
    import eer_ref
    s, t = np.array([1.0, 2.0, 2.0, 0.0, 0.0, 3.0, 4.0]), np.array([0, 1, 0, 1, 0, 1, 0], bool)
    ref = eer_ref.by_sort(s[t], s[~t], p_target=0.5)
    assert det.eer() == (ref.eer, ref.eer_th) and det.min_dcf() == (ref.min_dcf, ref.min_dcf_th)
    only = DetCurve(thr[:2], np.array([1, 2]), np.array([0, 0]), 2, 0, 0, 0)      # targets only: the counts stand, the rate is NaN
    assert only.frr.tolist() == [0.5, 1.0] and np.isnan(only.far).all()
    with pytest.raises(ValueError, match="both kinds"):
        only.eer()


WS, WSB = object(), object()
# entry point: (the size query and its arguments, the smallest valid arguments with the workspace and its size marked)
CALLS = {
    "xvec_report_range": (("xvec_report_range_workspace_bytes", ()), (P, 1, 1, 1, P, WS, WSB, None)),
    "xvec_report_det": (("xvec_report_det_workspace_bytes", (1,)), (P, 1, 1, 1, None, None, P, 1, 0, P, None, None, None, 0, WS, WSB, None)),
    "xvec_report_det_all_pairs": (("xvec_report_det_workspace_bytes", (1,)), (P, 1, 1, 1, P, P, 0, 0, P, None, None, None, 0, WS, WSB, None)),
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_null_and_short_workspaces_are_refused(name):
    """The style of tests/test_workspace_refusals.py: XVEC_ERR_ARG "null pointer: workspace" for a null workspace,
    XVEC_ERR_WORKSPACE "workspace too small: <have> < <need> bytes" for one a byte short; nothing is launched."""
    from xvector_amd import hip
    takes = {n for n, (_, a) in hip._SIGS.items() if any(x is hip._wsb_report and a[i - 1] is C.c_void_p for i, x in enumerate(a))}
    assert takes == set(CALLS)
    (size_fn, size_args), args = CALLS[name]
    need = getattr(hip.lib, size_fn)(*size_args)
    assert need >= 256 and need % 256 == 0

    def answer(ws, size):
        rc = getattr(hip.lib, name)(*[ws if a is WS else size if a is WSB else a for a in args])
        return rc, hip.lib.xvec_report_last_error().decode()
    assert answer(None, need) == (hip.ERR_ARG, "null pointer: workspace")
    assert answer(P, need - 1) == (hip.ERR_WORKSPACE, f"workspace too small: {need - 1} < {need} bytes")


def test_c_abi_argument_errors_return_before_any_device_call():
    from xvector_amd import hip
    lib, err = hip.lib, lambda: hip.lib.xvec_report_last_error().decode()
    A = hip.ERR_ARG
    # trial map: null pointers, negative sizes, a short or ragged row stride, a misaligned map
    assert lib.xvec_report_trial_map(None, P, P, 4, 3, 4, P, 4, None, None) == A and "row_idx / col_idx / is_target" in err()
    assert lib.xvec_report_trial_map(P, P, P, 4, 3, 4, None, 4, None, None) == A and err() == "xvec_report_trial_map: null pointer: map"
    assert lib.xvec_report_trial_map(P, P, P, -1, 3, 4, P, 4, None, None) == A and "n_trials = -1" in err()
    assert lib.xvec_report_trial_map(P, P, P, 4, -3, 4, P, 4, None, None) == A and "score matrix [-3, 4]" in err()
    assert lib.xvec_report_trial_map(P, P, P, 4, 3, 5, P, 4, None, None) == A and "ld_map = 4 is smaller than n_cols = 5" in err()
    assert lib.xvec_report_trial_map(P, P, P, 4, 3, 4, P + 1, 4, None, None) == A and "4-byte aligned" in err()
    assert lib.xvec_report_trial_map(P, P, P, 2 ** 31, 3, 4, P, 4, None, None) == hip.ERR_TOO_LARGE
    # range
    need = lib.xvec_report_range_workspace_bytes()
    assert lib.xvec_report_range(None, 4, 3, 4, P, P, need, None) == A and err() == "xvec_report_range: null pointer: scores"
    assert lib.xvec_report_range(P, 3, 3, 4, P, P, need, None) == A and "ld = 3 is smaller than n_cols = 4" in err()
    assert lib.xvec_report_range(P, 4, 0, 4, P, P, need, None) == A and "both sizes" in err()
    assert lib.xvec_report_range(P, 4, 3, 4, None, P, need, None) == A and "null pointer: out" in err()
    # images: every refusal comes before the launch
    img = lambda *a, which=63, dtype=0, out=(Q, Q, Q, Q, Q, Q): lib.xvec_report_images(*a, 0.0, 0.0, which, dtype, *out, None)
    assert img(None, 4, 3, 4, P, 4, P) == A and "null pointer: scores" in err()
    assert img(P, 4, 3, 4, None, 4, P) == A and "null pointer: map" in err()
    assert img(P, 4, 3, 4, P, 4, None) == A and "null pointer: range" in err()
    assert img(P, 3, 3, 4, P, 4, P) == A and "ld = 3" in err()
    assert img(P, 4, 3, -4, P, 4, P) == A and "both sizes" in err()
    assert img(P, 4, 3, 4, P, 4, P, which=0) == A and "which = 0x0" in err()
    assert img(P, 4, 3, 4, P, 4, P, which=64) == A and "which = 0x40" in err()
    assert img(P, 4, 3, 4, P, 4, P, dtype=2) == A and "dtype = 2" in err()
    assert img(P, 4, 3, 4, P, 4, P, out=(Q, Q, None, Q, Q, Q)) == A and "ground_truth_scores is selected" in err()
    assert img(P, 4, 3, 4, P, 4, P, dtype=1, out=(Q, Q, Q, Q + 2, Q, Q)) == A and "prediction: a float32 image" in err()
    # the curve
    need = lib.xvec_report_det_workspace_bytes(4)
    det = lambda *a: lib.xvec_report_det(*a, None)
    assert det(None, 4, 1, 4, None, None, P, 4, 0, P, None, None, None, 0, P, need) == A and err() == "xvec_report_det: null pointer: scores"
    assert det(P, 4, 1, 4, None, None, None, 4, 0, P, None, None, None, 0, P, need) == A and "is_target" in err()
    assert det(P, 4, 1, 4, None, None, P, 0, 0, P, None, None, None, 0, P, need) == A and "n_trials = 0" in err()
    assert det(P, 4, 1, 4, None, None, P, 2 ** 31, 0, P, None, None, None, 0, P, need) == hip.ERR_TOO_LARGE
    assert det(P, 3, 1, 4, None, None, P, 4, 0, P, None, None, None, 0, P, need) == A and "ld = 3" in err()
    assert det(P, 4, 1, 4, None, None, P, 4, -1, P, None, None, None, 0, P, need) == A and "grid = -1" in err()
    assert det(P, 4, 1, 4, None, None, P, 4, 0, None, None, None, None, 0, P, need) == A and "header" in err()
    assert det(P, 4, 1, 4, None, None, P, 4, 0, P, None, None, None, 3, P, need) == A and "capacity = 3" in err()
    assert det(P, 4, 1, 4, None, None, P, 4, 0, P, P, P, P, -2, P, need) == A and "capacity = -2" in err()
    assert lib.xvec_report_det_all_pairs(P, 65536, 65536, 65536, P, P, 1, 0, P, None, None, None, 0, P, need, None) == hip.ERR_TOO_LARGE
    assert lib.xvec_report_det_all_pairs(P, 4, 2, 4, None, P, 1, 0, P, None, None, None, 0, P, need, None) == A and "row_class" in err()
