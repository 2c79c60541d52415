"""CPU-only checks of score calibration (include/xvec_calib.h, xvector_amd.calibrate): the numpy restatement tests/calib_ref.py
against the fixture written from scipy and scikit-learn (tests/golden/g12_calib.npz); the properties the GPU tests rely on,
shown on the restatement first; the host-only plan (csrc/calib_plan.h) through its dump program -- the workspace regions are
aligned and disjoint, the window of the sort is exactly what xvec_eval_workspace_bytes reports, the level plan of the hull
reduction terminates for every count; the exports, the module's constants, and what the entry points answer to a null and to a
short workspace (each returns before the library touches a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import calib_ref
import eer_ref
from conftest import ROOT, load_golden
from hipcc_support import header_constants, host_program, needs_host_cxx

P, Q = 0x1000, 0x2000      # pointers that are never followed


@pytest.fixture(scope="module")
def g12():
    return load_golden("g12_calib.npz")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return host_program("calib_plan_dump", tmp_path_factory.mktemp("calib_plan"))


# ---------------------------------------------------------------- the restatement against scipy and scikit-learn

def test_restatement_reproduces_the_fixture(g12):
    g = g12
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g12_calib.npz")) < 100_000
    s, tgt = g["scores"], g["is_target"].astype(bool)
    assert len(s) == 2000 and 500 < tgt.sum() < 1500
    assert -50 < s.mean() < -30 and 20 < s.std() < 40                       # PLDA-like offset and scale
    s32 = s.astype(np.float32)
    assert (np.unique(s32, return_counts=True)[1] > 1).sum() >= 20          # exact ties
    assert s32[tgt].min() < s32[~tgt].max() and s32[~tgt].min() < s32[tgt].max()      # the classes overlap
    for name, p in (("05", 0.5), ("001", 0.01)):
        ref = calib_ref.fit(s, tgt, p)
        assert ref["converged"] and ref["grad"] < 1e-18
        # scipy's stopping point is not exact: its own gradient, taken through the inverse Hessian, times 4
        reach = 4.0 * np.abs(calib_ref.raw_hessian_inverse(ref)).astype(np.float64) @ np.abs(g[f"grad_{name}"])
        got = np.array([float(ref["a"]), float(ref["b"])])
        print(f"p_target {p}: restatement {got}, scipy {g[f'ab_{name}']}, |difference| {np.abs(got - g[f'ab_{name}'])}, reach {reach}")
        assert (np.abs(got - g[f"ab_{name}"]) <= reach + 1e-15).all()
        # and the objective the restatement reports is J at its point
        assert abs(float(ref["J"] - calib_ref.objective(s, tgt, ref["a"], ref["b"], p))) <= 1e-17
    k_end, tp_end = calib_ref.pav(s, tgt)
    order = np.argsort(s32, kind="stable")
    assert np.abs(calib_ref.pav_values(k_end, tp_end).astype(np.float64) - g["isotonic"][order]).max() <= 1e-12
    by_segments = calib_ref.min_cllr_from_segments(k_end, tp_end)[0]
    by_trials = calib_ref.min_cllr_from_values(g["isotonic"][order], tgt[order])
    assert abs(float(by_segments - by_trials)) <= 1e-12
    fitted = calib_ref.fit(s, tgt, 0.5)
    assert float(by_segments) <= float(calib_ref.cllr(fitted["a"] * s.astype(calib_ref.LD) + fitted["b"], tgt))
    # objective_bits at p_target = 0.5 is Cllr of the fitted map
    assert abs(float(fitted["J"] / calib_ref.LN2 - calib_ref.cllr(fitted["a"] * s.astype(calib_ref.LD) + fitted["b"], tgt))) <= 1e-15


def test_pav_restatement_on_the_shapes_the_gpu_test_uses():
    one = lambda s, t: [v.tolist() for v in calib_ref.pav(np.asarray(s, dtype=np.float64), np.asarray(t))]
    assert one([3.0] * 7, [1, 0, 1, 1, 0, 0, 1]) == [[7], [4]]                                  # all equal: one segment
    assert float(calib_ref.min_cllr_from_segments(*calib_ref.pav(np.full(7, 3.0), np.array([1, 0, 1, 1, 0, 0, 1])))[0]) == 1.0
    assert one([1, 2, 3, 4, 5], [0, 0, 1, 1, 1]) == [[2, 5], [0, 3]]                            # separated: two segments, cost 0
    assert float(calib_ref.min_cllr_from_segments(np.array([2, 5]), np.array([0, 3]))[0]) == 0.0
    assert one([1, 2, 3, 4, 5], [1, 1, 0, 0, 0]) == [[5], [2]]                                  # reversed: one segment
    assert one([1, 2, 3, 4, 5, 6], [1, 0, 1, 0, 1, 0]) == [[6], [3]]                            # collinear runs are dropped
    s, t = strictly_convex(5)
    k, tp = calib_ref.pav(s, t)
    assert k.tolist() == [2, 5, 9, 14, 20] and tp.tolist() == [0, 1, 3, 6, 10]                 # every tie group a vertex


def strictly_convex(groups):
    """Tie group j = 1 .. groups has j + 1 trials, j - 1 of them targets: the share of targets (j - 1) / (j + 1) rises strictly,
    so every group is a vertex of the minorant."""
    s = np.concatenate([np.full(j + 1, float(j)) for j in range(1, groups + 1)])
    t = np.concatenate([np.r_[np.ones(j - 1, bool), np.zeros(2, bool)] for j in range(1, groups + 1)])
    return s, t


def test_reference_properties_the_gpu_tests_rely_on():
    rng = np.random.default_rng(5)
    for n_t, n_n in ((40, 60), (300, 701)):
        l, tgt = calib_ref.grid_llrs(rng, n_t, n_n)
        assert np.array_equal(l.astype(np.float32).astype(np.float64), l)
        for c_miss, c_fa, p in ((1.0, 1.0, 0.5), (1.0, 1.0, 0.01), (10.0, 1.0, 0.05)):
            act = calib_ref.act_dcf(l, tgt, c_miss, c_fa, p)[0]
            assert act >= calib_ref.min_dcf(l, tgt, c_miss, c_fa, p)
            assert calib_ref.min_dcf(l, tgt, c_miss, c_fa, p) == eer_ref.by_sort(l[tgt], l[~tgt], c_miss, c_fa, p).min_dcf
    assert float(calib_ref.cllr(np.zeros(9), np.arange(9) % 2 == 0)) == 1.0
    assert calib_ref.act_dcf(np.array([0.0, 1.0, -1.0]), np.array([True, True, False]))[1] == 0.5      # a target AT the threshold is missed
    # the end-to-end claims, on a planted-speaker matrix: the fit lowers Cllr, and a > 0 keeps the order and with it the EER
    x, labels = calib_ref.planted(8, 6, 24, seed=3)
    S = calib_ref.planted_scores(x)
    s, tgt, _, _ = calib_ref.select_all_pairs(S, labels, labels, True)
    ref = calib_ref.fit(s, tgt, 0.5)
    a, b = float(ref["a"]), float(ref["b"])
    assert ref["converged"] and a > 0
    assert float(calib_ref.cllr(a * s + b, tgt)) < float(calib_ref.cllr(s, tgt))
    cal = a * s + b
    assert eer_ref.by_sort(cal[tgt], cal[~tgt]).eer == eer_ref.by_sort(s[tgt], s[~tgt]).eer


# ---------------------------------------------------------------- the host-only plan

def _counts():
    B, I, G, Cc, F = 256, 8, 1024, 16, 256
    n = {1, 2, 3, B - 1, B, B + 1, B * I - 1, B * I, B * I + 1, B * I * G - 1, B * I * G, B * I * G + 1, 37720, 4874 * 4874,
         2 ** 31 - 1}
    p = 1
    while p <= 2 ** 31:
        n |= {p - 1, p, p + 1, p * F - 1, p * F, p * F + 1}
        p *= Cc
    return sorted(v for v in n if 1 <= v <= 2 ** 31 - 1)


@needs_host_cxx
def test_plan_constants_are_the_headers_and_the_modules(plan):
    from xvector_amd import calibrate
    consts = header_constants("xvec_calib.h", "XVEC_CALIB_")
    threads, items, max_blocks, chunk, final, hull_tile, words = (int(v) for v in plan(["const"])[0].split()[1:])
    assert (threads, items, max_blocks, chunk, final) == (consts["THREADS"], consts["ITEMS"], consts["MAX_BLOCKS"],
                                                          consts["HULL_CHUNK"], consts["HULL_FINAL"])
    assert (calibrate.THREADS, calibrate.ITEMS, calibrate.MAX_BLOCKS, calibrate.HULL_CHUNK, calibrate.HULL_FINAL,
            calibrate.TERM_ULPS, calibrate.APPLY_ROWS, calibrate.APPLY_COLS) == (threads, items, max_blocks, chunk, final,
                                                                                 consts["TERM_ULPS"], consts["APPLY_ROWS"],
                                                                                 consts["APPLY_COLS"])
    assert hull_tile == threads * chunk and words == 8 and final <= threads and max_blocks % threads == 0
    assert (calibrate.CONVERGED, calibrate.MAX_ITER_REACHED, calibrate.ONE_CLASS, calibrate.INF_SCORE) == (
        consts["CONVERGED"], consts["MAX_ITER"], consts["ONE_CLASS"], consts["INF_SCORE"]) == (0, 1, 2, 3)


@needs_host_cxx
def test_pass_blocks_and_the_depth_of_the_sums(plan):
    ns = _counts()
    for n, line in zip(ns, plan([f"blocks {n}" for n in ns])):
        blocks, depth = (int(v) for v in line.split()[1:])
        assert blocks == min(-(-n // 2048), 1024) and depth == -(-n // (blocks * 256)) + 22, (n, line)


@needs_host_cxx
def test_hull_level_plan_terminates_for_every_count(plan):
    ns = _counts()
    Cc, F = 16, 256
    for n, line in zip(ns, plan([f"hull {n}" for n in ns])):
        v = [int(t) for t in line.split()[1:]]
        levels, pairs = v[0], list(zip(v[1::2], v[2::2]))
        assert 1 <= levels == len(pairs) <= 6, (n, line)
        groups = n
        for l, (g, span) in enumerate(pairs, 1):
            groups = -(-groups // Cc)
            assert g == groups and span == Cc ** l and (g - 1) * span < n <= g * span, (n, line)      # the groups tile the trials
            assert (g <= F) == (l == levels), (n, line)                                               # stops as soon as one block can finish
    assert plan([f"hull {Cc * F}", f"hull {Cc * F + 1}", f"hull {Cc * Cc * F + 1}"]) == [
        f"hull 1 {F} {Cc}", f"hull 2 {F + 1} {Cc} 17 {Cc * Cc}", f"hull 3 {Cc * F + 1} {Cc} {F + 1} {Cc * Cc} 17 {Cc ** 3}"]
    assert plan(["hull 0", "hull -3", f"hull {2 ** 31}"]) == ["refused"] * 3


@needs_host_cxx
def test_workspace_regions_are_aligned_disjoint_and_hold_the_sort_window(plan):
    from xvector_amd import hip
    ns = _counts()
    ev = [hip.lib.xvec_eval_workspace_bytes(n) for n in ns]
    for n, e, line in zip(ns, ev, plan([f"layout {n} {e}" for n, e in zip(ns, ev)])):
        v = [int(t) for t in line.split()[1:]]
        offs, total, hull_blocks = v[:10], v[10], v[11]
        g1 = -(-n // 16)
        g2 = -(-g1 // 16) if g1 > 256 else 0
        sizes = [256, 1024 * 8 * 8, 8 * n, n, e, 4 * n, n, 8 * n, 8 * hull_blocks, 4 * (g1 + g2)]
        assert e > 0 and hull_blocks == -(-n // 4096)
        assert offs[0] == 0 and all(o % 256 == 0 for o in offs), (n, line)
        for k in range(len(offs) - 1):
            assert offs[k] + sizes[k] <= offs[k + 1] < offs[k] + sizes[k] + 256, (n, k, line)
        assert offs[5] - offs[4] == e                                         # the sort's window is exactly what it asks for
        assert offs[-1] + sizes[-1] <= total < offs[-1] + sizes[-1] + 256, (n, line)
        assert hip.lib.xvec_calib_workspace_bytes(n) == total, n
    for bad in (0, -1, 2 ** 31, 2 ** 40):
        assert hip.lib.xvec_calib_workspace_bytes(bad) == 0, bad
    assert plan(["layout 0 256", "layout 10 0"]) == ["layout" + " 0" * 12] * 2


@needs_host_cxx
def test_argument_checks_of_the_plan(plan):
    asked = ["trials 4 1 4 0 4", "trials 4 1 4 0 0", "trials 4 1 3 0 4", f"trials 4 1 4 0 {2 ** 31}", "trials 3 2 4 1 9", "trials 4 2 4 0 3",
             "pairs 4 3 4", "pairs 65536 65536 65536", "pairs 4 0 4", "fit 0.5 50", "fit 0 50", "fit 1 50", "fit 0.5 0", "fit 0.5 1001",
             "fit nan 5", "costs 1 1 0.5", "costs 0 1 0.5", "costs 1 inf 0.5", "costs 1 1 1", "apply 4 3 4 4 1", "apply 4 3 4 5 1",
             "apply 4 3 4 5 0", "apply 3 3 4 4 0", "segments 0 0", "segments 5 1", "segments 5 0", "segments -1 1"]
    got = plan(asked)
    verdict = {a: g.split()[0] for a, g in zip(asked, got)}
    ok = {"trials 4 1 4 0 4", "pairs 4 3 4", "fit 0.5 50", "costs 1 1 0.5", "apply 4 3 4 4 1", "apply 4 3 4 5 0", "segments 0 0",
          "segments 5 1"}
    large = {f"trials 4 1 4 0 {2 ** 31}", "pairs 65536 65536 65536"}
    for a in asked:
        assert verdict[a] == ("ok" if a in ok else "toolarge" if a in large else "refused"), (a, verdict[a])
    assert "n_trials = 0: need at least one trial" in got[1] and "in place (out == scores) needs ld_out == ld" in got[20]


# ---------------------------------------------------------------- the header, the module and the C ABI without a device

EXPORTS = {"xvec_calib_last_error", "xvec_calib_workspace_bytes", "xvec_calib_fit", "xvec_calib_fit_all_pairs", "xvec_calib_apply",
           "xvec_calib_cllr", "xvec_calib_cllr_all_pairs", "xvec_calib_min_cllr"}


def _header_signatures():
    """{function: [parameter type, ...]} of include/xvec_calib.h."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xvec_calib.h")).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\n([a-z_0-9 ]+?\**)\s*(xvec_calib_\w+)\s*\(([^)]*)\)\s*;", src):
        types = []
        for prm in (p.strip() for p in params.split(",")):
            if prm != "void":
                types.append(re.sub(r"\s*\w+$", "", prm).replace("const ", "").strip())
        out[name] = (ret.replace("const ", "").strip(), types)
    return out


def test_exports_and_python_signatures_match_the_header():
    import xvector_amd
    from xvector_amd import calibrate, hip
    sigs = _header_signatures()
    assert set(sigs) == EXPORTS <= set(hip.EXPORTS) and all(hasattr(hip.lib, n) for n in EXPORTS)
    size_t = {C.c_size_t, hip._wsb}
    ctype = {"int64_t": {C.c_int64}, "int32_t": {C.c_int32}, "double": {C.c_double}, "size_t": size_t, "xvec_stream": {C.c_void_p}}
    for name, (ret, types) in sigs.items():
        res, args = hip._SIGS[name]
        assert res is {"char*": C.c_char_p, "size_t": C.c_size_t, "int": C.c_int}[ret], name
        assert len(args) == len(types), name
        for a, t in zip(args, types):
            assert a in (ctype[t] if t in ctype else {C.c_void_p}) and (t in ctype or t.endswith("*")), (name, t, a)
    assert C.sizeof(hip._wsb) == C.sizeof(C.c_size_t) and issubclass(hip._wsb, C.c_size_t)
    # the records the module reads are the header's
    assert (C.sizeof(calibrate._Fit), C.sizeof(calibrate._Cllr), C.sizeof(calibrate._Pav)) == (64, 72, 40)
    assert [f[0] for f in calibrate._Fit._fields_[:2]] == ["a", "b"]
    for name in ("Calibration", "ScoreCalibrator", "CalibrationReport", "fit_calibration", "fit_calibration_all_pairs", "cllr",
                 "min_cllr", "pav_segments", "calibration_report"):
        assert getattr(xvector_amd, name) is getattr(calibrate, name) and name in xvector_amd.__all__
    import torch
    cpu = torch.zeros(3, 3, dtype=torch.float64)
    trials = xvector_amd.TrialList([0, 1], [1, 2], [1, 0])
    for call in (lambda: calibrate.fit_calibration(cpu, trials), lambda: calibrate.fit_calibration_all_pairs(cpu, [0, 0, 1]),
                 lambda: calibrate.cllr(cpu, trials), lambda: calibrate.min_cllr(cpu, trials),
                 lambda: calibrate.calibration_report(cpu, trials), lambda: calibrate.ScoreCalibrator().fit(cpu, trials)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()
    with pytest.raises(ValueError, match="p_target"):
        calibrate.ScoreCalibrator(p_target=1.0)
    with pytest.raises(RuntimeError, match="call fit"):
        calibrate.ScoreCalibrator().calibrate(cpu)


WS, WSB = object(), object()
# entry point: the smallest valid arguments (one trial), the workspace and its size marked
CALLS = {
    "xvec_calib_fit": (P, 1, 1, 1, None, None, P, 1, 0.5, 10, P, WS, WSB, None),
    "xvec_calib_fit_all_pairs": (P, 1, 1, 1, P, P, 0, 0.5, 10, P, WS, WSB, None),
    "xvec_calib_cllr": (P, 1, 1, 1, None, None, P, 1, 1.0, 1.0, 0.05, P, WS, WSB, None),
    "xvec_calib_cllr_all_pairs": (P, 1, 1, 1, P, P, 0, 1.0, 1.0, 0.05, P, WS, WSB, None),
    "xvec_calib_min_cllr": (P, 1, 1, 1, None, None, P, 1, P, None, None, None, None, 0, WS, WSB, None),
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_null_and_short_workspaces_are_refused(name):
    """The style of tests/test_workspace_refusals.py: XVEC_ERR_ARG "null pointer: workspace" for a null workspace,
    XVEC_ERR_WORKSPACE "workspace too small: <have> < <need> bytes" for one a byte short; nothing is launched."""
    from xvector_amd import hip
    takes = {n for n, (_, a) in hip._SIGS.items() if any(x is hip._wsb and a[i - 1] is C.c_void_p for i, x in enumerate(a))}
    assert takes == set(CALLS)
    need = hip.lib.xvec_calib_workspace_bytes(1)
    assert need >= 256 and need % 256 == 0

    def answer(ws, size):
        rc = getattr(hip.lib, name)(*[ws if a is WS else size if a is WSB else a for a in CALLS[name]])
        return rc, hip.lib.xvec_calib_last_error().decode()
    assert answer(None, need) == (hip.ERR_ARG, "null pointer: workspace")
    assert answer(P, need - 1) == (hip.ERR_WORKSPACE, f"workspace too small: {need - 1} < {need} bytes")


def test_c_abi_argument_errors_return_before_any_device_call():
    from xvector_amd import hip
    lib, err = hip.lib, lambda: hip.lib.xvec_calib_last_error().decode()
    need = lib.xvec_calib_workspace_bytes(4)
    assert lib.xvec_calib_fit(None, 4, 1, 4, None, None, P, 4, 0.5, 10, P, P, need, None) == hip.ERR_ARG
    assert err() == "xvec_calib_fit: null pointer: scores"
    assert lib.xvec_calib_fit(P, 4, 1, 4, None, None, P, 4, 1.5, 10, P, P, need, None) == hip.ERR_ARG and "p_target = 1.5" in err()
    assert lib.xvec_calib_fit(P, 4, 1, 4, None, None, P, 4, 0.5, 0, P, P, need, None) == hip.ERR_ARG and "max_iter = 0" in err()
    assert lib.xvec_calib_fit(P, 4, 1, 4, None, None, P, 2 ** 31, 0.5, 10, P, P, need, None) == hip.ERR_TOO_LARGE
    assert lib.xvec_calib_fit(P, 4, 1, 4, None, None, P, 4, 0.5, 10, None, P, need, None) == hip.ERR_ARG and "out" in err()
    assert lib.xvec_calib_fit_all_pairs(P, 65536, 65536, 65536, P, P, 1, 0.5, 10, P, P, need, None) == hip.ERR_TOO_LARGE
    assert lib.xvec_calib_apply(P, 4, 2, 4, None, Q, 4, None) == hip.ERR_ARG and err() == "xvec_calib_apply: null pointer: scores / fit / out"
    assert lib.xvec_calib_apply(P, 4, 2, 4, P, P, 5, None) == hip.ERR_ARG and "in place" in err()
    assert lib.xvec_calib_cllr(P, 4, 1, 4, None, None, P, 4, 0.0, 1.0, 0.5, P, P, need, None) == hip.ERR_ARG and "c_miss = 0" in err()
    assert lib.xvec_calib_min_cllr(P, 4, 1, 4, None, None, P, 4, P, None, None, None, None, 3, P, need, None) == hip.ERR_ARG
    assert "seg_capacity = 3" in err()
    assert lib.xvec_calib_min_cllr(P, 4, 1, 4, None, None, P, 4, None, None, None, None, None, 0, P, need, None) == hip.ERR_ARG
