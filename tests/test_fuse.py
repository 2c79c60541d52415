"""CPU-only checks of score fusion (include/xvec_fuse.h, xvector_amd.fuse): the numpy restatement tests/fuse_ref.py against
scipy's BFGS and against a case worked by hand; the properties the GPU tests rely on, shown on the restatement for every input
they use; the host-only plan (csrc/fuse_plan.h) through its dump program -- the constants, the words of a pass, the workspace
regions aligned and disjoint for every K, every refusal's text; the exports, and what the entry points answer to a null and to a
short workspace and to bad arguments (each returns before the library touches a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fuse_ref as fr
from calib_ref import LD, LN2
from conftest import ROOT
from hipcc_support import header_constants, host_program, needs_host_cxx

P, Q = 0x1000, 0x2000      # pointers that are never followed


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return host_program("fuse_plan_dump", tmp_path_factory.mktemp("fuse_plan"))


# ---------------------------------------------------------------- the restatement

def _standardised_problem(F, tgt, p_target, l2):
    """(objective with gradient over (w', b'), Z) in float64, written independently of fuse_ref._derivatives."""
    from scipy.special import expit
    z = (F - F.mean(axis=1, keepdims=True)) / F.std(axis=1, keepdims=True)
    w = np.where(tgt, p_target / tgt.sum(), (1 - p_target) / (~tgt).sum())
    tau = np.log(p_target / (1 - p_target))
    sign = np.where(tgt, -1.0, 1.0)

    def f(x):
        u = sign * (x[:-1] @ z + x[-1] + tau)
        dj = sign * w * expit(u)
        return ((w * np.logaddexp(0.0, u)).sum() + l2 / 2 * (x[:-1] ** 2).sum(), np.r_[z @ dj + l2 * x[:-1], dj.sum()])
    return f


@pytest.mark.parametrize("k,p_target,l2", [(4, 0.5, 0.0), (4, 0.01, 0.0), (8, 0.5, 0.0), (2, 0.5, 1e-3)])
def test_restatement_against_scipy_bfgs(k, p_target, l2):
    from scipy.optimize import minimize
    pl = fr.planted()
    r, c, t = fr.upper_triangle(pl["n"], pl["labels"])
    F, tgt, n_nan, n_bad = fr.select_trials(fr.planted_terms(pl, k), pl["n"], pl["n"], r, c, t)
    assert F.shape == (k, 2556) and (n_nan, n_bad) == (0, 0)
    ref = fr.fit(F, tgt, p_target, l2)
    assert ref["converged"] and ref["grad"] < 1e-18 and not ref["constant"].any()
    res = minimize(_standardised_problem(F, tgt, p_target, l2), np.zeros(k + 1), jac=True, method="BFGS", options={"gtol": 1e-10})
    diff = np.abs(res.x - ref["x_std"].astype(np.float64)).max()
    print(f"K = {k}, p_target {p_target}, l2 {l2}: BFGS after {res.nit} iterations, max |difference| {diff:.3e}")
    assert diff <= 1e-5
    # the raw coordinates are the standardised ones carried over, and the objective the restatement reports is J at its point
    assert abs(float(ref["J_data"] - fr.objective(F, tgt, ref["w"], ref["b"], p_target))) <= 1e-17
    assert abs(float(ref["penalty"] - LD(l2) / 2 * (ref["x_std"][:-1] ** 2).sum())) <= 1e-18      # (J - J_data: numbers of size 1 at 2^-64)
    assert abs(res.fun - float(ref["J"])) <= 1e-10


def test_restatement_against_a_case_worked_by_hand():
    """K = 1, four trials: f = (-2, -1, 1, 2), the second and the fourth targets, p_target = 0.5.  mu = 0, sd^2 = 10 / 4; at
    (0, 0) every logistic is 1 / 2 and every weight 1 / 4, so J = ln 2, g_w = (1 / 8) (z_1 + z_3 - z_2 - z_4) = -1 / (4 sd),
    g_b = 0, H_ww = (1 / 16) sum z^2 = 1 / 4, H_wb = (1 / 16) sum z = 0, H_bb = 1 / 4: the Newton step is (1 / sd, 0), which is
    w = 1 / sd^2 = 0.4 and b = 0 in raw coordinates."""
    F = np.array([[-2.0, -1.0, 1.0, 2.0]])
    tgt = np.array([False, True, False, True])
    mu, sd, const = fr.standardise(F)
    assert float(mu[0]) == 0.0 and abs(float(sd[0] ** 2) - 2.5) < 1e-18 and not const[0]
    Z = np.vstack([F.astype(LD) / sd[0], np.ones((1, 4), dtype=LD)])
    w = np.full(4, LD(1) / 4)
    J, Jd, g, H, at = fr._derivatives(Z, tgt, w, LD(0), LD(0), np.zeros(2, dtype=LD))
    tiny = 1e-18
    assert abs(float(J - LN2)) < tiny and J == Jd
    assert abs(float(g[0] + 1 / (4 * sd[0]))) < tiny and abs(float(g[1])) < tiny
    assert np.abs((H - np.array([[0.25, 0.0], [0.0, 0.25]])).astype(np.float64)).max() < tiny
    assert abs(at["j"] - float(LN2)) < 1e-15 and abs(at["g"][0] - float((np.abs(F[0]) / sd[0]).sum() / 8)) < 1e-15
    step = fr._solve(H, -g[:, None])[:, 0]
    assert abs(float(step[0] - 1 / sd[0])) < tiny and abs(float(step[1])) < tiny
    x, _, passes, _ = fr._newton(Z, tgt, w, LD(0), LD(0), np.zeros(2, dtype=LD), None, 0.0, 2)      # one step: two passes
    assert passes == 2 and abs(float(x[0] / sd[0]) - 0.4) < 1e-17 and abs(float(x[1])) < tiny
    # and the fit goes on from there to the minimum of this set (it has one: the classes overlap)
    ref = fr.fit(F, tgt, 0.5)
    assert ref["converged"] and 0.4 < float(ref["w"][0]) < 1.0 and abs(float(ref["b"])) < 1e-15


def test_the_exact_constant_rule_and_the_separability_test():
    F = np.vstack([np.full(7, 0.1), np.arange(7.0), np.r_[np.full(6, 0.1), 0.1 + 2.0 ** -56]])
    mu, sd, const = fr.standardise(F)
    assert const.tolist() == [True, False, False] and float(mu[0]) == 0.1 and float(sd[0]) == 1.0
    assert float(np.full(7, 0.1).sum() / 7) != 0.1                             # why the rule is not "the variance is 0"
    assert 0 < float(sd[2]) < 1e-16                                            # a tiny spread is a scale, not a constant
    Fs, ts = fr.separable_set()
    assert not fr.fit(Fs, ts, 0.5)["converged"] and fr.fit(Fs, ts, 0.5, 1e-3)["converged"]
    weak = np.array([[0.0, 0.0, 1.0, 1.0, 2.0]])                               # targets >= 1 >= non-targets: weakly separable
    assert not fr.fit(weak, np.array([False, False, False, True, True]), 0.5)["converged"]
    ones = np.ones((1, 5))
    assert fr.weakly_separable(np.vstack([weak, ones]), np.array([False, False, False, True, True]))
    assert not fr.weakly_separable(np.vstack([weak, ones]), np.array([False, True, False, True, False]))
    # identical terms are not a direction of separation: the minimum exists, it is only not unique
    Fi, ti = fr.identical_case()
    ref = fr.fit(Fi, ti, 0.5)
    assert ref["converged"] and not np.isfinite(ref["H_inv"]).all()
    one = fr.fit(Fi[:1], ti, 0.5)
    assert abs(float(ref["w"].sum() - one["w"][0])) < 1e-12 and abs(float(ref["J"] - one["J"])) < 1e-17


@pytest.mark.parametrize("case", list(fr.gpu_fit_cases()), ids=lambda c: c[0])
def test_reference_properties_the_gpu_tests_rely_on(case):
    """For the inputs of every fit the GPU tests hold to bounds: the restatement converges in well under the max_iter they pass,
    its inverse Hessian is finite, and the bounds that follow are tight enough to mean something."""
    name, F, tgt, p, l2, has_minimum = case
    ref = fr.fit(F, tgt, p, l2)
    assert ref["converged"] == has_minimum, name
    if not has_minimum:
        return
    assert ref["passes"] <= fr.GPU_MAX_ITER // 4 and ref["grad"] < 1e-17, (name, ref["passes"], ref["grad"])
    assert np.isfinite(ref["H_inv"].astype(np.float64)).all(), name
    bw, bb, bj, bp = fr.fit_bounds(ref, fr.sum_constant(F.shape[1], len(F)))
    print(f"{name}: {ref['passes']} passes, ||H^-1|| {float(np.abs(ref['H_inv']).sum(axis=1).max()):.3e}, bounds w {bw.max():.3e} b {bb:.3e} "
          f"objective {bj:.3e} penalty {bp:.3e}")
    assert bw.max() < 1e-8 and bb < 1e-8 and bj < 1e-8
    assert (bw[ref["constant"]] == 0).all() and (ref["w"][ref["constant"]] == 0).all()


def test_term_ulps_is_the_headers_derivation():
    text = open(os.path.join(ROOT, "include", "xvec_fuse.h")).read()
    macro = re.search(r"#define XVEC_FUSE_TERM_ULPS\(K\) \((.*)\)\n", text).group(1)
    calib = header_constants("xvec_calib.h", "XVEC_CALIB_")["TERM_ULPS"]
    for k in range(1, 9):
        assert eval(macro.replace("/", "//").replace("(K)", f"({k})")) == fr.term_ulps(k) == 6 + -(-(calib - 6) * (4 * k + 1) // 5)
    assert fr.term_ulps(1) == calib and fr.term_ulps(8) == 389
    assert "4 K + 1 roundings" in text and "58 / 5" in text                    # the derivation is in the header's text


# ---------------------------------------------------------------- the host-only plan

@needs_host_cxx
def test_plan_constants_are_the_headers_and_the_modules(plan):
    from xvector_amd import calibrate, fuse
    consts = header_constants("xvec_fuse.h", "XVEC_FUSE_")
    v = [int(x) for x in plan(["const"])[0].split()[1:]]
    assert v[0] == consts["MAX_TERMS"] == fuse.MAX_TERMS == fr.MAX_TERMS == 8
    assert v[1:4] == [calibrate.THREADS, calibrate.ITEMS, calibrate.MAX_BLOCKS] == [fr.B, fr.ITEMS, fr.MAX_BLOCKS]
    assert v[4] == 1024 and v[5] == 5
    assert v[6:9] == [consts["MATRIX"], consts["ROW"], consts["COL"]] == [fuse.MATRIX, fuse.ROW, fuse.COL] == [fr.MATRIX, fr.ROW, fr.COL]
    assert v[9:] == [consts["CONVERGED"], consts["MAX_ITER"], consts["ONE_CLASS"], consts["INF_SCORE"]] == [0, 1, 2, 3]
    assert v[9:] == [fuse.CONVERGED, fuse.MAX_ITER_REACHED, fuse.ONE_CLASS, fuse.INF_SCORE]
    assert v[9:] == [calibrate.CONVERGED, calibrate.MAX_ITER_REACHED, calibrate.ONE_CLASS, calibrate.INF_SCORE]      # numbered as calibration's
    text = open(os.path.join(ROOT, "include", "xvec_fuse.h")).read()
    assert float(re.search(r"#define XVEC_FUSE_STEP_TOL (\S+)", text).group(1)) == fuse.STEP_TOL == fr.STEP_TOL == calibrate_step_tol()
    assert [fuse.term_ulps(k) for k in range(1, 9)] == [fr.term_ulps(k) for k in range(1, 9)]


def calibrate_step_tol():
    text = open(os.path.join(ROOT, "include", "xvec_calib.h")).read()
    return float(re.search(r"#define XVEC_CALIB_STEP_TOL (\S+)", text).group(1))


@needs_host_cxx
def test_words_of_a_pass_and_where_the_hessian_lies(plan):
    for k, line, hess in zip(range(1, 9), plan([f"words {k}" for k in range(1, 9)]), plan([f"hess {k}" for k in range(1, 9)])):
        words, gather, stride, ulps = (int(x) for x in line.split()[1:])
        assert words == (k + 1) * (k + 4) // 2 + 1 == 1 + (k + 1) + (k + 1) * (k + 2) // 2, k
        assert gather == 5 + 3 * k and stride == max(words, gather) and ulps == fr.term_ulps(k), k
        at = [int(x) for x in hess.split()[1:]]
        assert at == list(range(k + 2, words)), k                               # J, the gradient, then the triangle row by row
    assert plan(["words 1", "words 8"]) == ["words 6 8 8 64", "words 55 29 55 389"]
    ns = [1, 2047, 2048, 2049, 2 ** 21, 2 ** 21 + 5, 2 ** 31 - 1]
    for n, line in zip(ns, plan([f"blocks {n}" for n in ns])):
        blocks, depth = (int(x) for x in line.split()[1:])
        assert blocks == min(-(-n // 2048), 1024) and depth == -(-n // (blocks * 256)) + 22, (n, line)
        assert fr.sum_constant(n, 3) == depth + fr.term_ulps(3)


@needs_host_cxx
def test_workspace_regions_are_aligned_and_disjoint_for_every_k(plan):
    from xvector_amd import hip
    ns = [1, 2, 255, 256, 257, 2047, 2048, 2049, 37720, 4874 * 4874, 2 ** 31 - 1]
    asked = [(n, k) for n in ns for k in range(1, 9)]
    for (n, k), line in zip(asked, plan([f"layout {n} {k}" for n, k in asked])):
        offs = [int(x) for x in line.split()[1:]]
        total = offs.pop()
        sizes = [1024, 1024 * max((k + 1) * (k + 4) // 2 + 1, 5 + 3 * k) * 8, 8 * n * k, n]
        assert offs[0] == 0 and all(o % 256 == 0 for o in offs), (n, k, line)
        for q in range(3):
            assert offs[q] + sizes[q] <= offs[q + 1] < offs[q] + sizes[q] + 256, (n, k, q, line)
        assert offs[3] + sizes[3] <= total < offs[3] + sizes[3] + 256, (n, k, line)
        assert hip.lib.xvec_fuse_workspace_bytes(n, k) == total, (n, k)
    assert 1.49e9 < hip.lib.xvec_fuse_workspace_bytes(4874 * 4874, 8) < 1.56e9      # the header's 1.5 GB
    for n, k in ((0, 1), (-1, 1), (2 ** 31, 1), (10, 0), (10, 9), (10, -1)):
        assert hip.lib.xvec_fuse_workspace_bytes(n, k) == 0, (n, k)
    assert plan(["layout 0 1", "layout 10 0", "layout 10 9"]) == ["layout 0 0 0 0 0"] * 3


# request -> what the plan answers: ok, or the refusal's text (one per refusal)
REFUSALS = {
    "terms 3 4 0 4 1": "ok",
    "terms 8 4 2 0 1": "ok",
    "terms 0 4 0 4 1": "refused n_terms = 0 must lie in 1 .. 8",
    "terms 9 4 0 4 1": "refused n_terms = 9 must lie in 1 .. 8",
    "terms 3 4 3 4 1": "refused term 2: unknown kind 3",
    "terms 2 4 -1 4 1": "refused term 1: unknown kind -1",
    "terms 3 4 1 0 0": "refused term 2: null pointer: data",
    "terms 1 4 0 3 1": "refused term 0: ld = 3 is smaller than n_cols = 4",
    "terms 2 4 1 3 1": "ok",                                                   # ld means nothing to a ROW term
    "ridge 0": "ok",
    "ridge 0.001": "ok",
    "ridge -1e-9": "refused l2 = -1e-09 must be finite and not negative",
    "ridge nan": "refused l2 = nan must be finite and not negative",
    "ridge inf": "refused l2 = inf must be finite and not negative",
    "fit 0.5 50": "ok",
    "fit 1 50": "refused p_target = 1 must lie strictly between 0 and 1",
    "fit 0.5 0": "refused max_iter = 0 must lie in 1 .. 1000",
    "fit 0.5 1001": "refused max_iter = 1001 must lie in 1 .. 1000",
    "trials 2 1 4 0 4": "ok",
    "trials 2 3 4 1 9": "ok",
    "trials 2 1 4 0 0": "refused n_trials = 0: need at least one trial",
    f"trials 2 1 4 0 {2 ** 31}": f"toolarge n_trials = {2 ** 31} exceeds 2^31 - 1",
    "trials 2 0 4 1 4": "refused score matrix [0, 4]: both sizes must be in 1 .. 2^31 - 1",
    "trials 9 1 4 0 4": "refused n_terms = 9 must lie in 1 .. 8",
    "trials 2 2 4 0 3": "refused without index arrays the scores are a vector: n_rows = 1 and n_cols >= n_trials (got [2, 4] for 3 trials)",
    "trials 2 1 3 0 4": "refused without index arrays the scores are a vector: n_rows = 1 and n_cols >= n_trials (got [1, 3] for 4 trials)",
    "pairs 2 3 4": "ok",
    "pairs 2 3 0": "refused score matrix [3, 0]: both sizes must be in 1 .. 2^31 - 1",
    "pairs 0 3 4": "refused n_terms = 0 must lie in 1 .. 8",
    "pairs 1 65536 65536": "toolarge 65536 x 65536 cells exceed 2^31 - 1 trials",
    "apply 2 3 4 4 -1 0 4": "ok",
    "apply 2 3 4 5 -1 0 4": "ok",
    "apply 2 3 4 3 -1 0 4": "refused ld_out = 3 must be at least n_cols = 4",
    "apply 2 3 4 6 0 0 6": "ok",                                               # in place over a MATRIX term
    "apply 2 3 4 4 0 0 6": "refused in place (out is the data of term 0) needs ld_out == ld (got 4 and 6)",
    "apply 2 3 4 4 0 1 0": "refused out is the data of term 0, which is not a MATRIX term",
    "apply 2 3 4 4 0 2 0": "refused out is the data of term 0, which is not a MATRIX term",
    "apply 2 3 4 4 1 0 4": "ok",
    "apply 2 3 4 4 -1 0 3": "refused term 0: ld = 3 is smaller than n_cols = 4",
    "apply 9 3 4 4 -1 0 4": "refused n_terms = 9 must lie in 1 .. 8",
}


@needs_host_cxx
def test_argument_checks_of_the_plan_one_text_each(plan):
    asked = list(REFUSALS)
    for a, got in zip(asked, plan(asked)):
        assert got == REFUSALS[a], (a, got)
    texts = {re.sub(r"-?\d+(\.\d+)?(e-?\d+)?|nan|inf", "#", v) for v in REFUSALS.values() if v != "ok"}
    assert len(texts) >= 14


# ---------------------------------------------------------------- the header, the module and the C ABI without a device

EXPORTS = {"xvec_fuse_last_error", "xvec_fuse_workspace_bytes", "xvec_fuse_fit", "xvec_fuse_fit_all_pairs", "xvec_fuse_apply"}


def _header_signatures():
    """{function: (return type, [parameter type, ...])} of include/xvec_fuse.h."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xvec_fuse.h")).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\n([a-z_0-9 ]+?\**)\s*(xvec_fuse_\w+)\s*\(([^)]*)\)\s*;", src):
        types = []
        for prm in (p.strip() for p in params.split(",")):
            if prm != "void":
                types.append(re.sub(r"\s*\w+$", "", prm).replace("const ", "").strip())
        out[name] = (ret.replace("const ", "").strip(), types)
    return out


def test_exports_and_python_signatures_match_the_header():
    import torch
    import xvector_amd
    from xvector_amd import fuse, hip
    sigs = _header_signatures()
    assert set(sigs) == EXPORTS <= set(hip.EXPORTS) and all(hasattr(hip.lib, n) for n in EXPORTS)
    ctype = {"int64_t": {C.c_int64}, "int32_t": {C.c_int32}, "double": {C.c_double}, "size_t": {C.c_size_t, hip._wsb_fuse},
             "xvec_stream": {C.c_void_p}}
    for name, (ret, types) in sigs.items():
        res, args = hip._SIGS[name]
        assert res is {"char*": C.c_char_p, "size_t": C.c_size_t, "int": C.c_int}[ret], name
        assert len(args) == len(types), name
        for a, t in zip(args, types):
            assert a in (ctype[t] if t in ctype else {C.c_void_p}) and (t in ctype or t.endswith("*")), (name, t, a)
    # one more class of workspace size: a subclass the older units' tests do not see
    assert C.sizeof(hip._wsb_fuse) == C.sizeof(C.c_size_t) and issubclass(hip._wsb_fuse, hip._wsb_der) and hip._wsb_fuse is not hip._wsb_der
    # the records the module reads are the header's
    assert C.sizeof(fuse._Fit) == 128 and C.sizeof(fuse._Term) == 24
    assert [f[0] for f in fuse._Fit._fields_[:2]] == ["w", "b"] and fuse._Fit.b.offset == 64
    for name in ("Fusion", "FusionResult", "ScoreFuser", "Term", "fit_fusion", "fit_fusion_all_pairs", "log_duration_terms",
                 "row_quality", "col_quality"):
        assert getattr(xvector_amd, name) is getattr(fuse, name) and name in xvector_amd.__all__
    assert xvector_amd.fuse is fuse and "fuse" in xvector_amd.__all__
    cpu = torch.zeros(3, 3, dtype=torch.float64)
    for call in (lambda: fuse.matrix(cpu), lambda: fuse.row_quality(cpu[0]), lambda: fuse.col_quality(cpu[0]),
                 lambda: fuse.log_duration_terms(cpu[0] + 300, cpu[0] + 300),
                 lambda: fuse.fit_fusion([fuse.Term(fuse.MATRIX, cpu)], xvector_amd.TrialList([0, 1], [1, 2], [1, 0])),
                 lambda: fuse.fit_fusion_all_pairs([fuse.Term(fuse.MATRIX, cpu)], [0, 0, 1])):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()
    # the module's own argument checks, one text each
    for kwargs, text in (({"p_target": 1.0}, "p_target = 1.0 must lie strictly between 0 and 1"), ({"l2": -1.0}, "l2 = -1.0 must be finite"),
                         ({"l2": float("nan")}, "l2 = nan must be finite"), ({"l2": float("inf")}, "l2 = inf must be finite"),
                         ({"max_iter": 0}, "max_iter = 0 must lie in 1 .. 1000")):
        with pytest.raises(ValueError, match=re.escape(text)):
            fuse.ScoreFuser(**kwargs)
    with pytest.raises(ValueError, match="0 terms: the count must lie in 1 .. 8"):
        fuse.fit_fusion([], [1, 0])
    with pytest.raises(ValueError, match="9 terms: the count must lie in 1 .. 8"):
        fuse.fit_fusion([fuse.Term(fuse.MATRIX, cpu)] * 9, [1, 0])
    with pytest.raises(TypeError, match="term 0 is not a Term"):
        fuse.fit_fusion([cpu], [1, 0])
    with pytest.raises(ValueError, match="term 0: unknown kind 7"):
        fuse.fit_fusion([fuse.Term(7, cpu)], [1, 0])
    with pytest.raises(RuntimeError, match="call fit"):
        fuse.ScoreFuser().fuse([fuse.Term(fuse.MATRIX, cpu)])


WS, WSB = object(), object()


def _terms(n, *spec):
    """A host array of xvec_fuse_term: (data, ld, kind) each."""
    from xvector_amd import fuse
    arr = (fuse._Term * max(1, n))()
    for k, (data, ld, kind) in enumerate(spec):
        arr[k].data, arr[k].ld, arr[k].kind = data, ld, kind
    return arr


def _calls():
    one = _terms(1, (P, 1, 0))
    # entry point: the smallest valid arguments (one term, one trial), the workspace and its size marked
    return {
        "xvec_fuse_fit": (one, 1, 1, 1, None, None, P, 1, 0.5, 0.0, 10, P, WS, WSB, None),
        "xvec_fuse_fit_all_pairs": (one, 1, 1, 1, P, P, 0, 0.5, 0.0, 10, P, WS, WSB, None),
    }


@pytest.mark.parametrize("name", ["xvec_fuse_fit", "xvec_fuse_fit_all_pairs"])
def test_null_and_short_workspaces_are_refused(name):
    """The style of tests/test_workspace_refusals.py: XVEC_ERR_ARG "null pointer: workspace" for a null workspace,
    XVEC_ERR_WORKSPACE "workspace too small: <have> < <need> bytes" for one a byte short; nothing is launched."""
    from xvector_amd import hip
    calls = _calls()
    takes = {n for n, (_, a) in hip._SIGS.items() if any(x is hip._wsb_fuse and a[i - 1] is C.c_void_p for i, x in enumerate(a))}
    assert takes == set(calls)
    need = hip.lib.xvec_fuse_workspace_bytes(1, 1)
    assert need >= 1024 and need % 256 == 0

    def answer(ws, size):
        rc = getattr(hip.lib, name)(*[ws if a is WS else size if a is WSB else a for a in calls[name]])
        return rc, hip.lib.xvec_fuse_last_error().decode()
    assert answer(None, need) == (hip.ERR_ARG, "null pointer: workspace")
    assert answer(P, need - 1) == (hip.ERR_WORKSPACE, f"workspace too small: {need - 1} < {need} bytes")


def test_c_abi_argument_errors_return_before_any_device_call():
    from xvector_amd import hip
    lib, err = hip.lib, lambda: hip.lib.xvec_fuse_last_error().decode()
    need = lib.xvec_fuse_workspace_bytes(4, 2)
    two = _terms(2, (P, 4, 0), (Q, 0, 2))
    fit = lambda terms=two, k=2, cols=4, tgt=P, n=4, p=0.5, l2=0.0, it=10, out=P: lib.xvec_fuse_fit(
        terms, k, 1, cols, None, None, tgt, n, p, l2, it, out, P, need, None)
    assert fit(terms=None) == hip.ERR_ARG and err() == "xvec_fuse_fit: null pointer: terms"
    assert fit(k=0) == hip.ERR_ARG and err() == "xvec_fuse_fit: n_terms = 0 must lie in 1 .. 8"
    assert fit(k=9) == hip.ERR_ARG and err() == "xvec_fuse_fit: n_terms = 9 must lie in 1 .. 8"
    assert fit(terms=_terms(2, (P, 4, 0), (Q, 0, 5))) == hip.ERR_ARG and err() == "xvec_fuse_fit: term 1: unknown kind 5"
    assert fit(terms=_terms(2, (P, 4, 0), (None, 0, 1))) == hip.ERR_ARG and err() == "xvec_fuse_fit: term 1: null pointer: data"
    assert fit(terms=_terms(2, (P, 3, 0), (Q, 0, 2))) == hip.ERR_ARG and err() == "xvec_fuse_fit: term 0: ld = 3 is smaller than n_cols = 4"
    assert fit(l2=-1.0) == hip.ERR_ARG and err() == "xvec_fuse_fit: l2 = -1 must be finite and not negative"
    assert fit(l2=float("nan")) == hip.ERR_ARG and "l2 = nan" in err()
    assert fit(l2=float("inf")) == hip.ERR_ARG and "l2 = inf" in err()
    assert fit(p=1.5) == hip.ERR_ARG and "p_target = 1.5" in err()
    assert fit(it=0) == hip.ERR_ARG and "max_iter = 0" in err()
    assert fit(tgt=None) == hip.ERR_ARG and err() == "xvec_fuse_fit: null pointer: is_target"
    assert fit(n=2 ** 31) == hip.ERR_TOO_LARGE
    assert fit(n=5) == hip.ERR_ARG and "without index arrays" in err()
    assert fit(out=None) == hip.ERR_ARG and err() == "xvec_fuse_fit: null pointer: out"
    assert lib.xvec_fuse_fit(two, 2, 3, 4, P, None, P, 4, 0.5, 0.0, 10, P, P, need, None) == hip.ERR_ARG and "both be given" in err()
    assert lib.xvec_fuse_fit_all_pairs(two, 2, 65536, 65536, P, P, 1, 0.5, 0.0, 10, P, P, need, None) == hip.ERR_ARG      # ld = 4 < 65536
    big = _terms(1, (P, 65536, 0))
    assert lib.xvec_fuse_fit_all_pairs(big, 1, 65536, 65536, P, P, 1, 0.5, 0.0, 10, P, P, need, None) == hip.ERR_TOO_LARGE
    assert lib.xvec_fuse_fit_all_pairs(two, 2, 1, 4, None, P, 1, 0.5, 0.0, 10, P, P, need, None) == hip.ERR_ARG
    assert err() == "xvec_fuse_fit_all_pairs: null pointer: row_class / col_class"
    assert lib.xvec_fuse_apply(two, 2, 1, 4, None, Q, 4, None) == hip.ERR_ARG and err() == "xvec_fuse_apply: null pointer: fit / out"
    assert lib.xvec_fuse_apply(two, 2, 1, 4, P, P, 5, None) == hip.ERR_ARG and "in place (out is the data of term 0)" in err()
    assert lib.xvec_fuse_apply(two, 2, 1, 4, P, Q, 4, None) == hip.ERR_ARG and "term 1, which is not a MATRIX term" in err()
    assert lib.xvec_fuse_apply(two, 2, 1, 4, P, 0x3000, 3, None) == hip.ERR_ARG and "ld_out = 3" in err()
