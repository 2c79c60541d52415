"""CPU-only checks of the GMM-UBM unit (include/xvec_gmm.h, xvector_amd.gmm): the numpy oracle tests/gmm_ref.py against the
scikit-learn fixture tests/golden/g13_gmm.npz and, where it is installed, against scikit-learn itself; EM's lower bound; MAP
and linear scoring against hand-computed two-component cases and against the first-order expansion of the exact LLR; the
host-only plan (csrc/gmm_plan.h) through its dump program against a Python restatement, with every refusal's text; the
exports against the header and what the entry points answer to bad arguments and to a null or short workspace (each returns
before the library touches a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gmm_ref as gr
from conftest import ROOT
from hipcc_support import header_constants, host_program, needs_host_cxx

P = 0x1000      # a pointer that is never followed
LD = np.longdouble
MARGIN = 8      # as tests/test_gmm_gpu.py: the bar is 8 x the distance of the fp64 oracle to the longdouble one


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return host_program("gmm_plan_dump", tmp_path_factory.mktemp("gmm_plan"))


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "g13_gmm.npz")) as z:
        return {k: z[k] for k in z.files}


def within(got, r64, rld):
    bar = MARGIN * float(np.abs(np.asarray(r64).astype(LD) - rld).max())
    assert float(np.abs(np.asarray(got).astype(LD) - rld).max()) <= bar, bar


# ---------------------------------------------------------------- the oracle

def test_oracle_reproduces_the_scikit_learn_fixture(golden):
    z = golden
    x, w0, mu0, v0 = z["x"], z["w0"], z["mu0"], z["v0"]
    assert x.shape == (333, 7) and mu0.shape == (5, 7)
    r64, rld = gr.loglik(x, w0, mu0, v0), gr.loglik(x, w0, mu0, v0, dtype=LD)
    within(z["score_samples"], r64["lse"], rld["lse"])
    within(z["predict_proba"], r64["gamma"], rld["gamma"])
    for k in (1, 10):
        e64, eld = gr.em(x, w0, mu0, v0, k), gr.em(x, w0, mu0, v0, k, dtype=LD)
        for name, a, b in zip(("w", "mu", "v"), e64, eld):
            within(z[f"{name}{k}"], a, b)
        within([z[f"lb{k}"]], e64[3][-1:], eld[3][-1:])


def test_oracle_equals_live_scikit_learn():
    mix = pytest.importorskip("sklearn.mixture")
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.normal(m, 1.0, (80, 4)) for m in (-3.0, 0.0, 4.0)])
    w0, mu0, v0 = np.array([0.2, 0.5, 0.3]), x[[3, 100, 200]], np.full((3, 4), 2.0)
    gm = mix.GaussianMixture(3, covariance_type="diag", tol=0.0, max_iter=4, weights_init=w0, means_init=mu0, precisions_init=1 / v0)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm.fit(x)
    w, mu, v, lb, n = gr.em(x, w0, mu0, v0, 4)
    np.testing.assert_allclose(w, gm.weights_, rtol=0, atol=1e-13)
    np.testing.assert_allclose(mu, gm.means_, rtol=0, atol=1e-12)
    np.testing.assert_allclose(v, gm.covariances_, rtol=0, atol=1e-12)
    np.testing.assert_allclose(lb[-1], gm.lower_bound_, rtol=0, atol=1e-12)
    np.testing.assert_allclose(gr.loglik(x, w, mu, v)["lse"], gm.score_samples(x), rtol=0, atol=1e-12)


def test_lower_bound_does_not_decrease_and_bad_frames_leave(golden):
    z = golden
    lb = gr.em(z["x"], z["w0"], z["mu0"], z["v0"], 25)[3]
    assert (np.diff(lb) >= -1e-12).all() and lb[-1] > lb[0] + 1.0
    x = z["x"].copy()
    x[4, 2], x[9, 0] = np.nan, np.inf
    a = gr.accumulate(x, z["w0"], z["mu0"], z["v0"])
    b = gr.accumulate(np.delete(z["x"], [4, 9], axis=0), z["w0"], z["mu0"], z["v0"])
    assert (a["n_bad"], a["n_frames"]) == (2, 331)
    for k in ("n", "f", "s"):
        np.testing.assert_allclose(a[k], b[k], rtol=1e-13, atol=1e-13)
    # utterances: overlap doubles a row, an empty range gives zeros, the global form is their sum
    first, count = [0, 10, 5, 300], [20, 0, 30, 33]
    per = gr.accumulate(z["x"], z["w0"], z["mu0"], z["v0"], first, count, per_utt=True)
    glob = gr.accumulate(z["x"], z["w0"], z["mu0"], z["v0"], first, count)
    assert not per["n"][1].any() and per["n_frames"].tolist() == count and glob["n_frames"] == 83
    np.testing.assert_allclose(per["n"].sum(axis=0), glob["n"], rtol=1e-13)
    np.testing.assert_allclose(per["f"].sum(axis=0), glob["f"], rtol=1e-12, atol=1e-12)
    w = z["w0"].copy()
    w[2] = 0.0
    r = gr.loglik(z["x"], w / w.sum(), z["mu0"], z["v0"])
    assert not r["gamma"][:, 2].any() and np.isfinite(r["gamma"]).all() and np.allclose(r["gamma"].sum(axis=1), 1.0)


def test_map_and_linear_scores_by_hand():
    mu = np.array([[0.0, 2.0], [4.0, -2.0]])
    v = np.array([[1.0, 4.0], [2.0, 0.5]])
    n = np.array([[16.0, 0.0], [48.0, 16.0]])
    f = np.array([[[16.0, 48.0], [0.0, 0.0]], [[96.0, 0.0], [32.0, -64.0]]])
    hat = gr.map_means(n, f, mu, relevance=16.0)
    # row 0: alpha = (1/2, -): component 0 halfway to f / n = (1, 3); component 1 without frames keeps mu exactly
    assert hat[0].tolist() == [[0.5, 2.5], [4.0, -2.0]]
    # row 1: alpha = (3/4, 1/2): (3/4)(2, 0) + (1/4)(0, 2) = (1.5, 0.5); (1/2)(2, -4) + (1/2)(4, -2) = (3, -3)
    assert hat[1].tolist() == [[1.5, 0.5], [3.0, -3.0]]
    # scores of the two models against test statistics n = (2, 2), f = ((2, 6), (6, -2)): centred f - n mu = ((2, 2), (-2, 2)),
    # over 4 frames ((.5, .5), (-.5, .5)); model 0: offsets ((.5, .5), (0, 0)) / v = ((.5, .125), (0, 0)) -> .25 + .0625
    tn, tf = np.array([[2.0, 2.0], [0.0, 0.0]]), np.array([[[2.0, 6.0], [6.0, -2.0]], [[0.0, 0.0], [0.0, 0.0]]])
    S = gr.linear_scores(hat, tn, tf, mu, v)
    assert S[0, 0] == 0.3125
    # model 1: offsets ((1.5, -1.5), (-1, -1)) / v = ((1.5, -.375), (-.5, -2)) -> .75 - .1875 + .25 - 1 = -.1875
    assert S[1, 0] == -0.1875 and S[:, 1].tolist() == [0.0, 0.0]          # a test row without frames scores 0


def test_linear_scores_are_the_first_order_expansion_of_the_exact_llr(golden):
    z = golden
    x, w, mu, v = z["x"], z["w10"], z["mu10"], z["v10"]
    rng = np.random.default_rng(7)
    delta = rng.normal(0.0, 1.0, (3,) + mu.shape)
    first, count = [0, 100, 250], [100, 150, 83]
    st = gr.accumulate(x, w, mu, v, first, count, per_utt=True)
    errs = []
    for t in (1e-2, 1e-3, 1e-4):
        lin = gr.linear_scores(mu[None] + t * delta, st["n"], st["f"], mu, v, dtype=LD)
        exact = gr.llr(x, w, mu, v, mu[None] + t * delta, first, count, dtype=LD)
        errs.append(float(np.abs(exact - lin).max()) / t)
        assert np.abs(lin).max() > 1e-2 * t
    # the remainder is of second order: (exact - linear) / t falls with t
    assert errs[0] > 5 * errs[1] > 25 * errs[2] and errs[2] < 1e-2


# ---------------------------------------------------------------- the plan

@needs_host_cxx
def test_plan_constants_and_tiles(plan):
    k = header_constants("xvec_gmm.h", "XVEC_GMM_")
    const = [int(x) for x in plan(["const"])[0].split()[1:]]
    assert const == [256, k["FRAME_TILE"], k["COMP_TILE"], 64, 16, 80, k["MAX_C"], k["MAX_D"], k["MAX_UTTS"], k["MAX_SLICES"],
                     k["MAX_ITER"], 1024, 1024, 64]
    assert (k["FRAME_TILE"], k["COMP_TILE"], k["MAX_C"], k["MAX_D"], k["MAX_SLICES"], k["X_F32"], k["X_F64"]) == (64, 64, 4096, 256, 1024, 0, 1)
    cases = [(1, 1, 1, 1, 0, 0), (65, 1, 3, 1, 0, 0), (257, 1, 63, 13, 0, 2), (300, 1, 65, 24, 0, 7), (1000, 1, 130, 36, 0, 0),
             (1000000, 1, 2048, 24, 0, 0), (1000000, 1, 512, 72, 0, 0), (1000000, 4874, 2048, 24, 1, 0), (0, 3, 4096, 256, 0, 0),
             (2 ** 30, 1, 64, 31, 0, 0), (2 ** 30, 1, 64, 32, 0, 1024), (5000, 2, 64, 63, 1, 0), (5000, 2, 64, 64, 1, 0)]
    for n, U, C_, D, per, sl in cases:
        got = [int(x) for x in plan([f"plan {n} {U} {C_} {D} {per} {sl}"])[0].split()[1:]]
        want = gr.plan(n, C_, D, U, bool(per), sl)
        assert got == [want[key] for key in ("comp_tiles", "col_tiles", "slices", "slice_frames", "k_pad", "k_chunks", "slab_doubles")], (n, C_, D)
    assert gr.plan(1000000, 2048, 24)["slices"] == 32 and gr.plan(1000000, 512, 72)["slices"] == 42
    assert gr.plan(1000, 130, 36)["slices"] == 1 and gr.plan(3000, 64, 24)["slices"] == 3


@needs_host_cxx
def test_plan_workspace_regions(plan):
    up = lambda v: (v + 255) // 256 * 256
    for U, C_, D in ((1, 1, 1), (300, 65, 24), (4874, 2048, 24)):
        frames = up(8 * U) + up(8 * (U + 1))
        model = up(16 * C_ * D) + up(8 * C_)
        assert plan([f"loglik {U} {C_} {D}"])[0].split()[1:] == [str(v) for v in (0, up(8 * U), frames, frames + up(16 * C_ * D), frames + model)]
        for n, per, sl in ((1000, 0, 0), (1000, 0, 7), (1000, 1, 0), (0, 0, 0)):
            p = gr.plan(n, C_, D, U, bool(per), sl)
            lse = up(8 * max(n, 1))
            slab = 0 if per else up(8 * p["slab_doubles"])
            got = [int(v) for v in plan([f"acc {n} {U} {C_} {D} {per} {sl}"])[0].split()[1:]]
            assert got == [0, up(8 * U), frames, frames + up(16 * C_ * D), frames + model, 0 if per else frames + model + lse,
                           frames + model + lse + slab, p["slices"]]
            if not per:
                base = got[6]
                em = [int(v) for v in plan([f"em {n} {U} {C_} {D} {sl}"])[0].split()[1:]]
                assert em == [base, base + up(8 * C_), base + up(8 * C_) + up(8 * C_ * D), base + up(8 * C_) + 2 * up(8 * C_ * D),
                              base + up(8 * C_) + 2 * up(8 * C_ * D) + 256, base + up(8 * C_) + 2 * up(8 * C_ * D) + 512]
    assert plan(["score 3 5 65 24"])[0] == f"score 0 {up(8 * 3 * 65 * 24)} {up(8 * 3 * 65 * 24) + up(8 * 5 * 65 * 24)}"
    for bad in ("loglik 0 1 1", "loglik 1 0 1", "loglik 1 4097 1", "loglik 1 1 257", f"loglik {2 ** 24 + 1} 1 1"):
        assert plan([bad])[0].split()[-1] == "0", bad
    for bad in ("acc -1 1 1 1 0 0", f"acc {2 ** 30 + 1} 1 1 1 0 0", "acc 5 1 1 1 0 1025", "acc 5 1 1 1 1 2", "acc 5 1 1 1 0 -1"):
        assert plan([bad])[0].split()[-2] == "0", bad
    assert plan(["em 5 1 1 1 1025"])[0].split()[-1] == "0" and plan(["score 0 1 1 1"])[0].split()[-1] == "0"


@needs_host_cxx
def test_plan_refusals(plan):
    ask = lambda line: plan([line])[0]
    assert ask("model 1 1") == ask("model 4096 256") == "ok"
    assert ask("model 0 1") == "refused C = 0 must lie in 1 .. 4096" and ask("model 4097 1") == "refused C = 4097 must lie in 1 .. 4096"
    assert ask("model 1 0") == "refused D = 0 must lie in 1 .. 256" and ask("model 1 257") == "refused D = 257 must lie in 1 .. 256"
    ok = "frames 1 1 0 0 100 24 24 1"
    assert ask(ok + " 0 100") == "ok 100" and ask(ok + " 0 10 5 10 99 1 100 0 50 0") == "ok 21"      # overlap, the last row, empty ranges
    assert ask("frames 0 1 0 0 100 24 24 1 0 1") == "refused null pointer: frames"
    assert ask("frames 1 0 0 0 100 24 24 1 0 1") == "refused null pointer: x"
    assert ask("frames 1 1 2 0 100 24 24 1 0 1") == "refused x_type = 2 must be 0 (fp32) or 1 (fp64)"
    assert ask("frames 1 1 0 3 100 24 24 1 0 1") == "refused reserved = 3 must be 0"
    assert ask("frames 1 1 0 0 0 24 24 1 0 0") == "refused rows = 0: need at least one row"
    assert ask("frames 1 1 0 0 100 23 24 1 0 1") == "refused ldx = 23 is smaller than D = 24"
    assert ask("frames 1 1 0 0 100 24 24 1") == f"refused n_utts = 0 must lie in 1 .. {2 ** 24}"
    assert ask("frames 1 1 0 0 100 24 24 0 0 1") == "refused null pointer: utt_first / utt_count"
    assert ask(ok + " 0 5 7 -1") == "refused utt_count[1] = -1 is negative"
    assert ask(ok + " 0 101") == "refused utterance 0 = rows [0, 0 + 101) leaves the 100 rows"
    assert ask(ok + " 0 5 -1 2") == "refused utterance 1 = rows [-1, -1 + 2) leaves the 100 rows"
    assert ask(ok + " 99 2") == "refused utterance 0 = rows [99, 99 + 2) leaves the 100 rows"
    assert ask(ok + " 101 0") == "refused utterance 0 = rows [101, 101 + 0) leaves the 100 rows"
    assert ask(ok + f" 0 {2 ** 62} 0 {2 ** 62}").startswith("refused utterance 0")
    big = f"frames 1 1 0 0 {2 ** 30} 24 24 1" + f" 0 {2 ** 30}" * 2
    assert ask(big) == "refused the utterances hold more than 2^30 frames"
    assert ask("slices 0 0") == ask("slices 0 1024") == ask("slices 1 0") == "ok"
    assert ask("slices 0 -1") == "refused n_slices = -1 must lie in 0 .. 1024" and ask("slices 0 1025") == "refused n_slices = 1025 must lie in 0 .. 1024"
    assert ask("slices 1 2") == "refused n_slices = 2 must be 0 in the per-utterance form"
    assert ask("options 1 1e-6 0 0") == "ok" and ask("options 0 0 0 0") == "refused null pointer: options"
    assert ask("options 1 -1 0 0") == "refused reg_covar = -1 must be finite and not negative"
    assert ask("options 1 0 nan 0") == "refused var_floor = nan must be finite and not negative"
    assert ask("options 1 0 0 inf") == "refused min_count = inf must be finite and not negative"
    assert ask("iter 1 0") == ask("iter 10000 inf") == "ok"
    assert ask("iter 0 0") == "refused max_iter = 0 must lie in 1 .. 10000" and ask("iter 10001 0") == "refused max_iter = 10001 must lie in 1 .. 10000"
    assert ask("iter 5 -1") == "refused tol = -1 must not be negative" and ask("iter 5 nan") == "refused tol = nan must not be negative"
    assert ask("map 1 16") == "ok" and ask("map 0 16") == "refused M = 0 must lie in 1 .. 2^31 - 1"
    assert ask("map 1 0") == "refused relevance = 0 must be positive and finite" and ask("map 1 inf") == "refused relevance = inf must be positive and finite"
    assert ask("scores 2 3 3") == "ok" and ask("scores 0 3 3") == "refused M = 0 must lie in 1 .. 2^31 - 1"
    assert ask("scores 2 0 3") == "refused U = 0 must lie in 1 .. 2^31 - 1" and ask("scores 2 3 2") == "refused ld_s = 2 is smaller than U = 3"
    assert ask("query 5 1 1 1 0 0 1") == "ok" and ask("query 5 1 1 1 0 0 0") == "refused null pointer: out"
    assert ask("query -1 1 1 1 0 0 1") == "refused n_total = -1 must lie in 0 .. 2^30"
    assert ask("query 5 0 1 1 0 0 1") == f"refused n_utts = 0 must lie in 1 .. {2 ** 24}"
    assert ask("query 5 1 0 1 0 0 1") == "refused C = 0 must lie in 1 .. 4096" and ask("query 5 1 1 1 1 3 1") == "refused n_slices = 3 must be 0 in the per-utterance form"


# ---------------------------------------------------------------- the module and the C ABI without a device

EXPORTS = {"xvec_gmm_last_error", "xvec_gmm_plan_host", "xvec_gmm_loglik_workspace_bytes", "xvec_gmm_accumulate_workspace_bytes",
           "xvec_gmm_em_workspace_bytes", "xvec_gmm_linear_scores_workspace_bytes", "xvec_gmm_prepare", "xvec_gmm_loglik",
           "xvec_gmm_accumulate", "xvec_gmm_mstep", "xvec_gmm_em", "xvec_gmm_map_means", "xvec_gmm_linear_scores"}


def test_exports_and_module_surface():
    import torch
    import xvector_amd
    from xvector_amd import gmm, hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xvec_gmm.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(xvec_gmm_[a-z_0-9]+)\s*\(", src)) == EXPORTS <= set(hip.EXPORTS)
    assert all(hasattr(hip.lib, n) for n in EXPORTS)
    assert C.sizeof(hip._wsb_gmm) == C.sizeof(C.c_size_t) and issubclass(hip._wsb_gmm, hip._wsb_analyze) and hip._wsb_gmm is not hip._wsb_analyze
    assert C.sizeof(hip.GmmFrames) == 56 and hip.GmmFrames.rows.offset == 16 and C.sizeof(hip.GmmMstepOptions) == 24
    k = header_constants("xvec_gmm.h", "XVEC_GMM_")
    assert (gmm.MAX_C, gmm.MAX_D, hip.GMM_X_F32, hip.GMM_X_F64) == (k["MAX_C"], k["MAX_D"], k["X_F32"], k["X_F64"])
    for name in ("DiagGmm", "GmmStats", "fit_ubm", "map_adapt", "linear_scores", "llr_scores", "frames_of"):
        assert getattr(xvector_amd, name) is getattr(gmm, name) and name in xvector_amd.__all__
    assert xvector_amd.gmm is gmm and "gmm" in xvector_amd.__all__
    cpu = torch.zeros(6, 3, dtype=torch.float64)
    for call in (lambda: gmm.DiagGmm([1.0], [[0.0] * 3], [[1.0] * 3], device="cpu"), lambda: gmm.fit_ubm(cpu, 2)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()
    feats, (first, count) = gmm.frames_of(torch.zeros(3, 5, 2), [5, 0, 2])
    assert feats.shape == (15, 2) and first.tolist() == [0, 5, 10] and count.tolist() == [5, 0, 2]
    with pytest.raises(ValueError, match="lengths in 0 .. 5"):
        gmm.frames_of(torch.zeros(3, 5, 2), [5, 6, 2])
    # the statistics in SIDEKIT's layout: stat0 [U, C], stat1 [U, C D] component-major
    st = gmm.GmmStats(torch.arange(6.0).reshape(2, 3), torch.arange(24.0).reshape(2, 3, 4)).stat_object(["a", "b"], ["u0", "u1"])
    assert st.stat0.shape == (2, 3) and st.stat1.shape == (2, 12) and st.stat1[1, 4:8].tolist() == [16.0, 17.0, 18.0, 19.0]
    assert list(st.modelset) == ["a", "b"]


def test_plan_host_equals_the_restatement():
    from xvector_amd import gmm, hip
    for n, C_, D, U, per, sl in ((1, 1, 1, 1, False, 0), (300, 65, 24, 1, False, 7), (1000000, 2048, 24, 1, False, 0),
                                 (1000000, 512, 72, 1, False, 0), (1000000, 2048, 24, 4874, True, 0), (0, 5, 7, 2, True, 0)):
        assert gmm.plan(n, C_, D, U, per, sl) == gr.plan(n, C_, D, U, per, sl)
    err = lambda: hip.lib.xvec_gmm_last_error().decode()
    out = (C.c_int64 * 10)()
    assert hip.lib.xvec_gmm_plan_host(5, 1, 0, 1, 0, 0, out) == hip.ERR_ARG and err() == "C = 0 must lie in 1 .. 4096"
    assert hip.lib.xvec_gmm_plan_host(5, 1, 1, 1, 0, 0, None) == hip.ERR_ARG and err() == "null pointer: out"


def test_c_abi_argument_errors_return_before_any_device_call():
    from xvector_amd import hip
    lib, err = hip.lib, lambda: hip.lib.xvec_gmm_last_error().decode()
    first, count = (C.c_int64 * 2)(0, 4), (C.c_int64 * 2)(4, 6)
    frames = lambda **kw: hip.GmmFrames(**{**dict(x=P, x_type=1, reserved=0, rows=10, ldx=3, utt_first=first, utt_count=count, n_utts=2), **kw})
    opts = lambda **kw: hip.GmmMstepOptions(**{**dict(reg_covar=1e-6, var_floor=0.0, min_count=0.0), **kw})
    ref = lambda s: None if s is None else C.byref(s)
    need_l, need_a = lib.xvec_gmm_loglik_workspace_bytes(2, 5, 3), lib.xvec_gmm_accumulate_workspace_bytes(10, 2, 5, 3, 0, 0)
    need_u, need_e = lib.xvec_gmm_accumulate_workspace_bytes(10, 2, 5, 3, 1, 0), lib.xvec_gmm_em_workspace_bytes(10, 2, 5, 3, 0)
    need_s = lib.xvec_gmm_linear_scores_workspace_bytes(2, 3, 5, 3)
    assert need_l == 1024 and need_u == need_l + 256 and need_a == need_u + 32768 and need_e == need_a + 3 * 256 + 512 and need_s == 256 + 512
    assert all(v % 256 == 0 for v in (need_l, need_a, need_u, need_e, need_s))
    assert lib.xvec_gmm_loglik_workspace_bytes(0, 5, 3) == 0 == lib.xvec_gmm_accumulate_workspace_bytes(10, 2, 5, 3, 1, 1)
    assert lib.xvec_gmm_em_workspace_bytes(10, 2, 4097, 3, 0) == 0 == lib.xvec_gmm_linear_scores_workspace_bytes(0, 3, 5, 3)

    def loglik(fr, C_=5, D=3, w=P, lse=P, ws=P, size=need_l):
        return lib.xvec_gmm_loglik(ref(fr), w, P, P, None, C_, D, lse, P, P, P, None, ws, size, None)

    def acc(fr, C_=5, D=3, per=0, sl=0, n=P, s=P, llsum=P, ws=P, size=None):
        return lib.xvec_gmm_accumulate(ref(fr), P, P, P, C_, D, per, sl, n, P, s, llsum, P, P, ws, need_u if size is None and per else
                                       need_a if size is None else size, None)

    def em(fr, o, C_=5, D=3, it=3, tol=0.0, sl=0, lb=P, ws=P, size=need_e):
        return lib.xvec_gmm_em(ref(fr), C_, D, it, tol, ref(o), sl, P, P, P, lb, P, P, ws, size, None)
    for call in (loglik, acc, lambda fr, **kw: em(fr, opts(), **kw)):
        assert call(None) == hip.ERR_ARG and err() == "null pointer: frames"
        assert call(frames(), C_=0) == hip.ERR_ARG and err() == "C = 0 must lie in 1 .. 4096"
        assert call(frames(), D=257) == hip.ERR_ARG and err() == "D = 257 must lie in 1 .. 256"
        assert call(frames(x=None)) == hip.ERR_ARG and err() == "null pointer: x"
        assert call(frames(x_type=2)) == hip.ERR_ARG and err() == "x_type = 2 must be 0 (fp32) or 1 (fp64)"
        assert call(frames(ldx=2)) == hip.ERR_ARG and err() == "ldx = 2 is smaller than D = 3"
        assert call(frames(rows=9)) == hip.ERR_ARG and err() == "utterance 1 = rows [4, 4 + 6) leaves the 9 rows"
        assert call(frames(n_utts=0)) == hip.ERR_ARG and err() == f"n_utts = 0 must lie in 1 .. {2 ** 24}"
        assert call(frames(utt_count=None)) == hip.ERR_ARG and err() == "null pointer: utt_first / utt_count"
        assert call(frames(), ws=None) == hip.ERR_ARG and err() == "null pointer: workspace"
    assert loglik(frames(), w=None) == hip.ERR_ARG and err() == "null pointer: w / mu / v"
    assert loglik(frames(), lse=None) == hip.ERR_ARG and err() == "null pointer: lse / utt_llsum / utt_frames / n_bad"
    assert acc(frames(), sl=1025) == hip.ERR_ARG and err() == "n_slices = 1025 must lie in 0 .. 1024"
    assert acc(frames(), per=1, sl=1) == hip.ERR_ARG and err() == "n_slices = 1 must be 0 in the per-utterance form"
    assert acc(frames(), s=None) == hip.ERR_ARG and err() == "null pointer: n / f / s"
    assert acc(frames(), per=1, s=None, ws=None) == hip.ERR_ARG and err() == "null pointer: workspace"      # (s is not looked at)
    assert acc(frames(), llsum=None) == hip.ERR_ARG and err() == "null pointer: llsum / n_frames / n_bad"
    assert em(frames(), None) == hip.ERR_ARG and err() == "null pointer: options"
    assert em(frames(), opts(reg_covar=-1.0)) == hip.ERR_ARG and err() == "reg_covar = -1 must be finite and not negative"
    assert em(frames(), opts(), it=0) == hip.ERR_ARG and err() == "max_iter = 0 must lie in 1 .. 10000"
    assert em(frames(), opts(), tol=-1.0) == hip.ERR_ARG and err() == "tol = -1 must not be negative"
    assert em(frames(), opts(), lb=None) == hip.ERR_ARG and err() == "null pointer: lower_bound / n_iter_done / n_bad"
    none = (C.c_int64 * 2)(0, 0)
    assert em(frames(utt_count=none), opts()) == hip.ERR_ARG and err() == "the utterances hold no frame"
    for call, need in ((loglik, need_l), (acc, need_a), (lambda fr, **kw: acc(fr, per=1, **kw), need_u), (lambda fr, **kw: em(fr, opts(), **kw), need_e)):
        assert call(frames(), size=need - 1) == hip.ERR_WORKSPACE and err() == f"workspace too small: {need - 1} < {need} bytes"
    assert lib.xvec_gmm_prepare(P, P, P, None, 5, 3, None, P, None) == hip.ERR_ARG and err() == "null pointer: w / mu / v / P / g"
    assert lib.xvec_gmm_prepare(P, P, P, None, 5, 0, P, P, None) == hip.ERR_ARG and err() == "D = 0 must lie in 1 .. 256"
    assert lib.xvec_gmm_mstep(P, P, P, P, 5, 3, None, P, P, P, None) == hip.ERR_ARG and err() == "null pointer: options"
    assert lib.xvec_gmm_mstep(P, P, P, None, 5, 3, ref(opts()), P, P, P, None) == hip.ERR_ARG and err() == "null pointer: n / f / s / n_frames / w / mu / v"
    assert lib.xvec_gmm_map_means(P, P, P, 2, 5, 3, 0.0, P, None) == hip.ERR_ARG and err() == "relevance = 0 must be positive and finite"
    assert lib.xvec_gmm_map_means(P, P, P, 0, 5, 3, 16.0, P, None) == hip.ERR_ARG and err() == "M = 0 must lie in 1 .. 2^31 - 1"
    assert lib.xvec_gmm_map_means(P, P, P, 2, 5, 3, 16.0, None, None) == hip.ERR_ARG and err() == "null pointer: n / f / mu / mu_hat"
    score = lambda M=2, U=3, ld=3, S=P, ws=P, size=need_s: lib.xvec_gmm_linear_scores(P, M, P, P, U, P, P, 5, 3, S, ld, ws, size, None)
    assert score(M=0) == hip.ERR_ARG and err() == "M = 0 must lie in 1 .. 2^31 - 1"
    assert score(ld=2) == hip.ERR_ARG and err() == "ld_s = 2 is smaller than U = 3"
    assert score(S=None) == hip.ERR_ARG and err() == "null pointer: mu_hat / n / f / mu / v / S"
    assert score(ws=None) == hip.ERR_ARG and err() == "null pointer: workspace"
    assert score(size=need_s - 1) == hip.ERR_WORKSPACE and err() == f"workspace too small: {need_s - 1} < {need_s} bytes"
    # every (void*, _wsb_gmm) pair of the binding is held here
    takes = {n for n, (_, a) in hip._SIGS.items() if any(x is hip._wsb_gmm and a[i - 1] is C.c_void_p for i, x in enumerate(a))}
    assert takes == {"xvec_gmm_loglik", "xvec_gmm_accumulate", "xvec_gmm_em", "xvec_gmm_linear_scores"}
