"""CPU-only checks of VBx (include/xvec_vbx.h): the two forms of the numpy restatement tests/vbx_ref.py against each other and
against their np.longdouble runs, what the GPU test relies on in its cases (no frame a near tie, no ELBO increment near
epsilon), the oracle's rules, VbxModel.from_plda, the host-only plan (csrc/vbx_plan.h) through its dump program, and the C
ABI's argument errors (each returns before the library touches a device).

The gaps.  The scaled form keeps every quantity of the recurrences at the scale of 1, so its fp64 run stays within a few
1e-14 of the extended-precision run; the log-domain form loses the digits in front of the point of log-likelihoods of
thousands of nats (6e-13 .. 2e-10 over the issue's three cases).  The bounds asserted here are ten times the worst of those
figures, and every case prints what it measures."""
import ctypes

import numpy as np
import pytest

import vbx_ref
from hipcc_support import header_constants, host_program, needs_host_cxx

P = 0x1000          # a pointer that is never followed: every call here fails its argument checks first
INF, NAN = float("inf"), float("nan")
SCALED_GAP, LOG_GAP = 5e-13, 2e-9


# ---------------------------------------------------------------- the restatement

@pytest.mark.parametrize("name", ["issue65", "issue257", "issue513"])
def test_the_two_forms_agree_with_each_other_and_with_longdouble(name):
    refs = vbx_ref.case_refs(name)
    ld = refs["ld"]
    X, phi, gamma0, pi0 = vbx_ref.case_data(name)
    scaled_ld = vbx_ref.vbx_scaled(X, phi, gamma0, pi0, max_iter=10, epsilon=-INF, dtype=np.longdouble, **vbx_ref.OPTS)
    d_forms = vbx_ref.distances(scaled_ld, ld)                   # the two forms, both in extended precision
    d_scaled, d_log = vbx_ref.distances(refs["scaled"], ld), vbx_ref.distances(refs["log"], ld)
    print(f"[vbx] {name}: forms in longdouble {d_forms[0]:.2e}; to longdouble (gamma, pi, elbo): scaled fp64 "
          f"{d_scaled[0]:.2e} {d_scaled[1]:.2e} {d_scaled[2]:.2e}, log-domain fp64 {d_log[0]:.2e} {d_log[1]:.2e} {d_log[2]:.2e}")
    assert ld[0].dtype == np.longdouble and refs["scaled"][0].dtype == np.float64
    # one algorithm: what is left between them is the log-domain form's loss at 2^-11 of its fp64 size (the 64-bit significand)
    assert max(d_forms[:2]) <= LOG_GAP * 2.0 ** -11 and d_forms[2] <= 1e-15
    assert max(d_scaled[:2]) <= SCALED_GAP and max(d_log[:2]) <= LOG_GAP and max(d_scaled[2], d_log[2]) <= 1e-13
    assert np.allclose(np.asarray(ld[0], dtype=np.float64).sum(axis=1), 1.0, rtol=0, atol=1e-12) and abs(float(ld[1].sum()) - 1) < 1e-12
    assert all(refs[f][3] == 10 and not np.isnan(refs[f][2]).any() for f in ("ld", "log", "scaled"))


@pytest.mark.parametrize("name", list(vbx_ref.CASES))
def test_no_frame_of_a_gpu_case_is_a_near_tie(name):
    g = np.sort(np.asarray(vbx_ref.case_refs(name)["ld"][0], dtype=np.float64), axis=1)
    margin = float((g[:, -1] - g[:, -2]).min()) if g.shape[1] > 1 else INF
    print(f"[vbx] {name}: smallest top-1 - top-2 margin {margin:.3g}")
    assert margin > 1e-3


@pytest.mark.parametrize("name", vbx_ref.STOP_CASES)
def test_no_elbo_increment_of_a_stop_case_is_near_epsilon(name):
    ld = vbx_ref.case_refs(name, epsilon=1e-4, max_iter=40)["ld"]
    n = ld[3]
    e = np.asarray(ld[2], dtype=np.float64)
    assert 2 <= n < 40 and not np.isnan(e[:n]).any() and np.isnan(e[n:]).all()
    inc = np.diff(e[:n])
    clear = np.abs(inc - 1e-4) / np.abs(e[1:n])
    print(f"[vbx] {name}: {n} iterations, increments {inc}, nearest to epsilon {clear.min():.2e} |ELBO|")
    assert (clear > 1e-6).all() and inc[-1] < 1e-4 and (inc[:-1] >= 1e-4).all()
    for form in ("log", "scaled"):                               # and both fp64 forms stop where it does
        assert vbx_ref.case_refs(name, epsilon=1e-4, max_iter=40)[form][3] == n


def test_oracle_rules_dead_speakers_single_frames_and_single_speakers():
    X, phi, gamma0, _ = vbx_ref.case_data("issue65")
    pi0 = np.array([0.4, 0.0, 0.3, 0.0, 0.2, 0.1])
    with np.errstate(invalid="ignore", divide="ignore"):
        a = vbx_ref.vbx_log(X, phi, gamma0, pi0, max_iter=5, epsilon=-INF, **vbx_ref.OPTS)
    b = vbx_ref.vbx_scaled(X, phi, gamma0, pi0, max_iter=5, epsilon=-INF, **vbx_ref.OPTS)
    for g, pi, elbo, iters in (a, b):
        assert (g[:, [1, 3]] == 0).all() and (pi[[1, 3]] == 0).all() and np.isfinite(elbo).all() and iters == 5
    assert np.abs(a[0] - b[0]).max() < LOG_GAP
    # a dead speaker with the best emission must not take the row maximum: the scaled form stays finite
    Xd = X.copy()
    g_dead = gamma0.copy()
    g_dead[:, 1] = 50.0                                          # speaker 1 owns every frame on entry, and is dead
    c = vbx_ref.vbx_scaled(Xd, phi, g_dead, pi0, max_iter=2, epsilon=-INF, **vbx_ref.OPTS)
    assert np.isfinite(c[0]).all() and (c[0][:, 1] == 0).all()
    # T = 1 and S = 1
    one = vbx_ref.vbx_scaled(X[:1], phi, gamma0[:1], np.full(6, 1 / 6), max_iter=3, epsilon=-INF, **vbx_ref.OPTS)
    assert one[0].shape == (1, 6) and abs(one[0].sum() - 1) < 1e-15 and np.array_equal(one[1], one[0][0] / one[0][0].sum())
    solo = vbx_ref.vbx_scaled(X, phi, np.ones((65, 1)), np.ones(1), max_iter=3, epsilon=-INF, **vbx_ref.OPTS)
    assert np.abs(solo[0] - 1).max() < 1e-14 and solo[1].tolist() == [1.0]
    assert vbx_ref.labels_of(solo[0])[1] == 1
    # the labelling: ties to the lowest speaker, numbered in the order of first appearance
    lab, n = vbx_ref.labels_of(np.array([[0.2, 0.4, 0.4], [0.5, 0.1, 0.4], [0.1, 0.8, 0.1], [0.0, 0.0, 1.0]]))
    assert lab.tolist() == [0, 1, 0, 2] and n == 3
    g, pi = vbx_ref.init_gamma(np.array([1, 0, 7, -1]), 3, 5.0)
    assert np.allclose(g.sum(axis=1), 1) and g[0].argmax() == 1 and (g[2:] == 1 / 3).all() and (pi == 1 / 3).all()


def test_from_plda_diagonalises_both_covariances():
    from xvector_amd.vbx import VbxModel
    rng = np.random.default_rng(11)
    dim, rank = 24, 9
    R = rng.standard_normal((dim, dim))
    Sigma = R @ R.T + 0.5 * np.eye(dim)
    F = rng.standard_normal((dim, rank))
    F[:, 6:] = F[:, :3] * 2.0                                    # rank-deficient: six directions
    mean = rng.standard_normal(dim)
    vm = VbxModel.from_plda(mean, F, Sigma)
    assert vm.A.shape == (6, dim) and vm.phi.shape == (6,) and (vm.phi > 0).all() and (np.diff(vm.phi) <= 0).all()
    within, between = vm.A @ Sigma @ vm.A.T, vm.A @ F @ F.T @ vm.A.T
    assert np.abs(within - np.eye(6)).max() <= 1e-10
    assert np.abs(between - np.diag(vm.phi)).max() <= 1e-10 * vm.phi.max()

    class Model:
        pass
    m = Model()
    m.mean, m.F, m.Sigma = mean, F, Sigma
    again = VbxModel.from_plda(m)
    assert np.array_equal(again.A, vm.A) and np.array_equal(again.phi, vm.phi) and np.array_equal(again.mean, mean)
    with pytest.raises(ValueError, match="expected"):
        VbxModel.from_plda(mean, F[:5], Sigma)


# ---------------------------------------------------------------- the host-only plan

@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return host_program("vbx_plan_dump", tmp_path_factory.mktemp("vbx_plan"))


def _a256(n):
    return -(-n // 256) * 256


@needs_host_cxx
def test_plan_layout_is_the_restated_one_and_what_the_library_reports(plan):
    from xvector_amd import hip
    for dim, S, counts in ((16, 5, [1]), (128, 10, [37] * 64), (12, 5, [5, 64, 1, 65, 300, 37, 1]), (512, 64, [16384]), (1, 1, [2, 3])):
        v = [int(x) for x in plan([f"layout {dim} {S} " + " ".join(map(str, counts))])[0].split()[1:]]
        n_rec, N, dp = len(counts), sum(counts), dim + 1
        want, at = [], 0
        for nbytes in (8 * (n_rec + 1), 8 * N * dp, 8 * N, 8 * N * S, 8 * N * S, 8 * N, 8 * N, 4 * N, 8 * n_rec * S * dp):
            want.append(at)
            at += _a256(nbytes)
        assert v == want + [at], (dim, S, counts)
        rs = (ctypes.c_int64 * (n_rec + 1))(*np.concatenate([[0], np.cumsum(counts)]).tolist())
        assert hip.lib.xvec_vbx_workspace_bytes(rs, n_rec, dim, S) == at


@needs_host_cxx
def test_plan_refusals_and_launches(plan):
    from xvector_amd import vbx
    cap, threads = vbx.MAX_FRAMES, vbx.THREADS
    got = plan(["check 3 1 4", f"check {cap}", f"check 3 {cap + 1}", "check 3 0 4", "start 1 4", "start 0",
                "shape 512 64", "shape 513 4", "shape 0 4", "shape 8 65", "shape 8 0",
                "options 0.99 0.3 17 1e-4 40", "options 0 0.3 17 -inf 1", "options 1 0.3 17 1e-4 40", "options -0.1 0.3 17 1e-4 40",
                "options nan 0.3 17 1e-4 40", "options 0.5 0 17 1e-4 40", "options 0.5 0.3 -1 1e-4 40", "options 0.5 inf 17 1e-4 40",
                "options 0.5 0.3 17 1e-4 0", "options 0.5 0.3 17 nan 3",
                "launch 2368 64", f"launch {cap} 1", "launch 3 1000", f"launch {threads + 1} 2"])
    assert got[:2] == ["ok", "ok"]
    assert got[2] == f"refused recording 1 has {cap + 1} frames, more than XVEC_VBX_MAX_FRAMES = {cap}"
    assert got[3] == "refused recording 1 is empty or rec_start decreases: every recording needs a frame"
    assert got[4] == "refused rec_start must begin at 0 (got 1)" and got[5] == "refused n_rec = 0: need at least one recording"
    assert got[6] == "ok" and got[7] == "refused dim = 513 must lie in 1 .. XVEC_VBX_MAX_DIM = 512"
    assert got[8] == "refused dim = 0 must lie in 1 .. XVEC_VBX_MAX_DIM = 512"
    assert got[9] == "refused n_spk = 65 must lie in 1 .. XVEC_VBX_MAX_SPEAKERS = 64"
    assert got[10] == "refused n_spk = 0 must lie in 1 .. XVEC_VBX_MAX_SPEAKERS = 64"
    assert got[11:13] == ["ok", "ok"]
    assert got[13] == "refused loop_prob = 1 must lie in [0, 1)" and got[14] == "refused loop_prob = -0.1 must lie in [0, 1)"
    assert got[15] in ("refused loop_prob = nan must lie in [0, 1)", "refused loop_prob = -nan must lie in [0, 1)")
    assert got[16] == "refused Fa = 0 must be positive and finite" and got[17] == "refused Fb = -1 must be positive and finite"
    assert got[18] == "refused Fa = inf must be positive and finite"
    assert got[19] == "refused max_iter = 0: need at least one iteration" and got[20] == "refused epsilon is NaN (-inf never stops early)"
    # one block per recording whatever else; the init kernel a thread per row of gamma or pi
    assert got[21] == f"launch 64 {threads} {-(-2368 // threads)} {threads}" and got[22] == f"launch 1 {threads} {cap // threads} {threads}"
    assert got[23] == f"launch 1000 {threads} {-(-1000 // threads)} {threads}" and got[24] == f"launch 2 {threads} 2 {threads}"


# ---------------------------------------------------------------- the header, the module and the C ABI without a device

def test_module_restates_the_header_constants_and_refuses_the_cpu():
    import torch
    import xvector_amd
    from xvector_amd import diarize, vbx
    consts = header_constants("xvec_vbx.h", "XVEC_VBX_")
    assert consts == {"MAX_SPEAKERS": vbx.MAX_SPEAKERS, "MAX_DIM": vbx.MAX_DIM, "MAX_FRAMES": vbx.MAX_FRAMES, "THREADS": vbx.THREADS,
                      "PREFETCH": vbx.PREFETCH}
    assert (consts["MAX_SPEAKERS"], consts["MAX_DIM"], consts["MAX_FRAMES"]) == (64, 512, 16384)
    assert (vbx_ref.THREADS, vbx_ref.PREFETCH, vbx_ref.MAX_FRAMES) == (vbx.THREADS, vbx.PREFETCH, vbx.MAX_FRAMES)
    exports = {"xvec_vbx_last_error", "xvec_vbx_workspace_bytes", "xvec_vbx_init", "xvec_vbx_run"}
    assert exports <= set(xvector_amd.hip.EXPORTS) and all(hasattr(xvector_amd.hip.lib, n) for n in exports)
    with pytest.raises(RuntimeError, match="HIP device only"):
        vbx.vbx(torch.zeros(4, 3, dtype=torch.float64), [0, 4], np.ones(3), init_labels=[0, 0, 1, 1], n_speakers=2)
    with pytest.raises(RuntimeError, match="HIP device only"):
        vbx.vbx_init(torch.zeros(4, dtype=torch.int32), [0, 4], 2)
    model = vbx.VbxModel(np.zeros(3), np.eye(3), np.ones(3))
    with pytest.raises(RuntimeError, match="HIP device only"):
        diarize.Diarizer(None, "cosine", threshold=0.0, device="cpu", resegment=vbx.Vbx(model))
    assert xvector_amd.Vbx is vbx.Vbx and xvector_amd.VbxModel is vbx.VbxModel and xvector_amd.VbxResult is vbx.VbxResult
    assert xvector_amd.vbx is vbx and {"vbx", "Vbx", "VbxModel", "VbxResult"} <= set(xvector_amd.__all__)
    with pytest.raises(ValueError, match="positive phi"):
        vbx.VbxModel(np.zeros(3), np.eye(3), np.array([1.0, 0.0, 2.0]))


def _start(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _good(hip):
    return dict(X=P, ldx=16, dim=16, phi=P, start=_start(0, 4, 9), n_rec=2, n_spk=5, opts=hip.VbxOptions(0.99, 0.3, 17.0, 1e-4, 40, 0),
                gamma=P, ldg=5, pi=P, elbo=P, iters=P, labels=P, count=P, ws=P, ws_bytes=None)


def _call(hip, **kw):
    a = {**_good(hip), **kw}
    if a["ws_bytes"] is None:
        a["ws_bytes"] = hip.lib.xvec_vbx_workspace_bytes(_start(0, 4, 9), 2, 16, 5)
    opts = a["opts"]
    return hip.lib.xvec_vbx_run(a["X"], a["ldx"], a["dim"], a["phi"], a["start"], a["n_rec"], a["n_spk"],
                                None if opts is None else ctypes.byref(opts), a["gamma"], a["ldg"], a["pi"], a["elbo"], a["iters"],
                                a["labels"], a["count"], a["ws"], a["ws_bytes"], None)


def test_c_abi_argument_errors_return_before_any_device_call():
    from xvector_amd import hip
    lib, err = hip.lib, lambda: hip.lib.xvec_vbx_last_error().decode()
    O = hip.VbxOptions
    cap = 16384
    null = "null pointer: X / phi / gamma / pi / elbo / iters"
    cases = [
        (dict(n_rec=0), "n_rec = 0: need at least one recording"),
        (dict(start=None), "null pointer: rec_start"),
        (dict(start=_start(2, 4, 9)), "rec_start must begin at 0 (got 2)"),
        (dict(start=_start(0, 0, 9)), "recording 0 is empty or rec_start decreases: every recording needs a frame"),
        (dict(start=_start(0, 4, cap + 5)), f"recording 1 has {cap + 1} frames, more than XVEC_VBX_MAX_FRAMES = {cap}"),
        (dict(n_spk=65, ldg=65), "n_spk = 65 must lie in 1 .. XVEC_VBX_MAX_SPEAKERS = 64"),
        (dict(n_spk=0), "n_spk = 0 must lie in 1 .. XVEC_VBX_MAX_SPEAKERS = 64"),
        (dict(dim=513, ldx=513), "dim = 513 must lie in 1 .. XVEC_VBX_MAX_DIM = 512"),
        (dict(opts=None), "null pointer: options"),
        (dict(opts=O(1.0, 0.3, 17.0, 1e-4, 40, 0)), "loop_prob = 1 must lie in [0, 1)"),
        (dict(opts=O(0.99, 0.0, 17.0, 1e-4, 40, 0)), "Fa = 0 must be positive and finite"),
        (dict(opts=O(0.99, -2.0, 17.0, 1e-4, 40, 0)), "Fa = -2 must be positive and finite"),
        (dict(opts=O(0.99, 0.3, 0.0, 1e-4, 40, 0)), "Fb = 0 must be positive and finite"),
        (dict(opts=O(0.99, 0.3, 17.0, 1e-4, 0, 0)), "max_iter = 0: need at least one iteration"),
        (dict(opts=O(0.99, 0.3, 17.0, NAN, 40, 0)), "epsilon is NaN (-inf never stops early)"),
        (dict(ldx=15), "ldx = 15 is smaller than dim = 16"),
        (dict(ldg=4), "ldg = 4 is smaller than the 5 speakers"),
        *[(dict(**{k: None}), null) for k in ("X", "phi", "gamma", "pi", "elbo", "iters")],
    ]
    for kwargs, text in cases:
        assert _call(hip, **kwargs) == hip.ERR_ARG, kwargs
        assert err() == text, kwargs
    # the size query answers 0 for what the entry point refuses
    good = _start(0, 4, 9)
    for args in ((good, 0, 16, 5), (None, 2, 16, 5), (_start(1, 4, 9), 2, 16, 5), (_start(0, 4, cap + 5), 2, 16, 5), (good, 2, 513, 5),
                 (good, 2, 16, 65), (good, 2, 0, 5), (good, 2, 16, 0)):
        assert lib.xvec_vbx_workspace_bytes(*args) == 0
    assert lib.xvec_vbx_workspace_bytes(_start(0, cap), 1, 512, 64) >= 8 * cap * (513 + 2 * 64)
    # xvec_vbx_init
    init = lambda **kw: lib.xvec_vbx_init(*[{**dict(labels=P, start=good, n_rec=2, n_spk=5, sm=5.0, gamma=P, ldg=5, pi=P), **kw}[k]
                                           for k in ("labels", "start", "n_rec", "n_spk", "sm", "gamma", "ldg", "pi")], None)
    for kwargs, text in ((dict(n_rec=-1), "n_rec = -1: need at least one recording"), (dict(n_spk=65), "n_spk = 65 must lie in 1 .. XVEC_VBX_MAX_SPEAKERS = 64"),
                         (dict(sm=INF), "smoothing = inf must be finite"), (dict(ldg=4), "ldg = 4 is smaller than the 5 speakers"),
                         (dict(labels=None), "null pointer: labels / gamma / pi"), (dict(pi=None), "null pointer: labels / gamma / pi")):
        assert init(**kwargs) == hip.ERR_ARG and err() == text, kwargs


def test_workspace_refusals_through_the_vbx_pairs():
    """Every (void*, _wsb_vbx) pair of the binding is this unit's and is held here: a null and a one-byte-short workspace."""
    from xvector_amd import hip
    C = ctypes
    takes = {n for n, (_, a) in hip._SIGS.items() if any(x is hip._wsb_vbx and a[i - 1] is C.c_void_p for i, x in enumerate(a))}
    assert takes == {"xvec_vbx_run"} and issubclass(hip._wsb_vbx, hip._wsb_report) and hip._wsb_vbx is not hip._wsb_report
    need = hip.lib.xvec_vbx_workspace_bytes(_start(0, 4, 9), 2, 16, 5)
    assert need % 256 == 0 and need >= 8 * 9 * (17 + 5 + 5 + 3) + 8 * 2 * 5 * 17
    assert _call(hip, ws=None) == hip.ERR_ARG and hip.lib.xvec_vbx_last_error().decode() == "null pointer: workspace"
    assert _call(hip, ws_bytes=need - 1) == hip.ERR_WORKSPACE
    assert hip.lib.xvec_vbx_last_error().decode() == f"workspace too small: {need - 1} < {need} bytes"
    assert _call(hip, ws_bytes=0) == hip.ERR_WORKSPACE


def test_vbx_error_channel_is_its_own():
    from xvector_amd import hip
    lib = hip.lib
    assert lib.xvec_ahc_cluster(P, 9, _start(0, 4, 9), 2, 0.0, -2, None, P, P, None, None, None, P, 1 << 20, None) == hip.ERR_ARG
    assert _call(hip, ldg=3) == hip.ERR_ARG
    assert lib.xvec_vbx_last_error().decode() == "ldg = 3 is smaller than the 5 speakers"
    assert lib.xvec_diar_last_error().decode() == "max_clusters = -2 must not be negative (0 = no limit)"
