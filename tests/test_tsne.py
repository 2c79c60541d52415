"""CPU-only checks of exact t-SNE and the PCA map (include/xvec_tsne.h, xvector_amd.visualize): the numpy restatement
tests/tsne_ref.py against the fixture written from scikit-learn (tests/golden/g11_tsne.npz) and against scikit-learn's private
functions where it is installed; the host-only plan (csrc/tsne_plan.h) through its dump program -- the row groups and column
slices cover every (row, column) once, the workspace regions do not overlap; the C ABI's argument errors (each returns before
the library touches a device) and its error channel; and the module's schedule on a fake stepper."""
import os
import threading

import numpy as np
import pytest

import tsne_ref
from conftest import ROOT, load_golden
from hipcc_support import header_constants, host_program, needs_host_cxx

PTR = 0x1000          # a pointer that is never followed: every call here fails its argument checks first
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def g11():
    return load_golden("g11_tsne.npz")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return host_program("tsne_plan_dump", tmp_path_factory.mktemp("tsne_plan"))


# ---------------------------------------------------------------- the restatement against scikit-learn's own results

def test_restatement_reproduces_the_fixture(g11):
    g = g11
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g11_tsne.npz")) < 200_000
    n = g["x"].shape[0]
    assert (n, g["x"].shape[1], float(g["perplexity"])) == (65, 16, 5.0)
    d2 = tsne_ref.sqdist(g["x"])
    assert np.array_equal(d2, g["d2"].astype(np.float64))                    # the float32-rounded distances, bit for bit
    P = tsne_ref.joint_probabilities(d2, float(g["perplexity"]))
    assert np.abs(P - g["P"]).max() <= 1e-12 * g["P"].max()
    assert np.array_equal(P, P.T) and (np.diag(P) == 0).all()
    margin = tsne_ref.perplexity_search(d2, float(g["perplexity"]))[2]
    print(f"g11: smallest stop margin of the perplexity search {margin:.3e}")
    assert margin > 1e-9
    assert tsne_ref.smallest_q(g["y_grad"]) > 1e3 * tsne_ref.EPS           # far from the floor the gradient leaves out
    kl, grad, _ = tsne_ref.kl_gradient(g["P"], g["y_grad"])
    assert abs(kl - float(g["kl"])) <= 1e-12 * abs(float(g["kl"]))
    assert np.abs(grad - g["grad"]).max() <= 1e-12 * np.abs(g["grad"]).max()
    lr = float(g["learning_rate"])
    for start, end, kl_end, ex, mom in ((g["y0"], g["y1"], g["kl1"], float(g["exaggeration"]), 0.5), (g["y1"], g["y2"], g["kl2"], 1.0, 0.8)):
        Y = start.copy()
        kl, _ = tsne_ref.steps(g["P"], Y, np.zeros_like(Y), np.ones_like(Y), 10, ex, mom, lr)
        assert np.abs(Y - end).max() <= 1e-9 * np.abs(end).max()
        assert abs(kl - float(kl_end)) <= 1e-9 * abs(float(kl_end))
    z, lam = tsne_ref.pca(g["x_pca"])
    assert lam[1] - lam[2] > 0.1 * lam[0] and lam[0] - lam[1] > 0.1 * lam[0]      # the gap the comparison relies on
    assert np.abs(z - g["pca"]).max() <= 1e-9 * np.abs(g["pca"]).max()


def test_restatement_equals_scikit_learns_private_functions():
    t_sne = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    from sklearn.decomposition import PCA
    from sklearn.manifold import trustworthiness
    from sklearn.preprocessing import StandardScaler
    for n, dim, perplexity, seed in ((200, 64, 30.0, 1), (37, 3, 2.0, 2)):
        x, labels = tsne_ref.planted(8, n // 8 + 1, dim, seed)
        x = x[:n]
        d2 = tsne_ref.sqdist(x)
        P = tsne_ref.joint_probabilities(d2, perplexity)
        want = squareform(t_sne._joint_probabilities(d2.astype(np.float32), perplexity, 0))
        assert np.abs(P - want).max() <= 1e-12 * want.max(), (n, dim)
        Y = np.random.default_rng(seed).standard_normal((n, 2))
        kl, grad = t_sne._kl_divergence(Y.ravel().copy(), squareform(want) * 12.0, 1.0, n, 2)
        got_kl, got_grad, _ = tsne_ref.kl_gradient(want, Y, 12.0)
        assert abs(got_kl - kl) <= 1e-12 * abs(kl)
        assert np.abs(got_grad - grad.reshape(n, 2)).max() <= 1e-12 * np.abs(grad).max()
        z = PCA(2).fit_transform(StandardScaler().fit_transform(x.astype(np.float64)))
        assert np.abs(tsne_ref.pca(x)[0] - z).max() <= 1e-9 * np.abs(z).max()
        assert abs(tsne_ref.trustworthiness(x, Y, 5) - trustworthiness(x.astype(np.float64), Y, n_neighbors=5)) <= 1e-12


def test_restated_schedule_is_scikit_learns():
    """TSNE._tsne itself with its two stages shortened to 5 + 5 iterations (a longer run cannot be compared point by point):
    the exaggeration, the momentum switch, the fresh update and gains of the second descent, kl_divergence_ and n_iter_."""
    manifold = pytest.importorskip("sklearn.manifold")
    from scipy.spatial.distance import squareform
    x, _ = tsne_ref.planted(4, 15, 8, seed=3)
    n = x.shape[0]
    y0 = 1e-4 * np.random.default_rng(0).standard_normal((n, 2))
    P = tsne_ref.joint_probabilities(tsne_ref.sqdist(x), 10.0)
    sk = manifold.TSNE(2, method="exact", max_iter=10)
    sk._EXPLORATION_MAX_ITER, sk._N_ITER_CHECK, sk.learning_rate_ = 5, 5, 50.0
    y_sk = sk._tsne(squareform(P, checks=False), 1, n, X_embedded=y0.copy())
    y, kl, it = tsne_ref.run(P, y0, max_iter=10, exploration=5, check=5)
    assert it == sk.n_iter_ == 9
    assert np.abs(y - y_sk).max() <= 1e-9 * np.abs(y_sk).max()
    assert abs(kl - sk.kl_divergence_) <= 1e-9 * sk.kl_divergence_


# ---------------------------------------------------------------- the host-only plan

def _spread():
    return list(range(2, 601)) + [601, 1023, 1024, 1025, 1200, 2047, 2048, 2049, 3000, 4095, 4096, 4097, 4874, 6000, 8191, 8192]


@needs_host_cxx
def test_row_groups_and_column_slices_cover_every_pair_once(plan):
    from xvector_amd import visualize
    cases = [(n, cus) for n in _spread() for cus in (1, 8, 64, 256, 304)]
    got = plan([f"plan {n} {cus}" for n, cus in cases])
    for (n, cus), line in zip(cases, got):
        rows, slices, cols, groups = (int(v) for v in line.split()[1:])
        assert rows in (4, 8, 16) and cols % 128 == 0 and 128 <= cols <= 2048, (n, cus, line)
        # rows: group g takes g * rows .. min(n, (g + 1) * rows) - 1; the groups are disjoint by construction, and they cover
        # 0 .. n - 1 exactly when the last one starts below n and ends at or past it (likewise the slices)
        assert (groups - 1) * rows < n <= groups * rows, (n, cus, line)
        assert (slices - 1) * cols < n <= slices * cols, (n, cus, line)
        assert slices <= -(-n // 128), (n, cus, line)                            # what the workspace is sized by
    # the plan fills the chip at the workload's size and is the smallest possible at n = 2
    assert plan(["plan 4874 256", "plan 2 256"]) == ["plan 16 4 1280 305", "plan 4 1 128 1"]
    assert 305 * 4 >= 4 * 256
    if hasattr(visualize._hip.lib, "xvec_tsne_plan"):                            # the export answers with the same plan
        assert visualize.tsne_plan(4874, 256) == (16, 4, 1280) and visualize.tsne_plan(2, 7) == (4, 1, 128)


@needs_host_cxx
def test_workspace_regions_do_not_overlap_and_end_at_the_reported_size(plan):
    from xvector_amd import hip
    cases = [(n, d) for n in _spread()[::7] + [2, 600, 4874, 8192] for d in (0, 1, 31, 512)]
    got = plan([f"layout {n} {d}" for n, d in cases])
    for (n, d), line in zip(cases, got):
        v = [int(t) for t in line.split()[1:]]
        x64, sqnorm, row_sum, scalars, partials, kl_part, norm_part, total, slices, blocks = v
        sizes = [n * d * 8, n * 8, n * 8, 32, slices * n * 5 * 8, slices * n * 8, blocks * 8]
        offs = [x64, sqnorm, row_sum, scalars, partials, kl_part, norm_part]
        assert offs[0] == 0 and all(o % 256 == 0 for o in offs), (n, d)
        for k in range(len(offs) - 1):
            assert offs[k] + sizes[k] <= offs[k + 1], (n, d, k)
        assert offs[-1] + sizes[-1] <= total < offs[-1] + sizes[-1] + 256, (n, d)
        assert slices == -(-n // 128) and blocks == -(-n // 256)
        assert hip.lib.xvec_tsne_workspace_bytes(n, d) == total, (n, d)
    for bad in ((1, 4), (8193, 4), (10, -1), (10, 65537)):
        assert hip.lib.xvec_tsne_workspace_bytes(*bad) == 0, bad


# ---------------------------------------------------------------- the header, the module and the C ABI without a device

def test_module_restates_the_header_and_refuses_the_cpu():
    import torch
    import xvector_amd
    from xvector_amd import hip, visualize
    consts = header_constants("xvec_tsne.h", "XVEC_TSNE_")
    assert consts["MAX_POINTS"] == visualize.MAX_POINTS == 8192 and consts["SEARCH_STEPS"] == tsne_ref.SEARCH_STEPS
    assert (consts["X_F32"], consts["X_F64"]) == (hip.TSNE_X_F32, hip.TSNE_X_F64)
    exports = {"xvec_tsne_last_error", "xvec_tsne_workspace_bytes", "xvec_tsne_plan", "xvec_tsne_sqdist", "xvec_tsne_affinities",
               "xvec_tsne_steps"}
    assert exports <= set(hip.EXPORTS) and all(hasattr(hip.lib, n) for n in exports)
    for name in ("Tsne", "tsne_map", "tsne_affinities", "pca_map", "scatter_maps"):
        assert getattr(xvector_amd, name) is getattr(visualize, name) and name in xvector_amd.__all__
    cpu = torch.zeros(10, 4)
    for call in (lambda: visualize.pca_map(cpu, device="cpu"), lambda: visualize.tsne_affinities(cpu, device="cpu"),
                 lambda: visualize.Tsne(cpu, device="cpu"), lambda: visualize.tsne_map(cpu, device="cpu"),
                 lambda: visualize.scatter_maps(cpu, np.arange(10), device="cpu")):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()
    # plot_images itself still raises: the plotting stays out of scope
    with pytest.raises(NotImplementedError):
        xvector_amd.evaluate.plda_score_stat_object.plot_images(None, None)


def test_pca_matrix_is_scikit_learns_components_with_the_scales_folded_in(g11):
    from xvector_amd.visualize import pca_matrix_from_scatter
    x = g11["x_pca"]
    n = x.shape[0]
    mean = x.mean(0)
    cov = (x - mean).T @ (x - mean) / n
    cov[3, 3] = 1e-33                                        # the constant column as a device sum may leave it: not exactly 0
    for standardize in (True, False):
        w = pca_matrix_from_scatter(mean, cov, n, 2, standardize)
        want = tsne_ref.pca(x, 2, standardize)[0]
        assert np.abs((x - mean) @ w - want).max() <= 1e-9 * np.abs(want).max()
    assert np.abs(tsne_ref.pca(x)[0] - g11["pca"]).max() <= 1e-9 * np.abs(g11["pca"]).max()
    with pytest.raises(ValueError, match="n_components = 17"):
        pca_matrix_from_scatter(mean, cov, n, 17)


def test_c_abi_argument_errors_return_before_any_device_call():
    from xvector_amd import hip
    lib, err = hip.lib, lambda: hip.lib.xvec_tsne_last_error().decode()
    n, d = 65, 16
    need = lib.xvec_tsne_workspace_bytes(n, d)
    good = dict(x=PTR, dt=hip.TSNE_X_F32, n=n, d=d, ldx=d, rnd=1, d2=PTR, ldd=n, perp=5.0, p=PTR, ldp=n, betas=None, comp=2, y=PTR,
                upd=PTR, gains=PTR, ldy=2, steps=1, ex=12.0, mom=0.5, lr=50.0, mg=0.01, kl=None, norm=None, ws=PTR, wsb=need)

    def sqdist(a):
        return lib.xvec_tsne_sqdist(*[a[k] for k in ("x", "dt", "n", "d", "ldx", "rnd", "d2", "ldd", "ws", "wsb")], None)

    def affinities(a):
        return lib.xvec_tsne_affinities(*[a[k] for k in ("d2", "ldd", "n", "perp", "p", "ldp", "betas", "ws", "wsb")], None)

    def steps(a):
        return lib.xvec_tsne_steps(*[a[k] for k in ("p", "ldp", "n", "comp", "y", "upd", "gains", "ldy", "steps", "ex", "mom", "lr",
                                                    "mg", "kl", "norm", "ws", "wsb")], None)

    points = [
        (dict(n=1), hip.ERR_ARG, "n = 1: need at least two points"),
        (dict(n=0), hip.ERR_ARG, "n = 0: need at least two points"),
        (dict(n=8193), hip.ERR_ARG, "n = 8193 is over XVEC_TSNE_MAX_POINTS = 8192"),
        (dict(ws=None), hip.ERR_ARG, "null pointer: workspace"),
        (dict(ws=PTR + 4), hip.ERR_ARG, "workspace is not 8-byte aligned"),
        (dict(wsb=need - 1), hip.ERR_WORKSPACE, None),
    ]
    cases = {
        sqdist: points + [
            (dict(dt=2), hip.ERR_ARG, "unknown x_dtype 2"),
            (dict(d=0), hip.ERR_ARG, "d = 0 must lie in 1 .. XVEC_TSNE_MAX_DIM = 65536"),
            (dict(d=65537, ldx=65537), hip.ERR_ARG, "d = 65537 must lie in 1 .. XVEC_TSNE_MAX_DIM = 65536"),
            (dict(x=None), hip.ERR_ARG, "null pointer: x"),
            (dict(x=PTR + 2), hip.ERR_ARG, "x is not 4-byte aligned"),
            (dict(x=PTR + 4, dt=hip.TSNE_X_F64), hip.ERR_ARG, "x is not 8-byte aligned"),
            (dict(ldx=15), hip.ERR_ARG, "x row stride 15 is smaller than d = 16"),
            (dict(d2=None), hip.ERR_ARG, "null pointer: d2"),
            (dict(d2=PTR + 4), hip.ERR_ARG, "d2 is not 8-byte aligned"),
            (dict(ldd=64), hip.ERR_ARG, "d2 row stride 64 is smaller than its 65 columns"),
        ],
        affinities: points + [
            (dict(perp=0.0), hip.ERR_ARG, "perplexity = 0 must be finite, positive and below n = 65"),
            (dict(perp=-3.0), hip.ERR_ARG, "perplexity = -3 must be finite, positive and below n = 65"),
            (dict(perp=65.0), hip.ERR_ARG, "perplexity = 65 must be finite, positive and below n = 65"),
            (dict(perp=NAN), hip.ERR_ARG, "perplexity = nan must be finite, positive and below n = 65"),
            (dict(perp=INF), hip.ERR_ARG, "perplexity = inf must be finite, positive and below n = 65"),
            (dict(d2=None), hip.ERR_ARG, "null pointer: d2"),
            (dict(ldd=64), hip.ERR_ARG, "d2 row stride 64 is smaller than its 65 columns"),
            (dict(p=None), hip.ERR_ARG, "null pointer: p"),
            (dict(ldp=1), hip.ERR_ARG, "p row stride 1 is smaller than its 65 columns"),
            (dict(betas=PTR + 1), hip.ERR_ARG, "betas is not 8-byte aligned"),
        ],
        steps: points + [
            (dict(comp=3), hip.ERR_ARG, "n_components = 3: only two output dimensions"),
            (dict(comp=1), hip.ERR_ARG, "n_components = 1: only two output dimensions"),
            (dict(steps=0), hip.ERR_ARG, "n_steps = 0: need at least one iteration"),
            (dict(ex=0.0), hip.ERR_ARG, "exaggeration = 0 must be finite and positive"),
            (dict(ex=NAN), hip.ERR_ARG, "exaggeration = nan must be finite and positive"),
            (dict(mom=-0.5), hip.ERR_ARG, "momentum = -0.5 must be finite and not negative"),
            (dict(lr=INF), hip.ERR_ARG, "learning_rate = inf must be finite and positive"),
            (dict(mg=NAN), hip.ERR_ARG, "min_gain = nan must be finite and not negative"),
            (dict(p=None), hip.ERR_ARG, "null pointer: p"),
            (dict(ldp=64), hip.ERR_ARG, "p row stride 64 is smaller than its 65 columns"),
            (dict(y=None), hip.ERR_ARG, "null pointer: y"),
            (dict(upd=None), hip.ERR_ARG, "null pointer: update"),
            (dict(gains=None), hip.ERR_ARG, "null pointer: gains"),
            (dict(ldy=1), hip.ERR_ARG, "y row stride 1 is smaller than its 2 columns"),
            (dict(kl=PTR + 4), hip.ERR_ARG, "kl_out or grad_norm_out is not 8-byte aligned"),
        ],
    }
    for entry, rows in cases.items():
        name = "xvec_tsne_" + entry.__name__
        for kwargs, code, text in rows:
            a = {**good, **kwargs}
            if "wsb" in kwargs:                              # (sqdist alone sizes the workspace with d)
                full = lib.xvec_tsne_workspace_bytes(n, d if entry is sqdist else 0)
                a["wsb"] = full - 1
                text = f"workspace too small: {full - 1} < {full} bytes"
            else:
                text = f"{name}: {text}"
            assert entry(a) == code, (name, kwargs)
            assert err() == text, (name, kwargs)
    out = (hip.C.c_int32 * 3)()
    assert lib.xvec_tsne_plan(1, 4, out, out, out) == hip.ERR_ARG and err() == "xvec_tsne_plan: n = 1: need at least two points"
    assert lib.xvec_tsne_plan(10, 4, None, out, out) == hip.ERR_ARG and err() == "xvec_tsne_plan: null pointer"


def test_tsne_error_channel_is_its_own_and_per_thread():
    from xvector_amd import hip
    lib = hip.lib
    assert lib.xvec_mfcc_create(None, None) == hip.ERR_ARG
    assert lib.xvec_vad_energy(None, 0, 1, 1, 1, 1, None, None, None, 1, None, None, None) == hip.ERR_ARG
    assert lib.xvec_tsne_affinities(None, 0, 1, 5.0, None, 0, None, None, 0, None) == hip.ERR_ARG
    want = "xvec_tsne_affinities: n = 1: need at least two points"
    others = ((lib.xvec_mfcc_last_error, "null argument"), (lib.xvec_vad_last_error, "B = 0, T = 1, C = 1: every one must be at least 1"))
    assert lib.xvec_tsne_last_error().decode() == want and all(f().decode() == t for f, t in others)
    assert lib.xvec_gemm_nt_f64(None, 0, None, 0, -1, 0, 1, None, None, 0.0, 1.0, None, 0, None) == hip.ERR_ARG
    assert lib.xvec_tsne_last_error().decode() == want         # a later error of the product it calls leaves the text alone
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.xvec_tsne_last_error().decode()))
    t.start()
    t.join()
    assert seen == [""] and lib.xvec_tsne_last_error().decode() == want


# ---------------------------------------------------------------- the schedule on a fake stepper

class _Fake:
    """Answers step(count, exaggeration, momentum, learning_rate, fresh) from chosen KL / norm sequences, one entry per check."""

    def __init__(self, kls, norms=None):
        self.kls, self.norms, self.calls, self.done, self.fresh = list(kls), norms, [], 0, []

    def __call__(self, count, exaggeration, momentum, lr, fresh):
        self.calls.append((self.done, count, exaggeration, momentum, lr))
        if fresh:
            self.fresh.append(self.done)
        self.done += count
        k = len(self.calls) - 1
        return self.kls[min(k, len(self.kls) - 1)], (1.0 if self.norms is None else self.norms[min(k, len(self.norms) - 1)])


def test_schedule_switches_at_250_and_runs_to_max_iter():
    from xvector_amd.visualize import run_schedule
    fake = _Fake([5.0 - 0.01 * k for k in range(40)])          # always improving: no stop rule fires
    kl, it = run_schedule(fake, 4874)
    assert it == 999 and fake.done == 1000 and kl == fake.kls[19]
    lr = 4874 / 12.0 / 4.0
    assert [c[:2] for c in fake.calls] == [(50 * k, 50) for k in range(20)]
    assert all(c[2:] == (12.0, 0.5, lr) for c in fake.calls[:5]) and all(c[2:] == (1.0, 0.8, lr) for c in fake.calls[5:])
    assert fake.fresh == [0, 250]               # each of scikit-learn's two descents starts from a zero update and unit gains
    # 'auto' has a floor of 50; a number is taken as it is; a last stretch shorter than 50 still reports
    fake = _Fake([1.0])
    run_schedule(fake, 65, max_iter=270, early_exaggeration=4.0, learning_rate="auto")
    assert fake.calls[0][2:] == (4.0, 0.5, 50.0) and [c[:2] for c in fake.calls[5:]] == [(250, 20)]
    fake = _Fake([1.0])
    run_schedule(fake, 65, learning_rate=200.0)
    assert fake.calls[0][4] == 200.0
    with pytest.raises(ValueError, match="at least 250"):
        run_schedule(_Fake([1.0]), 65, max_iter=200)
    # the restatement's schedule is the same function of the same stepper
    a, b = _Fake([5.0, 4.0, 4.5, 4.4]), _Fake([5.0, 4.0, 4.5, 4.4])
    assert run_schedule(a, 300, max_iter=700, n_iter_without_progress=100) == tsne_ref.schedule(b, 300, max_iter=700, n_iter_without_progress=100)
    assert a.calls == b.calls


def test_schedule_stops_without_progress_and_on_a_small_gradient():
    from xvector_amd.visualize import run_schedule
    # second stage: the best KL at iteration 299 (the first check), none better after; it stops at the first check whose index
    # is MORE than 100 past 299: 449 (449 - 299 = 150 > 100; 399 - 299 = 100 is not)
    fake = _Fake([9.0, 8.0, 7.0, 6.0, 5.0] + [1.0] + [2.0] * 20)
    kl, it = run_schedule(fake, 300, n_iter_without_progress=100)
    assert (kl, it, fake.done) == (2.0, 449, 450)
    # first stage: patience 250 can never run out within 250 iterations, so a flat KL there changes nothing
    fake = _Fake([3.0] * 5 + [2.0 - 0.01 * k for k in range(30)])
    assert run_schedule(fake, 300)[1] == 999
    # a small gradient norm at a check of the first stage ends that stage only: the second starts at the next iteration
    fake = _Fake([5.0 - 0.1 * k for k in range(30)], norms=[1.0, 1e-8] + [1.0] * 30)
    kl, it = run_schedule(fake, 300, max_iter=400)
    assert [c[:4] for c in fake.calls] == [(0, 50, 12.0, 0.5), (50, 50, 12.0, 0.5), (100, 50, 1.0, 0.8), (150, 50, 1.0, 0.8),
                                           (200, 50, 1.0, 0.8), (250, 50, 1.0, 0.8), (300, 50, 1.0, 0.8), (350, 50, 1.0, 0.8)]
    assert it == 399 and fake.fresh == [0, 100]
    # ... and in the second stage it ends the run; the norm at the bound itself stops too
    fake = _Fake([5.0 - 0.1 * k for k in range(30)], norms=[1.0] * 6 + [1e-7])
    kl, it = run_schedule(fake, 300)
    assert (it, fake.done, kl) == (349, 350, fake.kls[6])
