"""PLDA training, CPU half: the package's host EM (xvector_amd.plda.host_em) against the literal restatement of
speechbrain's loop (tests/plda_em_ref.py, unpinned), the speechbrain-shaped surface, the C ABI's argument checks and the
kernels' resources.  The device half is tests/test_plda_train_gpu.py."""
import pickle
import re

import numpy as np
import pytest

import plda_em_ref as ref
from hipcc_support import kernel_resources, needs_hipcc


def numpy_products(sums_centred, counts):
    """What xvec_plda_em_products computes, in numpy float64 (the test's stand-in for the device)."""
    def products(pq, lam):
        H = (sums_centred @ pq) / (counts[:, None] * lam[None, :] + 1.0)
        return H.T @ H, H.T @ (counts[:, None] * H), H.T @ sums_centred
    return products


def em_inputs(C, dim, R, seed):
    """Seeded E-step inputs (class_sums [C, dim], counts [C], pq_t [R, dim], lam [R]): normal sums, counts k / 2 with
    k in 1 .. 60 (neither 1 nor always an integer), lam positive over three decades, pq of unit-norm-like columns."""
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (C, dim)), rng.integers(1, 61, C) * 0.5, rng.normal(0, 1, (R, dim)) / np.sqrt(dim),
            10.0 ** rng.uniform(-1.5, 1.5, R))


EM_SHAPES = [(1, 1, 1), (3, 5, 5), (130, 37, 7), (129, 64, 64), (257, 200, 50), (1211, 512, 200)]


def em_reference(sums, counts, pq_t, lam):
    """numpy_products in np.longdouble: (H'H, H' diag(n) H, H'S)."""
    ld = lambda a: np.asarray(a, dtype=np.longdouble)
    return numpy_products(ld(sums), ld(counts))(ld(pq_t).T, ld(lam))


@pytest.mark.parametrize("C,dim,R", EM_SHAPES[:5])
def test_em_products_bound_covers_float64_numpy(C, dim, R):
    """The bound the device E-step is held to (plda_em_ref.em_products_bound) is not tighter than float64's own rounding:
    numpy_products in float64 stays inside it against the longdouble evaluation."""
    sums, counts, pq_t, lam = em_inputs(C, dim, R, C + dim + R)
    got = numpy_products(sums, counts)(pq_t.T.copy(), lam)
    want = em_reference(sums, counts, pq_t, lam)
    bound = ref.em_products_bound(sums, counts, pq_t.T, lam)
    for g, w, b, name in zip(got, want, bound, ("hh", "nhh", "hs")):
        assert g.shape == w.shape == b.shape and (b > 0).all()
        ratio = float((np.abs(g - w) / b).max())
        print(f"C={C} dim={dim} R={R} {name}: float64 numpy error / bound = {ratio:.3f}")
        assert ratio <= 1.0, (name, ratio)


def host_fit(x, labels, rank_f, nb_iter=10, scaling_factor=1.0):
    from xvector_amd import plda
    mean, sigma_obs, _, counts, sums = ref.class_stats(x, labels, scaling_factor)
    F, Sigma = plda.host_em(sigma_obs, counts, rank_f, nb_iter, numpy_products(sums - counts[:, None] * mean, counts))
    return mean, F, Sigma


@pytest.mark.parametrize("rank_f,scaling_factor,string_labels", [(1, 1.0, False), (12, 1.0, True), (12, 0.5, False),
                                                                 (24, 0.5, True)])
def test_host_em_matches_restatement(rank_f, scaling_factor, string_labels):
    dim = 24
    x, labels, _ = ref.make_data(60, dim, 6, sizes=(1, 12), seed=rank_f)
    labels = labels.copy()
    labels[0] = 10_000                       # a class of exactly one row
    if string_labels:
        labels = np.array(["id" + str(v) for v in labels], dtype=object)
    want = ref.plda_em(x, labels, rank_f, 10, scaling_factor)
    got = host_fit(x, labels, rank_f, 10, scaling_factor)
    assert ref.rel(got[0], want[0]) <= 1e-10
    assert ref.rel(got[1] @ got[1].T, want[1] @ want[1].T) <= 1e-10
    assert ref.rel(got[2], want[2]) <= 1e-10


def test_host_em_rejects_bad_rank():
    from xvector_amd import plda
    with pytest.raises(ValueError):
        plda.host_em(np.eye(4), np.ones(3), 5, 1, None)
    with pytest.raises(ValueError):
        plda.host_em(np.eye(4), np.ones(3), 0, 1, None)


def test_surface_and_pickle(tmp_path):
    from xvector_amd import plda
    import xvector_amd as xa
    assert xa.PLDA is plda.PLDA and xa.PldaStats is plda.PldaStats and xa.StatObject is plda.StatObject
    xv = np.arange(12.0).reshape(4, 3)
    st = plda.get_train_x_vec(xv, [3, 3, 7, 1], ["a", "b", "c", "d"])
    assert list(st.modelset) == ["id3", "id3", "id7", "id1"] and list(st.segset) == ["a", "b", "c", "d"]
    assert st.stat0.shape == (4, 1) and st.stat1 is xv
    es = plda.get_x_vec_stat(xv, [5, 6, 7, 8])
    assert list(es.modelset) == list(es.segset) == ["5", "6", "7", "8"]
    p = plda.setup_plda(rank_f=2, nb_iter=3)
    assert (p.rank_f, p.nb_iter, p.scaling_factor, p.mean, p.F, p.Sigma) == (2, 3, 1, None, None, None)
    p.mean, p.F, p.Sigma = np.zeros(3), np.ones((3, 2)), np.eye(3)
    path = tmp_path / "plda.pkl"
    plda.save_plda(p, str(path))
    q = plda.load_plda(str(path))
    assert np.array_equal(q.F, p.F) and np.array_equal(q.Sigma, p.Sigma) and q.rank_f == 2
    assert pickle.loads(pickle.dumps(p)).nb_iter == 3
    with pytest.raises(NotImplementedError):
        p.plda(st, whiten=True)


def test_training_refuses_cpu_device():
    from xvector_amd import plda
    with pytest.raises(RuntimeError):
        plda.PldaStats(np.zeros((4, 3)), [0, 0, 1, 1], device="cpu")


def test_plda_abi_argument_errors_without_gpu():
    import ctypes as C
    from xvector_amd import hip
    lib = hip.lib
    start = (C.c_int64 * 3)(0, 2, 4)
    args = lambda **kw: [kw.get("x", 1), 0, kw.get("n", 4), kw.get("dim", 3), kw.get("order", 1), kw.get("start", start),
                         kw.get("c", 2), 1.0, 1, 1, 1, 1, 1, 1, 1 << 30, None]
    assert lib.xvec_plda_stats(*args(n=1)) == hip.ERR_ARG and b"two" in lib.xvec_plda_last_error()
    assert lib.xvec_plda_stats(*args(c=0)) == hip.ERR_ARG
    assert lib.xvec_plda_stats(*args(dim=0)) == hip.ERR_ARG
    assert lib.xvec_plda_stats(*args(x=None)) == hip.ERR_ARG and b"null" in lib.xvec_plda_last_error()
    assert lib.xvec_plda_stats(*args(order=None)) == hip.ERR_ARG
    assert lib.xvec_plda_stats(*args(start=None)) == hip.ERR_ARG
    assert lib.xvec_plda_stats(*args(n=5)) == hip.ERR_ARG and b"class_start" in lib.xvec_plda_last_error()
    bad = (C.c_int64 * 3)(0, 3, 2)
    assert lib.xvec_plda_stats(*args(start=bad, n=2)) == hip.ERR_ARG and b"decreases" in lib.xvec_plda_last_error()
    # a valid set of arguments with a workspace that is too small never reaches the device
    small = args()
    small[-2] = 8
    assert lib.xvec_plda_stats(*small) == hip.ERR_WORKSPACE
    assert lib.xvec_plda_stats_workspace_bytes(1, 3, 1) == 0
    assert lib.xvec_plda_stats_workspace_bytes(400_000, 512, 1211) > 0
    em = lambda **kw: [kw.get("p", 1), 1, 1, 1, 1, kw.get("c", 10), kw.get("dim", 8), kw.get("rank", 4), 1, 1, 1 << 30, None]
    assert lib.xvec_plda_em_products(*em(rank=9)) == hip.ERR_ARG and b"rank_f" in lib.xvec_plda_last_error()
    assert lib.xvec_plda_em_products(*em(c=0)) == hip.ERR_ARG
    assert lib.xvec_plda_em_products(*em(p=None)) == hip.ERR_ARG and b"null" in lib.xvec_plda_last_error()
    assert lib.xvec_plda_em_workspace_bytes(0, 4) == 0 and lib.xvec_plda_em_workspace_bytes(10, 4) > 0


@needs_hipcc
def test_plda_kernels_use_no_scratch():
    kernels = kernel_resources("plda_train.hip")
    assert len(kernels) == 10, sorted(kernels)    # class sums x2, mean, centre, scatter x4, reduce, E-step scale
    for k, r in kernels.items():
        assert r.get("scratch", 0) == 0 and r.get("spill", 0) == 0, f"{k}: {r}"
        assert r.get("vgprs", 0) + r.get("agprs", 0) <= 256, f"{k}: {r}"
    # the kernels of csrc/class_scatter.h as this file instantiates them; the scatter kernel's two double-buffered 16 x 80
    # images and __launch_bounds__(256, 4), as in tests/test_lda_resources.py
    scatter = [k for k in kernels if re.search(r"\dclass_scatter_kernelI[fd]Lb[01]ELb0EE", k)]      # <T, VEC, PER_ROW = false>
    assert len(scatter) == 4 and not any("class_scatter_kernel" in k for k in set(kernels) - set(scatter)), sorted(kernels)
    for k in scatter:
        assert kernels[k]["lds"] == 2 * 2 * 16 * 80 * 8 == 40960 and kernels[k]["occupancy"] == 4, f"{k}: {kernels[k]}"
    for want in ("plda_class_sum_kernelI", "stats_mean_kernelE", "class_scatter_reduce_kernelE"):
        assert any(re.search(rf"\d{want}", k) for k in kernels), (want, sorted(kernels))
