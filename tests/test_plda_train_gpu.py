"""PLDA training on the device (include/xvec_plda.h, xvector_amd.plda): the statistics pass against numpy float64, bit-for-bit
repeatability, full fits against the literal restatement of speechbrain's loop (tests/plda_em_ref.py, unpinned) and the
trained model's scores against the true model's."""
import numpy as np
import pytest
import torch

import plda_em_ref as ref

DEV = "cuda:0"


def _stats_ref(x, labels, sf):
    mean, sigma_obs, classes, counts, sums = ref.class_stats(x, labels, sf)
    return mean, sigma_obs, classes, counts, sums - counts[:, None] * mean, sums


@pytest.mark.gpu
@pytest.mark.parametrize("n_classes,dim,sizes,dtype,sf", [
    (1, 40, (777, 777), "f64", 1.0),          # one class; N not a multiple of any tile
    (7, 200, (1, 300), "f32", 0.5),           # dim not a multiple of 64
    (300, 512, (1, 9), "f64", 1.0),           # many classes of one or a few rows
    (1211, 512, (1, 60), "f32", 1.0),
    (50, 37, (1, 80), "f32", 1.0),            # dim % 4 != 0: the element-wise staging
])
def test_stats_match_numpy(n_classes, dim, sizes, dtype, sf):
    from xvector_amd import plda
    x, labels, _ = ref.make_data(n_classes, dim, min(8, dim), sizes=sizes, seed=n_classes + dim)
    if dtype == "f32":
        x = x.astype(np.float32)
    st = plda.PldaStats(torch.from_numpy(x).to(DEV), labels, scaling_factor=sf)
    mean, sigma_obs, classes, counts, cls, raw = _stats_ref(x.astype(np.float64), labels, sf)
    assert np.array_equal(st.classes, classes) and np.array_equal(st.counts, counts)
    assert ref.rel(st.mean, mean) <= 1e-12
    assert ref.rel(st.sigma_obs, sigma_obs) <= 1e-12
    # relative to the uncentred sums: with one class the centred sum is zero up to the cancellation's rounding
    assert np.linalg.norm(st.class_sums() - cls) <= 1e-12 * np.linalg.norm(raw)
    assert np.array_equal(st.sigma_obs, st.sigma_obs.T)
    assert np.array_equal(st._cls_t.cpu().numpy(), st.class_sums().T)


@pytest.mark.gpu
def test_stats_are_bit_identical_across_runs_and_poisoned_workspace():
    from xvector_amd import hip, plda
    x, labels, _ = ref.make_data(200, 512, 16, sizes=(1, 50), seed=5)
    xt = torch.from_numpy(x).to(DEV)
    a = plda.PldaStats(xt, labels)
    # the same call by hand with every output and the workspace filled with NaN first
    classes, order, start = plda._labels(labels, x.shape[0])
    n, dim, C = x.shape[0], x.shape[1], classes.shape[0]
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=DEV)
    mean, counts, cls, cls_t, sigma = nan(dim), nan(C), nan(C, dim), nan(dim, C), nan(dim, dim)
    wsb = int(hip.lib.xvec_plda_stats_workspace_bytes(n, dim, C))
    ws = nan((wsb + 7) // 8)
    rc = hip.lib.xvec_plda_stats(xt.data_ptr(), hip.PLDA_X_F64, n, dim, torch.from_numpy(order).to(DEV).data_ptr(),
                                 start.ctypes.data_as(hip.C.POINTER(hip.C.c_int64)), C, 1.0, mean.data_ptr(), counts.data_ptr(),
                                 cls.data_ptr(), cls_t.data_ptr(), sigma.data_ptr(), ws.data_ptr(), wsb,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.xvec_plda_last_error()
    b = plda.PldaStats(xt, labels)
    for u, v in ((a.mean, mean), (a.sigma_obs, sigma), (a.class_sums(), cls), (a.counts, counts), (b.sigma_obs, sigma),
                 (b.class_sums(), cls)):
        v = v.cpu().numpy() if torch.is_tensor(v) else v
        assert np.array_equal(u, v)
    fa = a.fit(20, 5)
    fb = b.fit(20, 5)
    for u, v in zip(fa, fb):
        assert np.array_equal(u, v)


@pytest.mark.gpu
@pytest.mark.parametrize("rank_f", [50, 200])
def test_fit_matches_restatement(rank_f):
    from xvector_amd import plda
    x, labels, _ = ref.make_data(400, 512, 64, sizes=(20, 280), seed=rank_f)
    assert 50_000 <= x.shape[0] <= 70_000
    want = ref.plda_em(x, labels, rank_f, 10)
    st = plda.PldaStats(torch.from_numpy(x.astype(np.float64)).to(DEV), labels)
    got = st.fit(rank_f, 10)
    assert ref.rel(got[0], want[0]) <= 1e-8
    assert ref.rel(got[1] @ got[1].T, want[1] @ want[1].T) <= 1e-8
    assert ref.rel(got[2], want[2]) <= 1e-8
    # fits from one reused PldaStats equal fresh fits bit for bit (another rank in between)
    st.fit(7, 3)
    again = st.fit(rank_f, 10)
    fresh = plda.PldaStats(torch.from_numpy(x).to(DEV), labels).fit(rank_f, 10)
    for u, v, w in zip(got, again, fresh):
        assert np.array_equal(u, v) and np.array_equal(u, w)


@pytest.mark.gpu
def test_trained_model_scores_like_the_true_model():
    from xvector_amd import plda, scoring
    dim, rank = 64, 10
    x, labels, (mu, F_true, Sigma_true) = ref.make_data(1000, dim, rank, sizes=(5, 30), seed=11)
    tr = plda.get_train_x_vec(x.astype(np.float32), labels, np.arange(x.shape[0]))
    model = plda.train_plda(plda.setup_plda(rank_f=rank, nb_iter=10), tr)
    # held-out speakers: 60 of them, 5 vectors each, scored all against all
    rng = np.random.default_rng(13)
    y = rng.normal(0, 1, (60, rank))
    L = np.linalg.cholesky(Sigma_true)
    lab = np.repeat(np.arange(60), 5)
    held = mu + (y @ F_true.T)[lab] + rng.normal(0, 1, (lab.shape[0], dim)) @ L.T
    got = scoring.PldaScorer(model.mean, model.F, model.Sigma).score(held).cpu().numpy()
    true = scoring.PldaScorer(mu, F_true, Sigma_true).score(held).cpu().numpy()
    iu = np.triu_indices(held.shape[0], 1)
    r = np.corrcoef(got[iu], true[iu])[0, 1]
    assert r >= 0.999, r
    st = plda.get_x_vec_stat(held, np.arange(held.shape[0]))
    s = scoring.plda_scores(model, st, st)
    assert np.allclose(s.scoremat, got, rtol=1e-9, atol=1e-9 * np.abs(got).max())


@pytest.mark.gpu
def test_full_size_fit():
    """The reference's training shape: ~400 000 rows of 512, 1211 classes, rank 200, 10 iterations, fp32 from the device."""
    from xvector_amd import plda
    x, labels, _ = ref.make_data(1211, 512, 150, sizes=(100, 560), seed=1)
    assert 350_000 <= x.shape[0] <= 450_000
    xt = torch.from_numpy(x.astype(np.float32)).to(DEV)
    st = plda.PldaStats(xt, labels)
    x32 = x.astype(np.float32).astype(np.float64)
    mean = x32.mean(0)
    assert ref.rel(st.mean, mean) <= 1e-12
    xc = x32 - mean
    assert ref.rel(st.sigma_obs, xc.T @ xc / x.shape[0]) <= 1e-12
    m, F, Sigma = st.fit(200, 10)
    assert F.shape == (512, 200) and Sigma.shape == (512, 512)
    assert np.isfinite(F).all() and np.isfinite(Sigma).all()
    assert np.linalg.eigvalsh(0.5 * (Sigma + Sigma.T)).min() > 0
    assert st.last_fit_timing["device_s"] > 0
