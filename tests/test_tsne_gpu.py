"""Exact t-SNE and the PCA map on the device (csrc/tsne.hip, include/xvec_tsne.h, xvector_amd.visualize) against the numpy
restatement tests/tsne_ref.py and the fixture written from scikit-learn (tests/golden/g11_tsne.npz).  scikit-learn itself is not
needed here.  Shapes sit where the kernels can go wrong -- n = 2, sizes around the 32-wide symmetrising tile, the 256 threads
of a row's block, the 128-column slice step and the row groups of the plan the device reports -- not at the workload's size.

Bounds.  Distances: derived below from the Gram form.  P, the gradient, its norm and the KL value: 1e-12 of the largest entry
(the orders of the sums differ from numpy's; at most a few thousand terms of one sign or of bounded ratio, 1e-16 each).
Trajectories: 1e-9 of the largest coordinate after ten iterations and no further -- t-SNE's descent amplifies a 1e-13 relative
change of the start to 1e-12 after 10 iterations, to 1e-6 .. 1e-2 after 50, and after 100 two runs are unrelated -- so the whole
optimisation is compared by quality (KL divergence, trustworthiness, 1-NN label accuracy) against the spread the restatement
itself shows under 1e-13 relative noise on its start.

Every call passes strides larger than the extent somewhere, NaN in the workspace, and sentinels behind what it may write."""
import threading

import numpy as np
import pytest
import torch

import tsne_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
EPS = float(np.finfo(np.float64).eps)
SENTINEL = -777.25


@pytest.fixture(scope="module")
def g11():
    return load_golden("g11_tsne.npz")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _padded(host, ld, offset=0, dtype=torch.float64):
    """(flat NaN-filled buffer, view [rows, cols] of row stride ld starting `offset` elements in) holding `host`."""
    rows, cols = host.shape
    flat = torch.full((rows * ld + offset + 8,), NAN, dtype=dtype, device=DEV)
    view = flat[offset:].as_strided((rows, cols), (ld, 1))
    view.copy_(_dev(host, dtype))
    return flat, view


class _Workspace:
    """NaN-filled, exactly the reported size inside a larger buffer whose rest must come back untouched."""

    def __init__(self, n, d=0, fill=NAN):
        from xvector_amd import hip
        self.bytes = int(hip.lib.xvec_tsne_workspace_bytes(n, d))
        assert self.bytes > 0 and self.bytes % 8 == 0
        self.buf = torch.full((self.bytes // 8 + 64,), SENTINEL, dtype=torch.float64, device=DEV)
        self.buf[32:32 + self.bytes // 8] = fill
        self.ptr = self.buf.data_ptr() + 256

    def check(self):
        torch.cuda.synchronize()
        assert (self.buf[:32] == SENTINEL).all() and (self.buf[32 + self.bytes // 8:] == SENTINEL).all(), "wrote outside the workspace"


def _check(rc):
    from xvector_amd import hip
    assert rc == hip.OK, hip.lib.xvec_tsne_last_error().decode()


# ---------------------------------------------------------------- distances

def _sqdist(x_view, round_f32, ldd=None):
    from xvector_amd import hip
    n, d = x_view.shape
    ldd = n + 3 if ldd is None else ldd
    out = torch.full((n * ldd + 8,), SENTINEL, dtype=torch.float64, device=DEV)
    ws = _Workspace(n, d)
    dt = hip.TSNE_X_F32 if x_view.dtype == torch.float32 else hip.TSNE_X_F64
    _check(hip.lib.xvec_tsne_sqdist(x_view.data_ptr(), dt, n, d, x_view.stride(0), int(round_f32), out.data_ptr(), ldd, ws.ptr,
                                    ws.bytes, _stream()))
    ws.check()
    full = out[:n * ldd].view(n, ldd).cpu().numpy()
    assert (full[:, n:] == SENTINEL).all() and (out[n * ldd:] == SENTINEL).all(), "wrote into the padding of d2"
    return full[:, :n].copy()


@pytest.mark.parametrize("n,d", [(2, 1), (63, 2), (64, 31), (65, 64), (257, 512), (65, 1), (2, 512), (257, 31)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_sqdist_inside_the_gram_form_bound(n, d, dtype):
    """Every term below is relative to a + b = |x_i|^2 + |x_j|^2, in units of u = eps / 2.  The Gram entry g is a sum of d
    products (each rounded, however the matrix pipe orders them): off by at most d u sum_k |x_ik x_jk| <= d u (a + b) / 2, and
    it enters doubled: d u (a + b).  Each norm is a sum of d rounded squares through at most d additions, lane partials and
    butterfly included: (d + 7) u a, together (d + 7) u (a + b).  The two additions (-2 g + a) + b round partial results no
    larger than 2 (a + b): 4 u (a + b).  The clamp at 0 only moves a value towards the true one.  Sum: (2 d + 11) u (a + b) =
    c eps (a + b) with c = d + 6.  fp32 input is exact in fp64, and the np.longdouble reference's own error is 2^-11 of u."""
    c = d + 6
    rng = np.random.default_rng(1000 * n + d)
    host = (rng.standard_normal((n, d)) * 3.0 + 1.0).astype(np.float32 if dtype == torch.float32 else np.float64)
    _, view = _padded(host, d + 5, offset=1, dtype=dtype)            # a padded stride and a base one element off any 16 bytes
    got = _sqdist(view, False)
    xl = host.astype(np.longdouble)
    sq = (xl ** 2).sum(1)
    want = ((xl[:, None, :] - xl[None, :, :]) ** 2).sum(-1) if n * n * d <= 1 << 22 else sq[:, None] + sq[None, :] - 2 * (xl @ xl.T)
    bound = c * EPS * (sq[:, None] + sq[None, :])
    err = np.abs(got.astype(np.longdouble) - want)
    print(f"sqdist n={n} d={d} {dtype}: worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert (np.diag(got) == 0.0).all() and (got >= 0.0).all()
    rounded = _sqdist(view, True)
    assert np.array_equal(rounded, got.astype(np.float32).astype(np.float64))      # exactly float32(D2)
    dense = _sqdist(_dev(host, dtype), False, ldd=n)                                # a dense, aligned call: the same bits
    assert np.array_equal(dense, got)


def test_sqdist_of_the_fixture_rounds_to_scikit_learns_distances(g11):
    from xvector_amd import visualize
    got = visualize.squared_distances(g11["x"], device=DEV).cpu().numpy()
    want = g11["d2"].astype(np.float64)
    # float32 rounding of two fp64 results that differ in their last bits: equal except where one sits on a rounding boundary
    off = got != want
    assert off.mean() <= 1e-3 and np.abs(got - want).max() <= 2.0 ** -23 * want.max()


# ---------------------------------------------------------------- affinities

def _affinities(d2, perplexity, ldd=None, ldp=None, want_betas=True):
    from xvector_amd import hip
    n = d2.shape[0]
    ldd, ldp = n + 1 if ldd is None else ldd, n + 2 if ldp is None else ldp
    _, dv = _padded(d2, ldd)
    out = torch.full((n * ldp + 8,), SENTINEL, dtype=torch.float64, device=DEV)
    betas = torch.full((n + 4,), SENTINEL, dtype=torch.float64, device=DEV)
    ws = _Workspace(n)
    _check(hip.lib.xvec_tsne_affinities(dv.data_ptr(), ldd, n, float(perplexity), out.data_ptr(), ldp,
                                        betas.data_ptr() if want_betas else None, ws.ptr, ws.bytes, _stream()))
    ws.check()
    full = out[:n * ldp].view(n, ldp).cpu().numpy()
    assert (full[:, n:] == SENTINEL).all() and (out[n * ldp:] == SENTINEL).all() and (betas[n:] == SENTINEL).all()
    return full[:, :n].copy(), betas[:n].cpu().numpy()


def _check_affinities(d2, perplexity, want=None, what=""):
    C, betas, margin, steps = tsne_ref.perplexity_search(d2, perplexity)
    print(f"affinities {what}: smallest stop margin {margin:.3e}, steps {steps.min()} .. {steps.max()}")
    assert margin > 1e-9, "choose another seed: a row's stop test sits within rounding of its bound"
    want = tsne_ref.joint_probabilities(d2, perplexity) if want is None else want
    got, got_betas = _affinities(d2, perplexity)
    assert np.abs(got - want).max() <= 1e-12 * want.max()
    assert np.array_equal(got, got.T) and (np.diag(got) == 0.0).all() and (got[~np.eye(len(got), dtype=bool)] >= EPS).all()
    assert np.abs(got_betas - betas).max() <= 1e-12 * betas.max()      # no row took another path through the search
    return got


def test_affinities_of_the_fixture(g11):
    d2 = g11["d2"].astype(np.float64)
    got = _check_affinities(d2, float(g11["perplexity"]), g11["P"], "g11")
    again, _ = _affinities(d2, float(g11["perplexity"]), ldd=65, ldp=65, want_betas=False)      # dense, no betas: the same bits
    assert np.array_equal(again, got)


# seeds at which every row's stop margin exceeds 1e-9 (checked on the CPU with tests/tsne_ref.py; the test asserts it again)
AFFINITY_SEEDS = {(n, p): 0 for n in (3, 64, 65, 255, 256, 257, 513) for p in (2.0, 5.0, 30.0) if p < n}
AFFINITY_SEEDS.update({(255, 2.0): 1, (255, 5.0): 2, (513, 2.0): 1, (513, 30.0): 3})


@pytest.mark.parametrize("n,perplexity", sorted(AFFINITY_SEEDS))
def test_affinities_equal_the_restatement(n, perplexity):
    x, _ = tsne_ref.planted(4, n // 4 + 1, 8, seed=AFFINITY_SEEDS[n, perplexity], spread=2.0)
    _check_affinities(tsne_ref.sqdist(x[:n]), perplexity, what=f"n={n} perplexity={perplexity}")


@pytest.mark.parametrize("n", [64, 257])
def test_affinities_with_duplicate_points_and_a_far_outlier(n):
    """Duplicates: zero distances off the diagonal (exp(-0 beta) = 1 whatever beta).  The outlier: every exp underflows to 0 at
    beta = 1, so its row sum takes the (double)1e-8f floor and the search halves beta from there."""
    x, _ = tsne_ref.planted(4, n // 4 + 1, 8, seed=5, spread=2.0)
    x = x[:n].astype(np.float64)
    x[1] = x[0]
    x[7] = x[0]
    x[n - 1] = 300.0
    d2 = tsne_ref.sqdist(x)
    assert d2[0, 1] == 0.0 and d2[1, 7] == 0.0 and np.exp(-d2[n - 1, :n - 1]).max() == 0.0
    _check_affinities(d2, 5.0, what=f"duplicates and an outlier, n={n}")


# ---------------------------------------------------------------- one gradient

def _steps(P, Y, update, gains, n_steps, exaggeration, momentum, lr, min_gain=0.01, ldp=None, p_offset=0, ldy=2, ws_fill=NAN,
           want_kl=True, want_norm=True):
    """xvec_tsne_steps on copies of the host arrays; returns (Y, update, gains, kl, norm) as numpy."""
    from xvector_amd import hip
    n = Y.shape[0]
    ldp = n if ldp is None else ldp
    _, pv = _padded(P, ldp, offset=p_offset)
    bufs = [_padded(a, ldy)[1] for a in (Y, update, gains)]
    rep = torch.full((4,), SENTINEL, dtype=torch.float64, device=DEV)
    ws = _Workspace(n, 0, ws_fill)
    _check(hip.lib.xvec_tsne_steps(pv.data_ptr(), ldp, n, 2, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), ldy,
                                   int(n_steps), float(exaggeration), float(momentum), float(lr), float(min_gain),
                                   rep.data_ptr() if want_kl else None, rep.data_ptr() + 8 if want_norm else None, ws.ptr, ws.bytes,
                                   _stream()))
    ws.check()
    r = rep.cpu().numpy()
    assert r[2] == SENTINEL and r[3] == SENTINEL and (want_kl or r[0] == SENTINEL) and (want_norm or r[1] == SENTINEL)
    return tuple(b.cpu().numpy().copy() for b in bufs) + (float(r[0]), float(r[1]))


def _gradient(P, Y, exaggeration, **kw):
    """(grad, kl, norm) from one iteration that starts at a zero update and unit gains with learning_rate = 1.25: the gains
    become 0.8 everywhere (0 * grad < 0 is false), so update = -1.25 (0.8 grad) = -grad to two roundings."""
    _, update, gains, kl, norm = _steps(P, Y, np.zeros_like(Y), np.ones_like(Y), 1, exaggeration, 0.5, 1.25, **kw)
    assert (gains == 0.8).all()
    return -update, kl, norm


def test_gradient_norm_and_kl_of_the_fixture(g11):
    grad, kl, norm = _gradient(g11["P"], g11["y_grad"], 1.0)
    top = np.abs(g11["grad"]).max()
    assert np.abs(grad - g11["grad"]).max() <= 1e-12 * top
    assert abs(norm - np.sqrt((g11["grad"] ** 2).sum())) <= 1e-12 * np.sqrt((g11["grad"] ** 2).sum())
    assert abs(kl - float(g11["kl"])) <= 1e-12 * abs(float(g11["kl"]))


def _reference_sums(P, Y, chunk=512):
    """(attraction at exaggeration 1, repulsion numerator, Z) in float64, a block of rows at a time."""
    n = Y.shape[0]
    A, R, Z = np.zeros((n, 2)), np.zeros((n, 2)), 0.0
    for r0 in range(0, n, chunk):
        diff = Y[r0:r0 + chunk, None, :] - Y[None, :, :]
        w = 1.0 / (1.0 + (diff ** 2).sum(-1))
        w[np.arange(w.shape[0]), r0 + np.arange(w.shape[0])] = 0.0
        Z += w.sum()
        A[r0:r0 + chunk] = ((P[r0:r0 + chunk] * w)[:, :, None] * diff).sum(1)
        R[r0:r0 + chunk] = ((w * w)[:, :, None] * diff).sum(1)
    return A, R, Z


GRADIENT_SIZES = (2, 3, 4, 5, 7, 8, 9, 17, 127, 128, 129, 255, 256, 257, 385, 2047, 2049, 4097)


def test_gradient_sizes_meet_every_edge_of_the_devices_plan():
    """GRADIENT_SIZES end a row group and a column slice of the device's own plan one short, exactly and one past."""
    from xvector_amd import visualize
    seen = set()
    for n in GRADIENT_SIZES:
        rows, slices, cols = visualize.tsne_plan(n)
        last = n - (slices - 1) * cols
        print(f"gradient n={n}: rows {rows}, {slices} slices of {cols} columns (the last {last})")
        seen |= {("row", n % rows == 0), ("row+1", n % rows == 1), ("row-1", n % rows == rows - 1), ("slices", slices > 1),
                 ("last slice 1", last == 1 and slices > 1), ("last slice full", last == cols), ("last slice -1", last == cols - 1),
                 ("rows", rows)}
    for edge in ("row", "row+1", "row-1", "slices", "last slice 1", "last slice full", "last slice -1"):
        assert (edge, True) in seen, f"no size met the edge {edge!r} on this device's plan"
    print("rows per block met:", sorted(v for k, v in seen if k == "rows"))


@pytest.mark.parametrize("n", GRADIENT_SIZES)
def test_gradient_on_both_sides_of_every_plan_boundary(n):
    rng = np.random.default_rng(n)
    Y = rng.standard_normal((n, 2))
    P = rng.random((n, n))
    P = P + P.T
    np.fill_diagonal(P, 0.0)
    P /= P.sum()
    small = n <= 513                                  # the KL value and the distance from the floor: where the dense forms fit
    assert not small or tsne_ref.smallest_q(Y) > 1e3 * EPS
    A, R, Z = _reference_sums(P, Y)
    for exaggeration in (1.0, 12.0):
        want = 4.0 * (exaggeration * A - R / Z)
        # an odd stride and a base 8 bytes off a 16-byte boundary take the 8-byte loads of P, the dense call the 16-byte ones
        for kw in (dict(), dict(ldp=n + 3, p_offset=1, ldy=5)):
            grad, kl, norm = _gradient(P, Y, exaggeration, want_kl=small, **kw)
            assert np.abs(grad - want).max() <= 1e-12 * np.abs(want).max(), (exaggeration, kw)
            assert abs(norm - np.sqrt((want ** 2).sum())) <= 1e-12 * np.sqrt((want ** 2).sum()), (exaggeration, kw)
            if small:
                want_kl = tsne_ref.kl_gradient(P, Y, exaggeration)[0]
                assert abs(kl - want_kl) <= 1e-12 * abs(want_kl), (exaggeration, kw)


# ---------------------------------------------------------------- trajectories

def test_both_fixture_trajectories_and_step_10_is_ten_steps(g11):
    g = g11
    lr = float(g["learning_rate"])
    for start, end, kl_end, ex, mom in ((g["y0"], g["y1"], g["kl1"], float(g["exaggeration"]), 0.5), (g["y1"], g["y2"], g["kl2"], 1.0, 0.8)):
        zeros, ones = np.zeros_like(start), np.ones_like(start)
        Y, update, gains, kl, norm = _steps(g["P"], start, zeros, ones, 10, ex, mom, lr)
        assert np.abs(Y - end).max() <= 1e-9 * np.abs(end).max()
        assert abs(kl - float(kl_end)) <= 1e-9 * abs(float(kl_end))
        state = (start, zeros, ones)
        for _ in range(10):
            *state, kl1, norm1 = _steps(g["P"], *state, 1, ex, mom, lr)
        assert all(np.array_equal(a, b) for a, b in zip(state, (Y, update, gains))) and (kl1, norm1) == (kl, norm)


# ---------------------------------------------------------------- determinism and hygiene

def test_bit_identical_whatever_the_workspace_and_the_strides(g11):
    g = g11
    args = (g["P"], g["y0"], np.zeros_like(g["y0"]), np.ones_like(g["y0"]), 7, 12.0, 0.5, 50.0)
    base = _steps(*args)
    for kw in (dict(), dict(ws_fill=1e300), dict(ws_fill=0.0), dict(ldp=70, ldy=3), dict(ldp=67, p_offset=1, ldy=7),
               dict(want_kl=False), dict(want_norm=False)):
        got = _steps(*args, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], base[:3])), kw
        assert (not kw.get("want_kl", True) or got[3] == base[3]) and (not kw.get("want_norm", True) or got[4] == base[4]), kw
    d2 = g["d2"].astype(np.float64)
    p0, b0 = _affinities(d2, 5.0)
    p1, b1 = _affinities(d2, 5.0, ldd=80, ldp=65)
    assert np.array_equal(p0, p1) and np.array_equal(b0, b1)


def test_two_handles_on_two_threads_work_independently(g11):
    from xvector_amd import visualize
    P = _dev(g11["P"])
    want = []
    for seed in (1, 2):
        t = visualize.Tsne(P=P, init="random", seed=seed, device=DEV)
        t.step(20)
        want.append(t.Y.cpu().numpy())
    got, errors = [None, None], []

    def work(k):
        try:
            with torch.cuda.stream(torch.cuda.Stream(DEV)):
                t = visualize.Tsne(P=P, init="random", seed=k + 1, device=DEV)
                for _ in range(20):
                    t.step(1)
                got[k] = t.Y.cpu().numpy()
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and not np.array_equal(got[0], got[1])


def test_step_follows_the_schedule_across_iteration_250(g11):
    """Tsne.step without exaggeration and momentum: 12 / 0.5 before iteration 250, then 1 / 0.8 from a zero update and unit
    gains; a count that crosses 250 is split there, bit for bit."""
    from xvector_amd import visualize
    P = _dev(g11["P"])

    def fresh():
        return visualize.Tsne(P=P, init=g11["y0"], device=DEV)

    a, b, c = fresh(), fresh(), fresh()
    a.step(260)
    b.step(250)
    b.step(10)
    c.step(250, 12.0, 0.5, fresh=True)
    c.step(10, 1.0, 0.8, fresh=True)
    assert a.n_iter == b.n_iter == c.n_iter == 260
    for other in (b, c):
        for name in ("Y", "update", "gains"):
            assert torch.equal(getattr(a, name), getattr(other, name)), name
    d = fresh()
    d.step(250)
    d.step(10, 1.0, 0.8)                                      # without the fresh start the second stage is another run
    assert not torch.equal(d.Y, a.Y)
    with pytest.raises(ValueError, match="both exaggeration and momentum"):
        d.step(1, exaggeration=2.0)


# ---------------------------------------------------------------- end to end

# The restatement's five runs below span 3.0e-5 of KL; forty-five of its runs from such starts (two float64 forms of its sums
# among them) span 8.3e-5: profiles/tsne_errors.txt.  The margin above `hi` is the wider of the two, from that record of the
# restatement alone -- no device figure enters it.
RECORDED_KL_WIDTH = 8.3e-5


@pytest.fixture(scope="module")
def planted_runs():
    """Planted speakers (8 x 25 points, D = 64) and the restatement's own 1000 iterations from five starts that differ by
    1e-13 relative noise: the spread any faithful implementation shows."""
    x, labels = tsne_ref.planted(8, 25, 64, seed=0)
    n = x.shape[0]
    g = torch.Generator(device="cpu").manual_seed(0)
    y0 = (1e-4 * torch.randn((n, 2), generator=g, dtype=torch.float64)).numpy()
    P = tsne_ref.joint_probabilities(tsne_ref.sqdist(x), 30.0)
    rng = np.random.default_rng(7)
    runs = []
    for k in range(5):
        start = y0 if k == 0 else y0 * (1.0 + 1e-13 * rng.standard_normal(y0.shape))
        y, kl, it = tsne_ref.run(P, start)
        runs.append((kl, tsne_ref.trustworthiness(x, y, 5), tsne_ref.nn_accuracy(y, labels), it))
    return x, labels, runs


def test_whole_run_on_planted_speakers_matches_the_restatement_by_quality(planted_runs):
    from xvector_amd import visualize
    x, labels, runs = planted_runs
    lo, hi = min(r[0] for r in runs), max(r[0] for r in runs)
    trust = min(r[1] for r in runs)
    assert all(r[2] == 1.0 and r[3] == 999 for r in runs)
    t = visualize.Tsne(x, perplexity=30.0, init="random", seed=0, device=DEV)
    y = t.run().cpu().numpy()
    got_trust, got_acc = tsne_ref.trustworthiness(x, y, 5), tsne_ref.nn_accuracy(y, labels)
    print(f"planted 8 x 25, D = 64: restatement KL {lo:.6f} .. {hi:.6f}, trustworthiness >= {trust:.6f}; "
          f"device KL {t.kl_divergence_:.6f}, trustworthiness {got_trust:.6f}, 1-NN accuracy {got_acc:.3f}, n_iter_ {t.n_iter_}")
    assert t.n_iter_ == 999 and t.n_iter == 1000 and t.embedding_ is t.Y
    assert t.kl_divergence_ <= hi + max(hi - lo, RECORDED_KL_WIDTH)
    assert got_trust >= trust - 0.01
    assert got_acc == 1.0
    # the KL value the run reports is the restatement's for the embedding that entered the last iteration ... which is gone;
    # one more reported iteration from the end state is checked instead
    kl, _ = t.step(1, report=True)
    P = tsne_ref.joint_probabilities(tsne_ref.sqdist(x), 30.0)
    assert abs(kl - tsne_ref.kl_gradient(P, y)[0]) <= 1e-9 * kl


# ---------------------------------------------------------------- PCA

def _pca_data(n, d, seed, constant=None):
    rng = np.random.default_rng(seed)
    basis = np.linalg.qr(rng.standard_normal((d, d)))[0]
    scales = np.array([6.0, 3.0] + [1.0] * (d - 2))[:d]
    x = (rng.standard_normal((n, d)) * scales) @ basis.T + rng.standard_normal(d)
    if constant is not None:
        x[:, constant] = 0.7
    return x


def _check_pca(x, standardize, want=None):
    from xvector_amd import visualize
    z, lam = tsne_ref.pca(x, 2, standardize)
    top = [lam[k] - lam[k + 1] for k in range(min(2, len(lam) - 1))]
    assert min(top) > 0.05 * lam[0], "the leading eigenvalues must be separated for the components to be comparable"
    got = visualize.pca_map(x, 2, standardize, device=DEV)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (x.shape[0], 2)
    want = z if want is None else want
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-9 * np.abs(want).max()


def test_pca_map_of_the_fixture(g11):
    _check_pca(g11["x_pca"], True, g11["pca"])


@pytest.mark.parametrize("n,d", [(3, 2), (65, 512), (200, 64)])
def test_pca_map_equals_the_restatement(n, d):
    """At D = 2 the standardised scatter is [[n, r], [r, n]]: its eigenvectors are (1, 1) and (1, -1) / sqrt 2 whatever the data,
    the second has two entries of EQUAL magnitude, and the sign rule (the larger one positive) is decided by rounding alone,
    in scikit-learn as here.  That case is compared without standardising; the others both ways, one with a constant column."""
    x = _pca_data(n, d, seed=n + d, constant=5 if d > 8 else None)
    for standardize in ((False,) if d == 2 else (True, False)):
        _check_pca(x, standardize)
    if d == 64:
        _check_pca(x.astype(np.float32), True)


# ---------------------------------------------------------------- scatter_maps

def test_scatter_maps_returns_the_three_maps_on_the_device(planted_runs):
    import xvector_amd as xa
    x, labels, _ = planted_runs
    maps = xa.scatter_maps(x, labels, perplexity=30.0, device=DEV, init="random", seed=0, max_iter=250)
    assert sorted(maps) == ["LDA", "PCA", "TSNE"]
    for name, m in maps.items():
        assert m.is_cuda and m.dtype == torch.float64 and tuple(m.shape) == (x.shape[0], 2) and torch.isfinite(m).all(), name
    want = xa.lda(xa.plda.get_x_vec_stat(x, labels), 2, device=DEV).stat1
    assert np.array_equal(maps["LDA"].cpu().numpy(), np.asarray(want))
    assert np.abs(maps["PCA"].cpu().numpy() - tsne_ref.pca(x)[0]).max() <= 1e-9 * np.abs(tsne_ref.pca(x)[0]).max()
    assert tsne_ref.nn_accuracy(maps["TSNE"].cpu().numpy(), labels) == 1.0
