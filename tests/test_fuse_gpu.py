"""Score fusion on the device (csrc/fuse.hip through xvector_amd.fuse) against the numpy restatement tests/fuse_ref.py, at the
kernels' edges: the 2048-trial round of a block, the second round of every block, the tile of the apply.  Every workspace of a
fit that is held to bounds is a window of exactly the queried size inside a guarded buffer (score_support.window), filled with
garbage first; the guards are checked after the call.

Bounds (all derived, none fitted to what the device gives; eps = 2^-53): fuse_ref.fit_bounds with
c = depth(n) + XVEC_FUSE_TERM_ULPS(K) of include/xvec_fuse.h, n the trials launched (left-out trials keep their places)."""
import numpy as np
import pytest
import torch

import calib_ref
import fuse_ref as fr
import score_support as ss
from calib_ref import EPS, LN2
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROUND = fr.B * fr.ITEMS
MAX_ITER = fr.GPU_MAX_ITER


class Window:
    """A workspace of exactly the size n trials of k terms need, inside guards, filled with `fill`."""

    def __init__(self, n, k, fill):
        from xvector_amd import hip
        self.need = hip.lib.xvec_fuse_workspace_bytes(n, k)
        assert self.need > 0
        self.big, self.off = ss.window(self.need, DEV)
        self.ws = self.big[self.off:self.off + self.need]
        if isinstance(fill, int):
            self.ws.fill_(fill)
        else:
            self.ws.copy_(torch.randint(0, 256, (self.need,), dtype=torch.uint8, generator=fill).to(DEV))

    def intact(self):
        torch.cuda.synchronize()
        return ss.guards_intact(self.big, self.off, self.need)


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _terms(terms):
    """The restatement's (kind, array) terms as device Terms."""
    from xvector_amd import fuse
    make = {fr.MATRIX: fuse.matrix, fr.ROW: fuse.row_quality, fr.COL: fuse.col_quality}
    return [make[kind](_dev(a)) for kind, a in terms]


def _vector_terms(F):
    """K rows of values over n trials as terms of the plain-vector form: [1, n] matrices."""
    from xvector_amd import fuse
    return [fuse.matrix(_dev(row)) for row in F]


def _check(got, F, tgt, p, l2, n_launched, what, n_nan=0, n_bad=0):
    """The device result against the restatement of the trials kept (F [K, kept]).  Returns the restatement."""
    K = len(F)
    ref = fr.fit(F, tgt, p, l2)
    assert (got.n_target, got.n_nontarget, got.n_nan, got.n_bad_index) == (int(tgt.sum()), int((~tgt).sum()), n_nan, n_bad), what
    assert got.constant_terms == np.nonzero(ref["constant"])[0].tolist(), what
    if not ref["converged"]:                   # no minimum: the device must say so too, with finite numbers
        assert got.status == 1 and np.isfinite(got.weights + [got.bias, got.objective_bits]).all(), (what, got)
        return ref
    bw, bb, bj, bp = fr.fit_bounds(ref, fr.sum_constant(n_launched, K))
    dw = np.abs(np.array(got.weights) - ref["w"].astype(np.float64))
    db = abs(got.bias - float(ref["b"]))
    dj = abs(got.objective_bits - float(ref["J_data"] / LN2))
    dp = abs(got.penalty_bits - float(ref["penalty"] / LN2))
    print(f"{what}: status {got.status} after {got.n_iter} passes (restatement {ref['passes']}); max |w - ref| / bound "
          f"{(dw / np.maximum(bw, 1e-300)).max():.3e} (|w - ref| {dw.max():.3e}), |b - ref| {db:.3e} (bound {bb:.3e}), "
          f"|objective - ref| {dj:.3e} (bound {bj:.3e}), |penalty - ref| {dp:.3e} (bound {bp:.3e})")
    assert got.status == 0 and got.n_iter < MAX_ITER, (what, got)
    assert (dw <= bw).all() and db <= bb and dj <= bj and dp <= bp, what
    for k in np.nonzero(ref["constant"])[0]:
        assert got.weights[k] == 0.0 and not np.signbit(got.weights[k]), what
    return ref


# ---------------------------------------------------------------- planted cases

@pytest.fixture(scope="module")
def pl():
    p = fr.planted()
    p["trials"] = fr.upper_triangle(p["n"], p["labels"])
    return p


@pytest.mark.parametrize("k,p_target", fr.PLANTED_CASES)
def test_planted_cases(pl, k, p_target):
    from xvector_amd import fuse, TrialList
    r, c, t = pl["trials"]
    assert len(r) == 2556
    terms = fr.planted_terms(pl, k)
    F, tgt, n_nan, n_bad = fr.select_trials(terms, pl["n"], pl["n"], r, c, t)
    w = Window(len(r), k, 0xFF)
    got = fuse.fit_fusion(_terms(terms), TrialList(r, c, t), p_target, max_iter=MAX_ITER, workspace=w.ws).result()
    assert w.intact()
    _check(got, F, tgt, p_target, 0.0, len(r), f"planted, K = {k}, p_target {p_target}")
    assert len(got.weights) == k and got.constant_terms == []


def test_one_term_is_calibration():
    """K = 1, one MATRIX term, no ridge: the fit of xvec_calib_fit on the same inputs.  Both lie inside the restatements' bounds
    (bit equality is not promised: the 2 x 2 closed form and the Cholesky solve round differently)."""
    from xvector_amd import calibrate as cal, fuse
    g = load_golden("g12_calib.npz")
    s, tgt = g["scores"], g["is_target"].astype(bool)
    assert fr.term_ulps(1) == cal.TERM_ULPS
    for p in (0.5, 0.01):
        f = fuse.fit_fusion([fuse.matrix(_dev(s))], _dev(tgt, torch.uint8), p).result()
        c = cal.fit_calibration(_dev(s), _dev(tgt, torch.uint8), p).result()
        ref = _check(f, s[None, :], tgt, p, 0.0, len(s), f"K = 1 at p_target {p}")
        cref = calib_ref.fit(s, tgt, p)
        ba, bb, bj = calib_ref.fit_bounds(cref, fr.sum_constant(len(s), 1))
        for name, a, b, j in (("fuse", f.weights[0], f.bias, f.objective_bits), ("calib", c.a, c.b, c.objective_bits)):
            assert abs(a - float(cref["a"])) <= ba and abs(b - float(cref["b"])) <= bb, name
            assert abs(j - float(cref["J"] / LN2)) <= bj, name
        assert abs(float(ref["w"][0] - cref["a"])) <= ba and f.status == c.status == fuse.CONVERGED


# ---------------------------------------------------------------- tile and block edges

@pytest.mark.parametrize("n", fr.VECTOR_SIZES)
def test_vector_form_at_the_block_tile(n):
    """The plain-vector form: two [1, n] matrices, a COL term and a ROW term (one row: constant, weight 0)."""
    from xvector_amd import fuse
    F, tgt = fr.vector_case(n)
    buf = _dev(np.r_[0.0, F[0], 0.0])                                          # a base 8 bytes off 16
    terms = [fuse.matrix(buf[1:n + 1]), fuse.matrix(_dev(F[1])), fuse.col_quality(_dev(F[2])), fuse.row_quality(_dev(F[3, :1]))]
    w = Window(n, 4, 0xA5)
    got = fuse.fit_fusion(terms, _dev(tgt, torch.uint8), 0.5, max_iter=MAX_ITER, workspace=w.ws).result()
    assert w.intact()
    _check(got, F, tgt, 0.5, 0.0, n, f"vector form, n = {n}")
    assert got.constant_terms == [3] and got.weights[3] == 0.0
    if n == 2:
        assert got.status == 1                 # one target and one non-target are separable: no minimum


def test_every_block_takes_a_second_round():
    """One n above XVEC_CALIB_MAX_BLOCKS * 2048: the grid is capped and every block walks on."""
    from xvector_amd import fuse
    n = fr.BIG_N
    assert n > fr.MAX_BLOCKS * ROUND
    F, tgt = fr.big_case()
    got = fuse.fit_fusion(_vector_terms(F), _dev(tgt, torch.uint8), 0.5, max_iter=MAX_ITER).result()
    _check(got, F, tgt, 0.5, 0.0, n, f"vector form, n = {n}")


def _index_case(poison):
    """fuse_ref.index_case in buffers of their own: the first MATRIX term under a row stride of 37, each term with cells of
    `poison` around it and in the padding of its rows, where the trials with a bad index point."""
    from xvector_amd import fuse
    ic = fr.index_case()
    (_, m0), (_, m1), (_, rq), (_, cq) = host = ic["terms"]
    rows, cols, ld, row, col, tgt = ic["rows"], ic["cols"], 37, ic["row"], ic["col"], ic["tgt"]

    def matrix_buffer(m, stride):
        buf = np.full((rows + 8, stride), poison)
        buf[2:2 + rows, :cols] = m
        return _dev(buf)[2:2 + rows, :cols]

    def vector_buffer(v):
        buf = np.full(len(v) + 16, poison)
        buf[8:8 + len(v)] = v
        return _dev(buf)[8:8 + len(v)]
    terms = [fuse.matrix(matrix_buffer(m0, ld)), fuse.matrix(matrix_buffer(m1, cols + 1)), fuse.row_quality(vector_buffer(rq)),
             fuse.col_quality(vector_buffer(cq))]
    assert terms[0].data.stride(0) == ld
    return terms, host, rows, cols, row, col, tgt


def test_index_form_with_stride_nan_cells_and_bad_indices():
    from xvector_amd import fuse, TrialList
    records = []
    for poison in (np.nan, 1e300):
        terms, host, rows, cols, row, col, tgt = _index_case(poison)
        F, t, n_nan, n_bad = fr.select_trials(host, rows, cols, row, col, tgt)
        assert n_nan > 3 and n_bad > 10
        w = Window(len(tgt), 4, 0x5A)
        fus = fuse.fit_fusion(terms, TrialList(row, col, tgt), 0.5, max_iter=MAX_ITER, workspace=w.ws)
        assert w.intact()
        records.append(fus.record.cpu().numpy().tobytes())
        _check(fus.result(), F, t, 0.5, 0.0, len(tgt), f"index form, poison {poison}", n_nan, n_bad)
    assert records[0] == records[1]            # no cell of a bad trial was read: the poison moved nothing


@pytest.mark.parametrize("shape", fr.ALL_PAIRS_SHAPES)
def test_all_pairs_form(shape):
    """A non-square matrix with ROW and COL terms; a square one with skip_diagonal."""
    from xvector_amd import fuse
    rows, cols = shape
    host, rc, cc, skip = fr.all_pairs_case(shape)
    F, t, n_nan, _ = fr.select_all_pairs(host, rows, cols, rc, cc, skip)
    w = Window(rows * cols, 4, 0xFF)
    got = fuse.fit_fusion_all_pairs(_terms(host), rc, None if skip else cc, skip_diagonal=skip, max_iter=MAX_ITER,
                                    workspace=w.ws).result()
    assert w.intact()
    _check(got, F, t, 0.5, 0.0, rows * cols, f"all pairs {shape}", n_nan, 0)
    assert got.n_target + got.n_nontarget + got.n_nan == rows * cols - (rows if skip else 0)


# ---------------------------------------------------------------- status paths

def test_one_class_and_an_infinity_in_the_second_term():
    from xvector_amd import fuse
    F, tgt = fr.draw(np.random.default_rng(7), 300, 2)
    r = fuse.fit_fusion(_vector_terms(F), _dev(np.ones(300), torch.uint8)).result()
    assert r.status == fuse.ONE_CLASS and (r.n_target, r.n_nontarget) == (300, 0)
    assert np.isnan(r.weights + [r.bias, r.objective_bits, r.penalty_bits]).all() and len(r.weights) == 2
    F_inf = F.copy()
    F_inf[1, 17] = -np.inf
    r = fuse.fit_fusion(_vector_terms(F_inf), _dev(tgt, torch.uint8)).result()
    assert r.status == fuse.INF_SCORE and np.isnan(r.weights + [r.bias, r.objective_bits]).all()
    assert (r.n_target, r.n_nontarget, r.n_nan) == (int(tgt.sum()), int((~tgt).sum()), 0)


def test_a_constant_term_has_weight_zero_and_moves_nothing():
    from xvector_amd import fuse
    F, tgt, value = fr.constant_case()
    flags = _dev(tgt, torch.uint8)
    plain = fuse.fit_fusion(_vector_terms(F), flags).result()
    for at in (0, 1, 2):                       # in front, between, behind
        Fc = np.insert(F, at, np.full(700, value), axis=0)
        got = fuse.fit_fusion(_vector_terms(Fc), flags).result()
        _check(got, Fc, tgt, 0.5, 0.0, 700, f"constant term at {at}")
        assert got.constant_terms == [at] and got.weights[at] == 0.0
        others = [w for k, w in enumerate(got.weights) if k != at]
        assert np.array(others).tobytes() == np.array(plain.weights).tobytes()                     # bit for bit
        assert (got.bias, got.objective_bits, got.n_iter) == (plain.bias, plain.objective_bits, plain.n_iter)


def test_two_identical_terms():
    from xvector_amd import fuse
    F, tgt = fr.identical_case()
    F1 = F[:1]
    flags = _dev(tgt, torch.uint8)
    got = fuse.fit_fusion(_vector_terms(F), flags, l2=1e-3).result()
    _check(got, F, tgt, 0.5, 1e-3, 500, "identical terms, l2 = 1e-3")
    print(f"identical terms, l2 = 1e-3: weights {got.weights[0]!r} and {got.weights[1]!r}")
    assert got.weights[0] == got.weights[1]                                    # bit for bit
    # without a ridge the Hessian is singular: the damping rule carries the iteration; only the sum is defined
    got = fuse.fit_fusion(_vector_terms(F), flags, l2=0.0, max_iter=MAX_ITER).result()
    one = fr.fit(F1, tgt, 0.5)
    bw, bb, bj, _ = fr.fit_bounds(one, fr.sum_constant(500, 2))
    total = got.weights[0] + got.weights[1]
    print(f"identical terms, l2 = 0: status {got.status} after {got.n_iter} passes; |w0 + w1 - ref| "
          f"{abs(total - float(one['w'][0])):.3e} (bound {bw[0] + 2 * EPS * abs(total):.3e})")
    assert got.status == fuse.CONVERGED and got.constant_terms == []
    assert abs(total - float(one["w"][0])) <= bw[0] + 2 * EPS * abs(total)       # (the sum's own rounding)
    assert abs(got.bias - float(one["b"])) <= bb and abs(got.objective_bits - float(one["J_data"] / LN2)) <= bj


def test_a_separable_set_with_and_without_a_ridge_and_one_pass():
    from xvector_amd import fuse
    F, tgt = fr.separable_set()
    flags = _dev(tgt, torch.uint8)
    r = fuse.fit_fusion(_vector_terms(F), flags, max_iter=MAX_ITER).result()
    assert not fr.fit(F, tgt, 0.5)["converged"]
    assert r.status == fuse.MAX_ITER_REACHED and r.n_iter <= MAX_ITER and r.weights[0] > 0
    assert np.isfinite(r.weights + [r.bias, r.objective_bits, r.penalty_bits]).all()
    r = fuse.fit_fusion(_vector_terms(F), flags, l2=1e-3, max_iter=MAX_ITER).result()
    ref = _check(r, F, tgt, 0.5, 1e-3, len(tgt), "separable set, l2 = 1e-3")
    assert ref["converged"] and r.penalty_bits > 0
    r = fuse.fit_fusion(_vector_terms(F), flags, max_iter=1).result()            # one pass cannot converge
    assert r.status == fuse.MAX_ITER_REACHED and r.n_iter == 1 and np.isfinite(r.weights + [r.bias]).all()


# ---------------------------------------------------------------- bit identity

def test_results_are_bit_identical_whatever_the_workspace_held(pl):
    from xvector_amd import fuse, TrialList
    r, c, t = pl["trials"]
    terms, trials = _terms(fr.planted_terms(pl, 4)), TrialList(r, c, t)
    gen = torch.Generator().manual_seed(5)
    records = []
    for fill in (0x00, 0xFF, gen):             # zeros, NaN, random; each a window of exactly the reported size
        w = Window(len(r), 4, fill)
        records.append(fuse.fit_fusion(terms, trials, 0.01, l2=1e-4, workspace=w.ws).record.cpu().numpy().tobytes())
        assert w.intact()
    records.append(fuse.fit_fusion(terms, trials, 0.01, l2=1e-4).record.cpu().numpy().tobytes())
    assert records[0] == records[1] == records[2] == records[3]


# ---------------------------------------------------------------- apply

def _record(weights, bias, k):
    from xvector_amd import fuse
    r = fuse._Fit(b=bias, objective_bits=0.0, penalty_bits=0.0, n_target=1, n_nontarget=1, n_nan=0, n_bad_index=0, n_terms=k,
                  n_iter=1, status=0, constant_mask=0)
    for q, w in enumerate(weights):
        r.w[q] = w
    return fuse.Fusion(torch.from_numpy(np.frombuffer(bytes(r), dtype=np.float64).copy()).to(DEV), k)


W = [0.04268166328079601, -1.7320508075688772, 0.3333333333333333, 2.718281828459045, -0.1, 7.0e-3, 1.1, -3.3]
BIAS = 1.504446028184007


@pytest.mark.parametrize("shape", [(1, 1), (8, 256), (9, 257), (70, 300)])
def test_apply_is_numpys_expression_bit_for_bit(shape):
    from xvector_amd import fuse
    rows, cols = shape
    rng = np.random.default_rng(rows * 1000 + cols)
    h0, h1 = rng.normal(-40.0, 30.0, (rows, cols + 5)), rng.normal(0.0, 1.0, (rows, cols))
    rq, cq = rng.normal(5.0, 0.5, rows), rng.normal(6.0, 0.7, cols)
    d0 = _dev(h0)
    terms = [fuse.matrix(d0[:, :cols]), fuse.row_quality(_dev(rq)), fuse.matrix(_dev(h1)), fuse.col_quality(_dev(cq))]
    # the weights beyond K are not read: they hold NaN
    fus = _record(W[:4] + [np.nan] * 4, BIAS, 4)
    want = W[0] * h0[:, :cols] + W[1] * rq[:, None] + W[2] * h1 + W[3] * cq[None, :] + BIAS
    out = fus.apply(terms)                                                      # a strided input
    assert np.array_equal(out.cpu().numpy(), want)
    wide = torch.full((rows, cols + 3), 7.0, dtype=torch.float64, device=DEV)
    fus.apply(terms, out=wide[:, :cols])                                        # a strided output
    assert np.array_equal(wide.cpu().numpy()[:, :cols], want) and bool((wide[:, cols:] == 7.0).all())
    view = d0[:, :cols]
    assert fus.apply(terms, out=view) is view                                   # in place over the first MATRIX term
    assert np.array_equal(d0.cpu().numpy()[:, :cols], want) and np.array_equal(d0.cpu().numpy()[:, cols:], h0[:, cols:])
    # all eight terms, and one alone
    mats = [rng.normal(0.0, 3.0, (rows, cols)) for _ in range(8)]
    want8 = W[0] * mats[0]
    for q in range(1, 8):
        want8 = want8 + W[q] * mats[q]
    assert np.array_equal(_record(W, BIAS, 8).apply([fuse.matrix(_dev(m)) for m in mats]).cpu().numpy(), want8 + BIAS)
    assert np.array_equal(_record([W[1]] + [np.nan] * 7, BIAS, 1).apply([fuse.matrix(_dev(mats[0]))]).cpu().numpy(),
                          W[1] * mats[0] + BIAS)


def test_apply_keeps_symmetric_matrices_symmetric_and_refuses_overlap():
    from xvector_amd import fuse, hip
    rng = np.random.default_rng(1)
    a, b = rng.normal(-40.0, 30.0, (259, 259)), rng.normal(0.0, 1.0, (259, 259))
    a, b = a + a.T, b + b.T
    fus = _record(W[:2], BIAS, 2)
    da = _dev(a)
    out = fus.apply([fuse.matrix(da), fuse.matrix(_dev(b))]).cpu().numpy()
    assert np.array_equal(out, out.T) and np.array_equal(out, W[0] * a + W[1] * b + BIAS)
    # out may not be a ROW term's data, nor a MATRIX term's under another row stride
    buf = torch.zeros(259 * 259, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="overlaps term 1"):
        fus.apply([fuse.matrix(da), fuse.row_quality(buf[:259])], out=buf.view(259, 259))
    with pytest.raises(ValueError, match="overlaps term 0"):
        fus.apply([fuse.matrix(buf.view(259, 259)[:, :200]), fuse.matrix(da[:, :200])], out=torch.as_strided(buf, (259, 200), (200, 1)))
    terms = (fuse._Term * 2)()
    terms[0].data, terms[0].ld, terms[0].kind = buf.data_ptr(), 259, fuse.MATRIX
    terms[1].data, terms[1].ld, terms[1].kind = da.data_ptr(), 259, fuse.MATRIX
    assert hip.lib.xvec_fuse_apply(terms, 2, 259, 200, fus.record.data_ptr(), buf.data_ptr(), 200, None) == hip.ERR_ARG
    assert "in place (out is the data of term 0) needs ld_out == ld" in hip.lib.xvec_fuse_last_error().decode()


# ---------------------------------------------------------------- end to end

def test_plda_cosine_and_durations_fused_and_reported(synth):
    from xvector_amd import calibrate as cal, fuse, ScoreFuser, TrialList
    from xvector_amd.scoring import PldaScorer
    dim, n_spk, per = 24, 8, 6
    rng = np.random.default_rng(3)
    labels = np.repeat(np.arange(n_spk), per)
    dur = rng.integers(200, 1001, len(labels))                                  # the 200-1000 frame batches
    centres = rng.standard_normal((n_spk, dim))
    x = centres[labels] + (1.6 * np.sqrt(500.0 / dur))[:, None] * rng.standard_normal((len(labels), dim))      # short: noisy
    S = PldaScorer(*synth.make_plda(dim, n_spk, seed=3), device=DEV).score(x)
    u = _dev(x / np.linalg.norm(x, axis=1, keepdims=True))
    Cm = u @ u.T
    n = len(labels)
    ii, jj = np.nonzero(~np.eye(n, dtype=bool))
    trials = TrialList(ii, jj, labels[ii] == labels[jj])
    terms = [fuse.matrix(S), fuse.matrix(Cm), *fuse.log_duration_terms(dur, dur, device=DEV)]
    fuser = ScoreFuser().fit(terms, trials)
    fused = fuser.fuse(terms)
    got = fuser.result()
    host = [(fr.MATRIX, S.cpu().numpy()), (fr.MATRIX, Cm.cpu().numpy()), (fr.ROW, terms[2].data.cpu().numpy()),
            (fr.COL, terms[3].data.cpu().numpy())]
    F, tgt, _, _ = fr.select_trials(host, n, n, ii, jj, labels[ii] == labels[jj])
    ref = _check(got, F, tgt, 0.5, 0.0, len(ii), "PLDA + cosine + durations")
    c1 = fr.sum_constant(len(ii), 1)

    def report_tol(bound_j, k, size, cllr):
        """What a report's Cllr may differ by from the restatement's objective: the fit's bound; the 2 K + 1 roundings of a
        fused score of size `size` (softplus has slope <= 1); Cllr's own sum (depth + calibration's term constant) and the four
        roundings of its final quotients."""
        return bound_j + (2 * k + 1) * EPS * size / float(LN2) + (c1 + 4) * EPS * cllr
    rep = cal.calibration_report(fused, trials)
    size = float((np.abs(np.array(got.weights))[:, None] * np.abs(F)).sum(axis=0).max() + abs(got.bias))
    tol = report_tol(fr.fit_bounds(ref, fr.sum_constant(len(ii), 4))[2], 4, size, rep.cllr)
    print(f"fused: {got}; report {rep}; |cllr - restatement| {abs(rep.cllr - float(ref['J_data'] / LN2)):.3e} (tolerance {tol:.3e})")
    assert abs(rep.cllr - float(ref["J_data"] / LN2)) <= tol
    # a single system is the fusion with the other weights held at 0: the restatements' minima are ordered exactly, the
    # measured values as far as their tolerances allow
    singles = []
    for k in (0, 1):
        c = cal.ScoreCalibrator().fit(terms[k].data, trials)
        r1, one = c.result(), fr.fit(F[k:k + 1], tgt, 0.5)
        cllr1 = cal.calibration_report(c.calibrate(terms[k].data), trials).cllr
        assert float(ref["J_data"]) <= float(one["J_data"])
        singles.append((cllr1, report_tol(fr.fit_bounds(one, c1)[2], 1, float(np.abs(r1.a * F[k]).max() + abs(r1.b)), cllr1)))
    best, slack = min(singles)
    print(f"single systems, calibrated (Cllr, tolerance): {singles}")
    assert rep.cllr <= best + slack + tol and rep.cllr < best               # no worse; on this set it is better
    assert rep.min_cllr <= rep.cllr and (rep.n_target, rep.n_nontarget) == (int(tgt.sum()), int((~tgt).sum()))
    # fit_fusion is the same fit, Fusion.apply the same map
    again = fuse.fit_fusion(terms, trials)
    assert again.record.cpu().numpy().tobytes() == fuser.fusion.record.cpu().numpy().tobytes()
    assert torch.equal(again.apply(terms), fused)
