"""Score calibration on the device (csrc/calib.hip through xvector_amd.calibrate) against the numpy restatement
tests/calib_ref.py, at the kernels' edges: B = XVEC_CALIB_THREADS, a block's round of B * ITEMS trials, C = the hull chunk,
F = the groups the final block takes.  Every workspace is a window of exactly the queried size inside a guarded buffer
(score_support.window), filled with garbage first; the guards are checked after every call.

Bounds (all derived, none fitted to what the device gives; eps = 2^-53):
  fit      calib_ref.fit_bounds with c = depth(n) + TERM_ULPS of include/xvec_calib.h: 4 ||H^-1||_inf c eps sum |gradient terms|
           in the standardised coordinates, carried to a and b; objective_bits through the gradient.
  cllr     every term is positive, so sum |terms| is the value: c eps cllr, plus four roundings of the final quotients.
  minCllr  (ceil(S / B) + 9 + TERM_ULPS) eps sum |terms| for S segments, plus the roundings of the segment LLRs
           (8 eps (max |log(t / f)| + |log(P / N)|), each term's derivative against its LLR being below its weight)."""
import numpy as np
import pytest
import torch

import calib_ref
import eer_ref
import score_support as ss
from calib_ref import EPS
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, ITEMS, MAXB, ULPS, CH, F = 256, 8, 1024, 64, 16, 256
ROUND = B * ITEMS


def _consts_are_the_modules():
    from xvector_amd import calibrate as cal
    assert (cal.THREADS, cal.ITEMS, cal.MAX_BLOCKS, cal.TERM_ULPS, cal.HULL_CHUNK, cal.HULL_FINAL) == (B, ITEMS, MAXB, ULPS, CH, F)


def _c(n):
    blocks = min(-(-n // ROUND), MAXB)
    return -(-n // (blocks * B)) + 22 + ULPS


class Window:
    """A workspace of exactly the size n trials need, inside guards, filled with `fill`."""

    def __init__(self, n, fill):
        from xvector_amd import hip
        self.need = hip.lib.xvec_calib_workspace_bytes(n)
        assert self.need > 0
        self.big, self.off = ss.window(self.need, DEV)
        self.ws = self.big[self.off:self.off + self.need]
        self.ws.fill_(fill)

    def intact(self):
        torch.cuda.synchronize()
        return ss.guards_intact(self.big, self.off, self.need)


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


@pytest.fixture(scope="module")
def g12():
    g = load_golden("g12_calib.npz")
    s, tgt = g["scores"], g["is_target"].astype(bool)
    return s, tgt, {p: calib_ref.fit(s, tgt, p) for p in (0.5, 0.01)}


def _draw(rng, n, ties=False):
    """n overlapping scores on the PLDA-like scale, both classes present for n >= 2."""
    tgt = rng.random(n) < 0.35
    tgt[0], tgt[-1] = True, False
    s = np.where(tgt, rng.normal(-22.0, 24.0, n), rng.normal(-50.0, 27.0, n))
    if ties:
        s = np.round(s / 4) * 4
    return s, tgt


def _check_fit(got, s, tgt, p, n_launched, what, n_nan=0, n_bad=0):
    ref = calib_ref.fit(s, tgt, p)
    assert (got.n_target, got.n_nontarget, got.n_nan, got.n_bad_index) == (int(tgt.sum()), int((~tgt).sum()), n_nan, n_bad), what
    if not ref["converged"]:                   # no minimum (a separable set): the device must say so too, with finite numbers
        assert got.status == 1 and np.isfinite([got.a, got.b, got.objective_bits]).all(), (what, got)
        return None
    ba, bb, bj = calib_ref.fit_bounds(ref, _c(n_launched))
    da, db = abs(got.a - float(ref["a"])), abs(got.b - float(ref["b"]))
    dj = abs(got.objective_bits - float(ref["J"] / calib_ref.LN2))
    print(f"{what}: status {got.status} after {got.n_iter} passes; |a - ref| {da:.3e} (bound {ba:.3e}), |b - ref| {db:.3e} "
          f"(bound {bb:.3e}), |objective - ref| {dj:.3e} (bound {bj:.3e})")
    assert got.status == 0, (what, got)
    assert da <= ba and db <= bb and dj <= bj, what
    return ref


# ---------------------------------------------------------------- the fit

@pytest.mark.parametrize("p_target", [0.5, 0.01])
def test_fit_on_the_fixture(g12, p_target):
    from xvector_amd import calibrate as cal
    _consts_are_the_modules()
    s, tgt, refs = g12
    w = Window(len(s), 0xFF)
    got = cal.fit_calibration(_dev(s), _dev(tgt, torch.uint8), p_target, workspace=w.ws).result()
    assert w.intact()
    _check_fit(got, s, tgt, p_target, len(s), f"fixture at p_target {p_target}")
    assert abs(got.a - float(refs[p_target]["a"])) < 1e-9


SIZES = [2, B - 1, B, B + 1, ROUND - 1, ROUND + 1]


@pytest.mark.parametrize("n", SIZES)
def test_fit_vector_form(n):
    from xvector_amd import calibrate as cal
    rng = np.random.default_rng(100 + n)
    s, tgt = _draw(rng, n)
    buf = _dev(np.r_[0.0, s, 0.0])
    w = Window(n, 0xA5)
    got = cal.fit_calibration(buf[1:n + 1], _dev(tgt, torch.uint8), 0.5, workspace=w.ws).result()      # a base 8 bytes off 16
    assert w.intact()
    _check_fit(got, s, tgt, 0.5, n, f"vector form, n = {n}")
    if n == 2:
        assert got.status == 1                 # one target and one non-target are separable: no minimum


@pytest.mark.parametrize("n", SIZES)
def test_fit_index_form_with_stride_nan_cells_and_bad_indices(n):
    from xvector_amd import calibrate as cal, TrialList
    rng = np.random.default_rng(200 + n)
    rows, cols, ld = 13, 29, 37
    host = rng.normal(-40.0, 30.0, (rows, ld))
    host[rng.random((rows, ld)) < 0.03] = np.nan
    host[0, 0], host[1, 1] = -10.0, -60.0
    # the matrix stays as it is; the LIST makes the classes differ and overlap: a target trial draws its cell from the upper two
    # thirds of the values, a non-target trial from the lower two thirds
    order = np.argsort(np.nan_to_num(host[:, :cols], nan=-40.0).ravel())
    tgt = rng.random(n) < 0.4
    pick = np.where(tgt, rng.choice(order[len(order) // 3:], n), rng.choice(order[: 2 * len(order) // 3], n))
    row, col = pick // cols, pick % cols
    tgt[0], tgt[-1] = True, False
    row[0], col[0], row[-1], col[-1] = 0, 0, 1, 1
    if n > 2:
        bad = np.nonzero(rng.random(n) < 0.05)[0]
        bad = bad[(bad > 0) & (bad < n - 1)]
        row[bad[::2]] = rows + 3
        col[bad[1::2]] = -1
    buf = _dev(np.r_[0.0, host.ravel()])
    mat = buf[1:].view(rows, ld)[:, :cols]                                   # strided (ld = 37), base 8 bytes off 16
    s, t, n_nan, n_bad = calib_ref.select_trials(host[:, :cols], row, col, tgt)
    w = Window(n, 0x5A)
    got = cal.fit_calibration(mat, TrialList(row, col, tgt), 0.5, workspace=w.ws).result()
    assert w.intact()
    _check_fit(got, s, t, 0.5, n, f"index form, n = {n}", n_nan, n_bad)


@pytest.mark.parametrize("shape", [(1, 2), (1, B - 1), (1, B), (1, B + 1), (1, ROUND - 1), (1, ROUND + 1), (47, 47), (45, 46)])
def test_fit_all_pairs_form(shape):
    from xvector_amd import calibrate as cal
    rows, cols = shape
    rng = np.random.default_rng(300 + rows * cols)
    rc, cc = (np.zeros(1, int), (rng.random(cols) < 0.6).astype(int)) if rows == 1 else (rng.integers(0, 6, rows), None)
    if rows == 1:
        cc[0], cc[-1] = 0, 1
    elif rows != cols:
        cc = rng.integers(0, 6, cols)
    same = rc[:, None] == (rc if cc is None else cc)[None, :]
    host = np.where(same, rng.normal(-22.0, 24.0, shape), rng.normal(-50.0, 27.0, shape))
    skip = rows == cols
    if rows > 1:
        host[3, 5] = np.nan
    s, t, n_nan, _ = calib_ref.select_all_pairs(host, rc, rc if cc is None else cc, skip)
    w = Window(rows * cols, 0xFF)
    got = cal.fit_calibration_all_pairs(_dev(host), rc, cc, skip_diagonal=skip, p_target=0.5, workspace=w.ws).result()
    assert w.intact()
    _check_fit(got, s, t, 0.5, rows * cols, f"all pairs {shape}", n_nan, 0)


def test_fit_status_paths():
    from xvector_amd import calibrate as cal
    rng = np.random.default_rng(7)
    s, tgt = _draw(rng, 300)
    r = cal.fit_calibration(_dev(s), _dev(np.ones(300), torch.uint8)).result()                      # no non-target
    assert r.status == cal.ONE_CLASS and np.isnan([r.a, r.b, r.objective_bits]).all() and (r.n_target, r.n_nontarget) == (300, 0)
    s_inf = s.copy()
    s_inf[17] = np.inf
    r = cal.fit_calibration(_dev(s_inf), _dev(tgt, torch.uint8)).result()
    assert r.status == cal.INF_SCORE and np.isnan([r.a, r.b, r.objective_bits]).all()
    assert (r.n_target, r.n_nontarget) == (int(tgt.sum()), int((~tgt).sum()))
    sep = np.where(tgt, rng.uniform(1.0, 5.0, 300), rng.uniform(-5.0, -1.0, 300))                 # separable: no minimum
    for max_iter in (3, 40):
        r = cal.fit_calibration(_dev(sep), _dev(tgt, torch.uint8), max_iter=max_iter).result()
        assert r.status == cal.MAX_ITER_REACHED and np.isfinite([r.a, r.b, r.objective_bits]).all() and r.a > 0, r
        assert r.n_iter <= max_iter
    r = cal.fit_calibration(_dev(s), _dev(tgt, torch.uint8), max_iter=1).result()                  # one pass cannot converge
    assert r.status == cal.MAX_ITER_REACHED and r.n_iter == 1 and np.isfinite([r.a, r.b]).all()


def test_results_are_bit_identical_whatever_the_workspace_held(g12):
    from xvector_amd import calibrate as cal, TrialList
    s, tgt, _ = g12
    sd, td = _dev(s), _dev(tgt, torch.uint8)
    fits, cllrs, pavs = [], [], []
    for fill in (0x00, 0xFF, 0xA5):
        w = Window(len(s), fill)
        c = cal.fit_calibration(sd, td, 0.01, workspace=w.ws)
        fits.append(c.record.cpu().numpy().tobytes())
        r = cal.cllr(sd, td, workspace=w.ws)
        cllrs.append((np.float64(r.cllr).tobytes(), np.float64(r.act_dcf).tobytes()))
        p = cal.pav_segments(sd, td, workspace=w.ws)
        pavs.append((np.float64(p.min_cllr).tobytes(), p.k_end.tobytes(), p.tp_end.tobytes(), p.llr.tobytes(), p.score.tobytes()))
        assert w.intact()
    assert fits[0] == fits[1] == fits[2] and cllrs[0] == cllrs[1] == cllrs[2] and pavs[0] == pavs[1] == pavs[2]
    # and the three trial forms of one list agree bit for bit: the gathered trials are the same in the same order
    idx = TrialList(np.zeros(len(s), int), np.arange(len(s)), tgt)
    assert cal.fit_calibration(sd.reshape(1, -1), idx, 0.01).record.cpu().numpy().tobytes() == fits[0]


# ---------------------------------------------------------------- apply

def _record(a, b):
    from xvector_amd import calibrate as cal
    r = cal._Fit(a=a, b=b, objective_bits=0.0, n_target=1, n_nontarget=1, n_nan=0, n_bad_index=0, n_iter=1, status=0)
    return cal.Calibration(torch.from_numpy(np.frombuffer(bytes(r), dtype=np.float64).copy()).to(DEV))


@pytest.mark.parametrize("rows", [1, 7, 8, 9])
@pytest.mark.parametrize("cols", [1, 255, 256, 257])
def test_apply_is_numpys_product_and_sum_bit_for_bit(rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    a, b = 0.04268166328079601, 1.504446028184007
    host = rng.normal(-40.0, 30.0, (rows, cols + 5))
    cal = _record(a, b)
    want = a * host[:, :cols] + b
    dev = _dev(host)
    out = cal.apply(dev[:, :cols])                                           # strided input
    assert np.array_equal(out.cpu().numpy(), want)
    wide = torch.full((rows, cols + 3), 7.0, dtype=torch.float64, device=DEV)
    cal.apply(dev[:, :cols], out=wide[:, :cols])                             # strided output
    assert np.array_equal(wide.cpu().numpy()[:, :cols], want) and bool((wide[:, cols:] == 7.0).all())
    view = dev[:, :cols]
    assert cal.apply(view, out=view) is view                                 # in place
    assert np.array_equal(dev.cpu().numpy()[:, :cols], want) and np.array_equal(dev.cpu().numpy()[:, cols:], host[:, cols:])


def test_apply_keeps_a_symmetric_matrix_symmetric():
    rng = np.random.default_rng(1)
    m = rng.normal(-40.0, 30.0, (259, 259))
    m = m + m.T
    out = _record(0.0376886892673981, -1.3391021341582696).apply(_dev(m)).cpu().numpy()
    assert np.array_equal(out, out.T) and np.array_equal(out, 0.0376886892673981 * m + -1.3391021341582696)


# ---------------------------------------------------------------- Cllr and the actual DCF

def _check_cllr(got, l, tgt, n_launched, what, c_miss=1.0, c_fa=1.0, p=0.5):
    want = float(calib_ref.cllr(l, tgt))
    bound = (_c(n_launched) + 4) * EPS * want
    act, p_miss, p_fa = calib_ref.act_dcf(l, tgt, c_miss, c_fa, p)
    print(f"{what}: cllr {got.cllr!r} against {want!r}: off by {abs(got.cllr - want):.3e} (bound {bound:.3e}); act_dcf {got.act_dcf!r}")
    assert abs(got.cllr - want) <= bound, what
    assert (got.p_miss, got.p_fa, got.act_dcf) == (p_miss, p_fa, act), what
    assert abs(got.threshold - calib_ref.bayes_threshold(c_miss, c_fa, p)) <= 8 * EPS * (abs(np.log((1 - p) * c_fa)) + abs(np.log(p * c_miss)))
    assert (got.n_target, got.n_nontarget) == (int(tgt.sum()), int((~tgt).sum()))


@pytest.mark.parametrize("n", [2, B - 1, B + 1, ROUND - 1, ROUND + 1, 5 * ROUND + 3])
def test_cllr_and_act_dcf_against_the_restatement(n):
    from xvector_amd import calibrate as cal, TrialList, evaluate_trials
    rng = np.random.default_rng(400 + n)
    l, tgt = calib_ref.grid_llrs(rng, max(1, n // 3), n - max(1, n // 3))
    for c_miss, c_fa, p in ((1.0, 1.0, 0.5), (10.0, 1.0, 0.05)):
        w = Window(n, 0xFF)
        got = cal.cllr(_dev(l), _dev(tgt, torch.uint8), c_miss, c_fa, p, workspace=w.ws)
        assert w.intact()
        _check_cllr(got, l, tgt, n, f"vector form, n = {n}, p_target {p}", c_miss, c_fa, p)
        if n > 2:                              # on the scale of min_dcf, and never below it
            trials = TrialList(np.zeros(n, int), np.arange(n), tgt)
            assert got.act_dcf >= evaluate_trials(_dev(l).reshape(1, -1), trials, c_miss, c_fa, p).min_dcf
    # the index form over a strided matrix with NaN cells and bad indices, and every cell as a trial
    rows, cols = 11, 23
    host = np.round(rng.normal(0.0, 3.0, (rows, cols + 4)) * 1024) / 1024
    host[2, 3] = host[7, 1] = np.nan
    row, col, t = rng.integers(0, rows, n), rng.integers(0, cols, n), rng.random(n) < 0.5
    t[0], t[-1] = True, False
    row[0], col[0], row[-1], col[-1] = 0, 0, 1, 1
    if n > 2:
        row[1], col[2] = rows, -5
    s, tk, n_nan, n_bad = calib_ref.select_trials(host[:, :cols], row, col, t)
    got = cal.cllr(_dev(host)[:, :cols], TrialList(row, col, t))
    assert (got.n_nan, got.n_bad_index) == (n_nan, n_bad)
    _check_cllr(got, s, tk, n, f"index form, n = {n}")
    labels = rng.integers(0, 3, rows)
    s, tk, n_nan, _ = calib_ref.select_all_pairs(host[:, :rows], labels, labels, True)
    got = cal.cllr_all_pairs(_dev(host)[:, :rows], labels)
    assert got.n_nan == n_nan
    _check_cllr(got, s, tk, rows * rows, "all pairs")


def test_cllr_exact_values_and_infinities():
    from xvector_amd import calibrate as cal
    tgt = np.arange(ROUND + 77) % 3 == 0
    r = cal.cllr(_dev(np.zeros(len(tgt))), _dev(tgt, torch.uint8))
    assert r.cllr == 1.0                                                     # all-zero LLRs: exactly one bit
    assert (r.p_miss, r.p_fa, r.act_dcf) == (1.0, 0.0, 0.5)                  # an LLR AT the Bayes threshold is rejected
    r = cal.cllr(_dev(np.array([0.0, 2.0, -1.0, 0.0])), _dev(np.array([1, 1, 0, 0]), torch.uint8))
    assert (r.p_miss, r.p_fa) == (0.5, 0.0)
    r = cal.cllr(_dev(np.array([-np.inf, 2.0, -1.0])), _dev(np.array([1, 1, 0]), torch.uint8))
    assert r.cllr == np.inf                                                  # a target at -inf
    r = cal.cllr(_dev(np.array([np.inf, 2.0, -np.inf])), _dev(np.array([1, 1, 0]), torch.uint8))
    assert np.isfinite(r.cllr) and abs(r.cllr - float(calib_ref.cllr(np.array([np.inf, 2.0, -np.inf]), np.array([1, 1, 0])))) < 1e-15
    r = cal.cllr(_dev(np.array([1.0, 2.0])), _dev(np.array([1, 1]), torch.uint8))
    assert np.isnan([r.cllr, r.act_dcf]).all() and (r.n_target, r.n_nontarget) == (2, 0)


# ---------------------------------------------------------------- PAV

def strictly_convex(groups):
    s = np.concatenate([np.full(j + 1, float(j)) for j in range(1, groups + 1)])
    t = np.concatenate([np.r_[np.ones(j - 1, bool), np.zeros(2, bool)] for j in range(1, groups + 1)])
    return s, t


def _pav_cases():
    rng = np.random.default_rng(9)
    cases = {"all equal": (np.full(41, -3.25), np.arange(41) % 3 == 0),
             "separated": (np.r_[rng.uniform(-9, -1, 30), rng.uniform(1, 9, 21)], np.r_[np.zeros(30, bool), np.ones(21, bool)]),
             "reversed": (np.r_[rng.uniform(-9, -1, 30), rng.uniform(1, 9, 21)], np.r_[np.ones(30, bool), np.zeros(21, bool)]),
             "strictly convex, 60 groups": strictly_convex(60),
             "strictly convex, three levels": strictly_convex(400),
             "collinear runs": (np.arange(600.0), np.arange(600) % 2 == 0),
             "collinear tie groups": (np.repeat(np.arange(150.0), 4), np.tile([True, False, False, True], 150))}
    for n in (CH - 1, CH, CH + 1, CH * F - 1, CH * F + 1, CH * CH * F + 1):
        s, t = _draw(rng, n, ties=True)
        cases[f"n = {n}"] = (s, t)
    perm = rng.permutation(80600)
    s, t = cases["strictly convex, three levels"]
    cases["strictly convex, three levels"] = (s[perm], t[perm])
    return cases


PAV_CASES = _pav_cases()


def _check_pav(got, s, tgt, what, left_out=0):
    k_end, tp_end = calib_ref.pav(s, tgt)
    assert got.n_segments == len(k_end), (what, got.n_segments, len(k_end))
    assert np.array_equal(got.k_end, k_end) and np.array_equal(got.tp_end, tp_end), what
    assert (got.n_target, got.n_nontarget, got.n_left_out) == (int(tgt.sum()), int((~tgt).sum()), left_out), what
    want, abs_terms = calib_ref.min_cllr_from_segments(k_end, tp_end)
    llr, t, f, P, N = calib_ref.segment_llrs(k_end, tp_end)
    inner = (t > 0) & (f > 0)
    logs = float(np.abs(np.log(t[inner] / f[inner])).max() + abs(np.log(P / N))) if inner.any() else 0.0
    bound = ((-(-len(k_end) // B) + 9 + ULPS) * abs_terms + 8 * logs) * EPS
    print(f"{what}: {len(k_end)} segments, min_cllr {got.min_cllr!r} against {float(want)!r}: off by "
          f"{abs(got.min_cllr - float(want)):.3e} (bound {bound:.3e})")
    assert abs(got.min_cllr - float(want)) <= bound, what
    s32 = np.sort(s.astype(np.float32))
    assert np.array_equal(got.score, s32[k_end - 1]), what                    # the largest score of every segment
    with np.errstate(divide="ignore"):
        assert np.allclose(got.llr[inner], llr[inner].astype(np.float64), rtol=0, atol=8 * EPS * max(logs, 1.0)), what
    assert (got.llr[t == 0] == -np.inf).all() and (got.llr[f == 0] == np.inf).all(), what


@pytest.mark.parametrize("name", sorted(PAV_CASES))
def test_pav_segments_are_the_restatements(name):
    from xvector_amd import calibrate as cal
    _consts_are_the_modules()
    s, tgt = PAV_CASES[name]
    w = Window(len(s), 0xFF)
    got = cal.pav_segments(_dev(s), _dev(tgt, torch.uint8), workspace=w.ws)
    assert w.intact()
    _check_pav(got, s, tgt, name)
    if name == "all equal":
        assert got.n_segments == 1 and got.min_cllr == 1.0
    if name == "separated":
        assert got.n_segments == 2 and got.min_cllr == 0.0
    if name in ("reversed", "collinear runs", "collinear tie groups"):
        assert got.n_segments == 1
    if name.startswith("strictly convex"):
        assert got.n_segments == len(np.unique(s))                           # every tie group is a vertex


def test_pav_on_the_fixture_index_form_left_out_trials_and_capacity(g12):
    from xvector_amd import calibrate as cal, TrialList
    s, tgt, refs = g12
    got = cal.pav_segments(_dev(s), _dev(tgt, torch.uint8))
    _check_pav(got, s, tgt, "fixture")
    assert cal.min_cllr(_dev(s), _dev(tgt, torch.uint8)) == got.min_cllr
    # min_cllr <= cllr after the fit at p_target = 0.5, on the device's own numbers
    c = cal.fit_calibration(_dev(s), _dev(tgt, torch.uint8), 0.5)
    fitted = cal.cllr(c.apply(_dev(s).reshape(1, -1)).reshape(-1), _dev(tgt, torch.uint8)).cllr
    assert got.min_cllr <= fitted and abs(fitted - c.result().objective_bits) < 1e-12
    # the index form over a strided matrix, NaN cells and bad indices left out
    rng = np.random.default_rng(11)
    n, rows, cols = CH * F + 300, 19, 31
    host = np.round(rng.normal(-40.0, 30.0, (rows, cols + 2)))
    host[4, 4] = host[9, 30] = np.nan
    row, col, t = rng.integers(0, rows, n), rng.integers(0, cols, n), rng.random(n) < 0.3
    row[5], col[77] = -1, cols
    sk, tk, n_nan, n_bad = calib_ref.select_trials(host[:, :cols], row, col, t)
    got = cal.pav_segments(_dev(host)[:, :cols], TrialList(row, col, t))
    _check_pav(got, sk, tk, "index form", n_nan + n_bad)
    # a capacity below the count truncates the list and still reports the count
    s, tgt = PAV_CASES["strictly convex, 60 groups"]
    full = cal.pav_segments(_dev(s), _dev(tgt, torch.uint8))
    part = cal.pav_segments(_dev(s), _dev(tgt, torch.uint8), capacity=7)
    assert part.n_segments == full.n_segments == 60 and len(part.k_end) == 7 and part.min_cllr == full.min_cllr
    assert np.array_equal(part.k_end, full.k_end[:7]) and np.array_equal(part.llr, full.llr[:7])


# ---------------------------------------------------------------- end to end

def test_score_fit_apply_report_on_planted_speakers(synth):
    from xvector_amd import calibrate as cal, evaluate_all_pairs, TrialList
    from xvector_amd.scoring import PldaScorer
    dim = 24
    x, labels = calib_ref.planted(8, 6, dim, seed=3)
    scorer = PldaScorer(*synth.make_plda(dim, 8, seed=3), device=DEV)
    S = scorer.score(x)
    host = S.cpu().numpy()
    # on the restatement first: the fit lowers Cllr, and a > 0 keeps the order and with it the EER
    s, tgt, _, _ = calib_ref.select_all_pairs(host, labels, labels, True)
    ref = calib_ref.fit(s, tgt, 0.5)
    a, b = float(ref["a"]), float(ref["b"])
    assert ref["converged"] and a > 0 and float(calib_ref.cllr(a * s + b, tgt)) < float(calib_ref.cllr(s, tgt))
    assert eer_ref.by_sort((a * s + b)[tgt], (a * s + b)[~tgt]).eer == eer_ref.by_sort(s[tgt], s[~tgt]).eer
    # the device
    c = cal.fit_calibration_all_pairs(S, labels)
    llr = c.apply(S)
    r = c.result()
    _check_fit(r, s, tgt, 0.5, host.size, "planted speakers")
    n = len(labels)
    off = ~np.eye(n, dtype=bool)
    ii, jj = np.nonzero(off)
    trials = TrialList(ii, jj, labels[ii] == labels[jj])
    raw, rep = cal.calibration_report(S, trials), cal.calibration_report(llr, trials)
    print(f"planted speakers: a {r.a:.6f}, b {r.b:.6f}; raw {raw}; calibrated {rep}")
    assert rep.cllr < raw.cllr and abs(rep.cllr - r.objective_bits) < 1e-12
    assert rep.eer == raw.eer == evaluate_all_pairs(S, labels).eer
    assert rep.min_cllr <= rep.cllr and abs(rep.calibration_loss - (rep.cllr - rep.min_cllr)) == 0.0
    assert rep.act_dcf >= rep.min_dcf and (rep.n_target, rep.n_nontarget) == (int(tgt.sum()), int((~tgt).sum()))
    # ScoreCalibrator is the same fit and the same map
    sc = cal.ScoreCalibrator().fit_all_pairs(S, labels)
    assert sc.calibration.record.cpu().numpy().tobytes() == c.record.cpu().numpy().tobytes()
    assert torch.equal(sc.calibrate(S), llr)
