"""numpy restatement of score fusion (include/xvec_fuse.h), the reference of tests/test_fuse*.py: the terms and the trial forms,
the standardisation with the exact constant rule, the prior-weighted logistic fit over K terms by Newton's method in
np.longdouble, the bounds a device fit has to stay inside, and the cases the GPU tests run (so that tests/test_fuse.py can
show on the CPU what they rely on).  A plain module like calib_ref.py, whose softplus and logistic it uses."""
import numpy as np

from calib_ref import EPS, LD, LN2, softplus

MATRIX, ROW, COL = 0, 1, 2
MAX_TERMS = 8
STEP_TOL = 1e-9
STEP_CAP = 8.0
B, ITEMS, MAX_BLOCKS = 256, 8, 1024


def term_ulps(k):
    """XVEC_FUSE_TERM_ULPS(K): 4 K + 1 roundings of the argument at calibration's 58 / 5 units each, six for the rest."""
    return 6 + -(-58 * (4 * k + 1) // 5)


def sum_constant(n, k):
    """c of the header's bound c eps sum |terms| for a pass over n trials (n as launched: left-out trials keep their places)."""
    blocks = min(-(-n // (B * ITEMS)), MAX_BLOCKS)
    return -(-n // (blocks * B)) + 22 + term_ulps(k)


# ---------------------------------------------------------------- the terms and the trial forms

def term_values(terms, rows, cols):
    """[K, n] float64: every term (kind, array) at the cells (rows[t], cols[t])."""
    out = np.empty((len(terms), len(rows)))
    for k, (kind, a) in enumerate(terms):
        a = np.asarray(a, dtype=np.float64)
        out[k] = a[rows, cols] if kind == MATRIX else a[rows] if kind == ROW else a[cols]
    return out


def select_trials(terms, n_rows, n_cols, row_idx, col_idx, is_target):
    """(F [K, kept] float64, target bool, n_nan, n_bad_index) of the trials kept, in trial order; row_idx = col_idx = None:
    the plain vector, trial t the cell (0, t).  A trial with a NaN in ANY term counts once."""
    tgt = np.asarray(is_target).astype(bool)
    if row_idx is None:
        r, c = np.zeros(len(tgt), dtype=np.int64), np.arange(len(tgt))
    else:
        r, c = np.asarray(row_idx, dtype=np.int64), np.asarray(col_idx, dtype=np.int64)
    ok = (r >= 0) & (r < n_rows) & (c >= 0) & (c < n_cols)
    F = np.zeros((len(terms), len(tgt)))
    F[:, ok] = term_values(terms, r[ok], c[ok])
    nan = ok & np.isnan(F).any(axis=0)
    keep = ok & ~nan
    return F[:, keep], tgt[keep], int(nan.sum()), int((~ok).sum())


def select_all_pairs(terms, n_rows, n_cols, row_class, col_class, skip_diagonal):
    r, c = (v.ravel() for v in np.meshgrid(np.arange(n_rows), np.arange(n_cols), indexing="ij"))
    tgt = np.asarray(row_class)[r] == np.asarray(col_class)[c]
    F = term_values(terms, r, c)
    off = r != c if skip_diagonal else np.ones(len(r), dtype=bool)
    nan = off & np.isnan(F).any(axis=0)
    keep = off & ~nan
    return F[:, keep], tgt[keep], int(nan.sum()), 0


# ---------------------------------------------------------------- the fit

def standardise(F):
    """(mu, sd, constant) in longdouble.  A term is constant iff its minimum equals its maximum, exactly; then mu is that value
    and sd 1."""
    F = np.asarray(F, dtype=np.float64)
    n = F.shape[1]
    const = F.min(axis=1) == F.max(axis=1)
    Fl = F.astype(LD)
    mu = np.where(const, Fl[:, 0], Fl.sum(axis=1) / n)
    sd = np.sqrt(((Fl - mu[:, None]) ** 2).sum(axis=1) / n)
    sd = np.where(const | ~(sd > 0), LD(1), sd)
    return mu, sd, const


def _solve(A, Bm):
    """A X = B by Gaussian elimination with partial pivoting in A's own type (numpy.linalg has no longdouble); None where a
    pivot falls below 1e-13 of the largest entry (singular to the purpose)."""
    A, X = A.copy(), Bm.copy()
    m = len(A)
    scale = np.abs(A).max()
    for j in range(m):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        if not np.abs(A[p, j]) > 1e-13 * scale:
            return None
        if p != j:
            A[[j, p]], X[[j, p]] = A[[p, j]], X[[p, j]]
        for i in range(j + 1, m):
            f = A[i, j] / A[j, j]
            A[i, j:] -= f * A[j, j:]
            X[i] -= f * X[j]
    for j in range(m - 1, -1, -1):
        X[j] = (X[j] - A[j, j + 1:] @ X[j + 1:]) / A[j, j]
    return X


def _derivatives(Z, tgt, w, tau, l2, x):
    """The penalised objective, its data part, gradient, Hessian and sum |terms| of J and of every gradient component at x
    (the weights of the active terms, then the bias), in Z's type."""
    a = x @ Z + tau
    u = np.where(tgt, -a, a)
    e = np.exp(-np.abs(u))                               # calib_ref's logistic and softplus, in Z's type
    sig = np.where(u >= 0, 1 / (1 + e), e / (1 + e))
    dj = np.where(tgt, -1, 1) * w * sig
    h = w * sig * np.where(u >= 0, e / (1 + e), 1 / (1 + e))
    jt = w * (np.maximum(u, 0) + np.log1p(e))
    gt = Z * dj
    g = gt.sum(axis=1)
    H = (Z * h) @ Z.T
    pen = l2 / 2 * (x[:-1] ** 2).sum()
    g[:-1] += l2 * x[:-1]
    H[np.arange(len(x) - 1), np.arange(len(x) - 1)] += l2
    return jt.sum() + pen, jt.sum(), g, H, {"j": float(np.abs(jt).sum()), "g": np.abs(gt).sum(axis=1).astype(np.float64)}


def _newton(Z, tgt, w, tau, l2, x, step_tol, grad_tol, max_iter, floor=0.0):
    """The header's procedure (full step capped at 8 in the max norm, halved while the penalised objective rises, the damping
    rule where the Hessian is singular) in Z's type from x.  Stops when the step falls to step_tol max(1, max |x|) (if given),
    when the gradient falls to grad_tol or to `floor` roundings of its own largest sum of |terms|, or when it has stopped
    falling: the floor of the format.  Returns x, what
    _derivatives gave there, the passes made and whether a stopping rule was met."""
    J, Jd, g, H, at = _derivatives(Z, tgt, w, tau, l2, x)
    passes, best, stalled = 1, np.abs(g).max(), 0
    while passes < max_iter:
        if np.abs(g).max() <= max(grad_tol, floor * float(np.finfo(Z.dtype).eps) * at["g"].max()):
            return x, (J, Jd, g, H, at), passes, True
        d = _solve(H, -g[:, None])
        if d is None:
            d = _solve(H + (1e-12 * np.trace(H) + 1e-300) * np.eye(len(x), dtype=Z.dtype), -g[:, None])
        if d is None or not np.isfinite(d.astype(np.float64)).all():
            return x, (J, Jd, g, H, at), passes, False
        d = d[:, 0]
        big = np.abs(d).max()
        if big > STEP_CAP:
            d = d * (STEP_CAP / big)
        if step_tol is not None and big <= step_tol * max(1.0, float(np.abs(x).max())):
            return x + d, (J, Jd, g, H, at), passes, True
        scale = Z.dtype.type(1)
        while True:                                     # halve while the objective rises: every trial point is a pass
            J2, Jd2, g2, H2, at2 = _derivatives(Z, tgt, w, tau, l2, x + scale * d)
            passes += 1
            if J2 <= J + Z.dtype.type(2) ** -40 * abs(J) or scale < 1e-12 or passes >= max_iter:
                break
            scale /= 2
        x, J, Jd, g, H, at = x + scale * d, J2, Jd2, g2, H2, at2
        if np.abs(g).max() < best:
            best, stalled = np.abs(g).max(), 0
        else:
            stalled += 1
            if stalled >= 2:
                return x, (J, Jd, g, H, at), passes, bool(best <= 1e3 * np.finfo(Z.dtype).eps * at["g"].max())
    return x, (J, Jd, g, H, at), passes, False


def weakly_separable(Z, tgt):
    """True iff some direction (v, c) puts every target at v z + c >= 0 and every non-target at <= 0 with at least one of them
    strictly inside: the logistic objective then has no minimum without a ridge.  A linear programme (scipy): maximise the sum
    of the signed margins subject to each being >= 0, (v, c) in the unit box.  Z: [m, n] float64, its last row the ones."""
    from scipy.optimize import linprog
    M = (np.where(tgt, 1.0, -1.0) * Z).T                 # [n, m]: the signed margins are M @ (v, c)
    res = linprog(-M.sum(axis=0), A_ub=-M, b_ub=np.zeros(len(M)), bounds=[(-1, 1)] * M.shape[1], method="highs")
    return bool(res.status == 0 and -res.fun > 1e-9 * len(M))


LP_LIMIT = 20000      # trials up to which the linear programme is asked; beyond it only the iteration itself is


def fit(F, tgt, p_target, l2=0.0, grad_tol=1e-25, max_iter=200):
    """The restatement.  F [K, n] float64 (the trials kept), tgt bool.  Newton's method as the header states it, first in
    float64 until the header's stopping rule is met (`passes`: what a device fit makes, rounding aside), then in longdouble
    until the gradient is at the format's floor.  `converged` is False for a set without a minimum: one the first phase does
    not finish within max_iter passes, or (l2 == 0, up to LP_LIMIT trials) one that weakly_separable finds.  Returns a dict:
    w [K], b (raw coordinates; w exactly 0 for a constant term), x_std (the active weights, then the bias), active, constant,
    mu, sd, J (penalised), J_data, penalty, H, H_inv (inf where H is singular), abs_terms, grad, passes, converged, l2."""
    F = np.asarray(F, dtype=np.float64)
    tgt = np.asarray(tgt).astype(bool)
    K, n = F.shape
    p = LD(p_target)
    mu, sd, const = standardise(F)
    active = np.nonzero(~const)[0]
    Zl = np.vstack([(F[active].astype(LD) - mu[active, None]) / sd[active, None], np.ones((1, n), dtype=LD)])
    wl = np.where(tgt, p / tgt.sum(), (1 - p) / (~tgt).sum())
    tau = np.log(p) - np.log1p(-p)
    x64, _, passes, met = _newton(Zl.astype(np.float64), tgt, wl.astype(np.float64), float(tau), float(l2),
                                  np.zeros(len(active) + 1), STEP_TOL, 0.0, max_iter)
    x, (J, Jd, g, H, at), _, floor = _newton(Zl, tgt, wl, tau, LD(l2), x64.astype(LD), None, grad_tol, 30, floor=16.0)
    converged = bool(met and floor)
    if converged and l2 == 0 and n <= LP_LIMIT and weakly_separable(Zl.astype(np.float64), tgt):
        converged = False
    inv = _solve(H, np.eye(len(x), dtype=LD))
    H_inv = inv if inv is not None else np.full(H.shape, np.inf)
    w = np.zeros(K, dtype=LD)
    w[active] = x[:-1] / sd[active]
    b = x[-1] - (w * mu).sum()
    return dict(w=w, b=b, x_std=x, active=active, constant=const, mu=mu, sd=sd, J=J, J_data=Jd, penalty=J - Jd, H=H, H_inv=H_inv,
                abs_terms=at, grad=float(np.abs(g).max()), passes=passes, converged=converged, l2=float(l2), g=g)


def objective(F, tgt, w, b, p_target):
    """The data part of J at raw weights, in longdouble."""
    p = LD(p_target)
    x = np.asarray(w, dtype=LD) @ np.asarray(F, dtype=LD) + LD(b) + (np.log(p) - np.log1p(-p))
    return p / tgt.sum() * softplus(-x[tgt]).sum() + (1 - p) / (~tgt).sum() * softplus(x[~tgt]).sum()


def fit_bounds(ref, c):
    """(bounds on w [K], bound on b, bound on objective_bits, bound on penalty_bits) of a device fit whose sums each carry an
    error below c eps sum |terms| (include/xvec_fuse.h), generalised from calib_ref.fit_bounds.  In standardised coordinates
    every parameter moves by at most
        std = 4 ||H^-1||_inf max_k err_k  +  ||H^-1||_inf |the restatement's own residual gradient|,
        err_k = c eps sum |g_k terms|  +  (2 c + 2) eps l2 |w'_k|
    (the second part: the ridge's own product and sum, and the device's sd, a sum of depth below c, inside w'_k = w_k sd_k).
    w_k = w'_k / sd_k carries that with 1 / sd_k, b = b' - sum_k w_k mu_k with 1 + sum_k |mu_k| / sd_k, plus their own
    roundings (4 for a weight as in calibration; a product and a sum per term, the weight's quotient and the last difference
    for the bias).  The data part of J moves by its own sum's error, by the gradient sums' size times the parameters' movement,
    and, as objective_bits is taken at the point the last step d left from, by l2 sum |w'_k| max |d| with
    max |d| <= STEP_TOL max(1, max |x|); the ridge part by that and l2 sum |w'_k| std, plus its K + 3 roundings."""
    at, x, act = ref["abs_terms"], np.abs(ref["x_std"].astype(np.float64)), ref["active"]
    K, l2 = len(ref["w"]), ref["l2"]
    h_norm = float(np.abs(ref["H_inv"]).sum(axis=1).max())
    err = c * EPS * at["g"] + (2 * c + 2) * EPS * l2 * np.r_[x[:-1], 0.0]
    std = 4.0 * h_norm * float(err.max()) + h_norm * ref["grad"]
    sd, mu = ref["sd"].astype(np.float64), np.abs(ref["mu"].astype(np.float64))
    bound_w = np.zeros(K)
    bound_w[act] = std / sd[act] + 4 * EPS * x[:-1] / sd[act]
    bound_b = std * (1 + (mu[act] / sd[act]).sum()) + (2 * K + 2) * EPS * (x[-1] + (x[:-1] * mu[act] / sd[act]).sum())
    step = STEP_TOL * max(1.0, float(x.max()))
    ridge = l2 * float(x[:-1].sum())
    bound_j = (c * EPS * at["j"] + len(x) * float(at["g"].max()) * std + ridge * step) / float(LN2)
    bound_p = (ridge * (std + step) + (K + 3) * EPS * float(ref["penalty"])) / float(LN2)
    return bound_w, bound_b, bound_j, bound_p


# ---------------------------------------------------------------- the planted cases of the GPU tests

def planted(n_speakers=12, per_speaker=6, dim=16, noise=1.5, seed=0):
    """Planted speakers and what the fits fuse: x [n, dim], labels, a cosine matrix, a noisy symmetric dot-product matrix, two
    more cosine matrices of perturbed vectors, integer durations in 100 .. 999 and a second row-side measure."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_speakers, dim))
    labels = np.repeat(np.arange(n_speakers), per_speaker)
    x = centres[labels] + noise * rng.standard_normal((len(labels), dim))
    n = len(labels)

    def cosine(v):
        u = v / np.linalg.norm(v, axis=1, keepdims=True)
        return u @ u.T
    e = rng.standard_normal((n, n))
    dot = x @ x.T + 2.0 * (e + e.T)
    e2 = rng.standard_normal((n, n))
    return dict(x=x, labels=labels, n=n, cos=cosine(x), dot=dot, cos_a=cosine(x + 0.8 * rng.standard_normal(x.shape)),
                cos_b=cosine(x + 0.8 * rng.standard_normal(x.shape)), dot_c=x @ x.T + 3.0 * (e2 + e2.T),
                dur=rng.integers(100, 1000, n), snr=rng.normal(15.0, 5.0, n))


def upper_triangle(n, labels):
    """The n (n - 1) / 2 trials i < j: (row_idx, col_idx, is_target)."""
    r, c = np.triu_indices(n, 1)
    return r.astype(np.int32), c.astype(np.int32), labels[r] == labels[c]


def planted_terms(pl, k):
    """The K = 2, 3, 4 and 8 term lists of the planted case."""
    logdur = np.log(pl["dur"].astype(np.float64))
    return {2: [(MATRIX, pl["cos"]), (MATRIX, pl["dot"])],
            3: [(MATRIX, pl["cos"]), (ROW, logdur), (COL, logdur)],
            4: [(MATRIX, pl["cos"]), (MATRIX, pl["dot"]), (ROW, logdur), (COL, logdur)],
            8: [(MATRIX, pl["cos"]), (MATRIX, pl["dot"]), (ROW, logdur), (COL, logdur), (MATRIX, pl["cos_a"]),
                (MATRIX, pl["cos_b"]), (MATRIX, pl["dot_c"]), (ROW, pl["snr"])]}[k]


PLANTED_CASES = [(2, 0.5), (3, 0.5), (4, 0.5), (4, 0.01), (8, 0.5)]      # (K, p_target)
GPU_MAX_ITER = 50                                                        # what the GPU tests pass (the module's default)


def separable_set(n=300, seed=7):
    """(F [2, n], tgt): two terms, the first of which separates the classes."""
    rng = np.random.default_rng(seed)
    tgt = rng.random(n) < 0.35
    tgt[0], tgt[-1] = True, False
    return np.vstack([np.where(tgt, rng.uniform(1.0, 5.0, n), rng.uniform(-5.0, -1.0, n)), rng.normal(0.0, 1.0, n)]), tgt


def draw(rng, n, k):
    """n overlapping trials of k terms on scales of their own (a PLDA-like first term), both classes present for n >= 2."""
    tgt = rng.random(n) < 0.35
    tgt[0], tgt[-1] = True, False
    F = np.empty((k, n))
    F[0] = np.where(tgt, rng.normal(-22.0, 24.0, n), rng.normal(-50.0, 27.0, n))
    for q in range(1, k):
        F[q] = np.where(tgt, rng.normal(0.3 * q, 1.0, n), rng.normal(-0.2, 1.0 + 0.1 * q, n)) * 10.0 ** (q % 3 - 1) + q
    return F, tgt


# ---------------------------------------------------------------- the other inputs of the GPU tests, host side

def vector_case(n):
    """Three drawn terms and a fourth that is constant (a ROW term of the one row), n trials."""
    F, tgt = draw(np.random.default_rng(100 + n), n, 3)
    return np.vstack([F, np.full(n, 5.25)]), tgt


VECTOR_SIZES = [2, B * ITEMS - 1, B * ITEMS, B * ITEMS + 1]       # one per class; the 2048-trial round of a block and one beyond it
BIG_N = 2 ** 21 + 5                                               # above MAX_BLOCKS rounds: every block takes a second one


def big_case():
    return draw(np.random.default_rng(2), BIG_N, 2)


def index_case():
    """13 x 29 cells, B * ITEMS + 1 trials: a MATRIX term with NaN cells, a second MATRIX term that is NaN in one of them too (a
    trial counts once), a ROW and a COL term; trials with a row or a column outside the matrix."""
    rng = np.random.default_rng(200)
    rows, cols, n = 13, 29, B * ITEMS + 1
    m0 = rng.normal(-40.0, 30.0, (rows, cols))
    m0[rng.random((rows, cols)) < 0.03] = np.nan
    m1 = rng.normal(0.0, 1.0, (rows, cols))
    both = tuple(int(v) for v in np.argwhere(np.isnan(m0))[-1])
    m1[both] = np.nan
    rq, cq = rng.normal(5.0, 0.5, rows), rng.normal(6.0, 0.7, cols)
    m0[0, 0], m0[1, 1] = -10.0, -60.0
    order = np.argsort(np.nan_to_num(m0, nan=-40.0).ravel())
    tgt = rng.random(n) < 0.4
    pick = np.where(tgt, rng.choice(order[len(order) // 3:], n), rng.choice(order[: 2 * len(order) // 3], n))
    row, col = pick // cols, pick % cols
    tgt[0], tgt[-1] = True, False
    row[0], col[0], row[-1], col[-1] = 0, 0, 1, 1
    row[5], col[5] = both
    bad = np.nonzero(rng.random(n) < 0.05)[0]
    bad = bad[(bad > 5) & (bad < n - 1)]
    row[bad[::2]] = rows + 3
    col[bad[1::2]] = -1
    return dict(terms=[(MATRIX, m0), (MATRIX, m1), (ROW, rq), (COL, cq)], rows=rows, cols=cols, row=row, col=col, tgt=tgt)


ALL_PAIRS_SHAPES = [(7, 300), (45, 45)]


def all_pairs_case(shape):
    """(terms, row classes, column classes, skip_diagonal): a matrix with a NaN cell, a ROW, a COL and a second MATRIX term;
    the square one shares its classes and skips the diagonal."""
    rows, cols = shape
    rng = np.random.default_rng(300 + rows * cols)
    rc = rng.integers(0, 4, rows)
    cc = rng.integers(0, 4, cols) if rows != cols else rc
    same = rc[:, None] == cc[None, :]
    m = np.where(same, rng.normal(-22.0, 24.0, shape), rng.normal(-50.0, 27.0, shape))
    m2 = np.where(same, rng.normal(0.5, 1.0, shape), rng.normal(-0.5, 1.0, shape))
    m[3, 5] = np.nan
    rq, cq = rng.normal(5.0, 0.5, rows), rng.normal(6.0, 0.7, cols)
    return [(MATRIX, m), (ROW, rq), (COL, cq), (MATRIX, m2)], rc, cc, rows == cols


def constant_case():
    """(F [2, 700], tgt, the value of the constant term: one whose rounded mean over 700 trials is not itself)."""
    F, tgt = draw(np.random.default_rng(8), 700, 2)
    return F, tgt, 0.1


def identical_case():
    """(F [2, 500], tgt): one drawn term, twice."""
    F, tgt = draw(np.random.default_rng(9), 500, 1)
    return np.vstack([F[0], F[0]]), tgt


def gpu_fit_cases(big=True):
    """(name, F, tgt, p_target, l2, has a unique minimum) of every fit tests/test_fuse_gpu.py holds to fit_bounds, but for the
    end-to-end one (its PLDA scores come from the device)."""
    pl = planted()
    r, c, t = upper_triangle(pl["n"], pl["labels"])
    for k, p in PLANTED_CASES:
        F, tgt, _, _ = select_trials(planted_terms(pl, k), pl["n"], pl["n"], r, c, t)
        yield f"planted K = {k}, p_target {p}", F, tgt, p, 0.0, True
    for n in VECTOR_SIZES:
        F, tgt = vector_case(n)
        yield f"vector form n = {n}", F, tgt, 0.5, 0.0, n > 2
    if big:
        F, tgt = big_case()
        yield f"vector form n = {BIG_N}", F, tgt, 0.5, 0.0, True
    ic = index_case()
    F, tgt, _, _ = select_trials(ic["terms"], ic["rows"], ic["cols"], ic["row"], ic["col"], ic["tgt"])
    yield "index form", F, tgt, 0.5, 0.0, True
    for shape in ALL_PAIRS_SHAPES:
        terms, rc, cc, skip = all_pairs_case(shape)
        F, tgt, _, _ = select_all_pairs(terms, shape[0], shape[1], rc, cc, skip)
        yield f"all pairs {shape}", F, tgt, 0.5, 0.0, True
    F, tgt, value = constant_case()
    yield "constant term", np.insert(F, 1, np.full(F.shape[1], value), axis=0), tgt, 0.5, 0.0, True
    F, tgt = identical_case()
    yield "identical terms, l2 = 1e-3", F, tgt, 0.5, 1e-3, True
    F, tgt = separable_set()
    yield "separable set, l2 = 0", F, tgt, 0.5, 0.0, False
    yield "separable set, l2 = 1e-3", F, tgt, 0.5, 1e-3, True
