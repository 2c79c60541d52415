"""numpy restatement of score calibration (include/xvec_calib.h), the reference of tests/test_calibrate*.py: the trial forms,
the prior-weighted logistic fit by Newton's method in np.longdouble, Cllr and the actual DCF, and pool-adjacent-violators as
the greatest convex minorant of the cumulative-sum diagram with exact (Python) integers.  A plain module like snorm_ref.py."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
LN2 = np.log(LD(2))


# ---------------------------------------------------------------- the trial forms

def select_trials(scores, row_idx, col_idx, is_target):
    """(scores float64, target bool, n_nan, n_bad_index) of the trials kept, in trial order.  `scores` [n_rows, n_cols];
    row_idx = col_idx = None: the plain vector scores[0, :len(is_target)]."""
    scores = np.asarray(scores, dtype=np.float64)
    tgt = np.asarray(is_target).astype(bool)
    if row_idx is None:
        s, ok = scores[0, : len(tgt)], np.ones(len(tgt), dtype=bool)
    else:
        r, c = np.asarray(row_idx, dtype=np.int64), np.asarray(col_idx, dtype=np.int64)
        ok = (r >= 0) & (r < scores.shape[0]) & (c >= 0) & (c < scores.shape[1])
        s = np.full(len(tgt), 0.0)
        s[ok] = scores[r[ok], c[ok]]
    nan = ok & np.isnan(s)
    keep = ok & ~nan
    return s[keep], tgt[keep], int(nan.sum()), int((~ok).sum())


def select_all_pairs(scores, row_class, col_class, skip_diagonal):
    scores = np.asarray(scores, dtype=np.float64)
    tgt = np.asarray(row_class)[:, None] == np.asarray(col_class)[None, :]
    keep = ~np.isnan(scores)
    n_nan = int((~keep).sum())
    if skip_diagonal:
        off = ~np.eye(scores.shape[0], scores.shape[1], dtype=bool)
        n_nan = int((~keep & off).sum())
        keep &= off
    return scores[keep], tgt[keep], n_nan, 0


# ---------------------------------------------------------------- the fit

def softplus(x):
    x = np.asarray(x, dtype=LD)
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def logistic(x):
    x = np.asarray(x, dtype=LD)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def objective(scores, tgt, a, b, p_target):
    """J(a, b) of include/xvec_calib.h in longdouble."""
    s, p = np.asarray(scores, dtype=LD), LD(p_target)
    x = LD(a) * s + LD(b) + (np.log(p) - np.log1p(-p))
    return p / tgt.sum() * softplus(-x[tgt]).sum() + (1 - p) / (~tgt).sum() * softplus(x[~tgt]).sum()


def _derivatives(z, tgt, w, tau, ab):
    x = ab[0] * z + ab[1] + tau
    u = np.where(tgt, -x, x)
    sig = logistic(u)
    dj = np.where(tgt, -1, 1) * w * sig
    h = w * sig * logistic(-u)
    terms = {"j": w * softplus(u), "ga": dj * z, "gb": dj}
    g = np.array([terms["ga"].sum(), terms["gb"].sum()], dtype=LD)
    H = np.array([[(h * z * z).sum(), (h * z).sum()], [(h * z).sum(), h.sum()]], dtype=LD)
    return terms["j"].sum(), g, H, {k: np.abs(v).sum() for k, v in terms.items()}


def fit(scores, tgt, p_target, grad_tol=1e-25, max_iter=200):
    """Newton's method in longdouble on the standardised coordinates of the header, until the gradient is below `grad_tol`
    or, where the format's own rounding keeps it above that, no longer falls.  A set one threshold separates (weakly) has no
    minimum: `converged` is False there, whatever the iteration reached.  Returns a dict: a, b (raw coordinates), ab_std,
    mu, sd, J, H and H_inv (standardised), abs_terms (sum |terms| of J, g_a, g_b), grad (the norm reached), converged."""
    s = np.asarray(scores, dtype=LD)
    tgt = np.asarray(tgt).astype(bool)
    p = LD(p_target)
    mu = s.sum() / len(s)
    sd = np.sqrt(((s - mu) ** 2).sum() / len(s))
    if not sd > 0:
        sd = LD(1)
    z = (s - mu) / sd
    w = np.where(tgt, p / tgt.sum(), (1 - p) / (~tgt).sum())
    tau = np.log(p) - np.log1p(-p)
    ab = np.zeros(2, dtype=LD)
    J, g, H, abs_terms = _derivatives(z, tgt, w, tau, ab)
    best, stalled, converged = np.abs(g).max(), 0, False
    for _ in range(max_iter):
        if np.abs(g).max() <= grad_tol:
            converged = True
            break
        det = H[0, 0] * H[1, 1] - H[0, 1] ** 2
        if not det > 1e-30 * H[0, 0] * H[1, 1]:
            break
        d = -np.array([H[1, 1] * g[0] - H[0, 1] * g[1], H[0, 0] * g[1] - H[0, 1] * g[0]], dtype=LD) / det
        scale = LD(1)
        while True:                                     # halve while the objective rises
            J2, g2, H2, abs2 = _derivatives(z, tgt, w, tau, ab + scale * d)
            if J2 <= J + LD(2) ** -60 * abs(J) or scale < 1e-12:
                break
            scale /= 2
        ab, J, g, H, abs_terms = ab + scale * d, J2, g2, H2, abs2
        if np.abs(g).max() < best:
            best, stalled = np.abs(g).max(), 0
        else:
            stalled += 1
            if stalled >= 2:                            # the floor of the format
                converged = best <= 1e3 * np.finfo(LD).eps * max(abs_terms["ga"], abs_terms["gb"])
                break
    if s[tgt].min() >= s[~tgt].max() or s[tgt].max() <= s[~tgt].min():
        converged = False
    det = H[0, 0] * H[1, 1] - H[0, 1] ** 2
    H_inv = np.array([[H[1, 1], -H[0, 1]], [-H[0, 1], H[0, 0]]], dtype=LD) / det if det > 0 else np.full((2, 2), np.inf)
    a = ab[0] / sd
    return dict(a=a, b=ab[1] - a * mu, ab_std=ab, mu=mu, sd=sd, J=J, H=H, H_inv=H_inv, abs_terms=abs_terms,
                grad=np.abs(g).max(), converged=bool(converged), g=g)


def raw_hessian_inverse(ref):
    """The inverse Hessian of J in the raw coordinates (a, b): (a', b') = T (a, b) with T = [[sd, 0], [mu, 1]], H_raw = T^T H T."""
    T = np.array([[ref["sd"], 0], [ref["mu"], 1]], dtype=LD)
    H = T.T @ ref["H"] @ T
    det = H[0, 0] * H[1, 1] - H[0, 1] ** 2
    return np.array([[H[1, 1], -H[0, 1]], [-H[0, 1], H[0, 0]]], dtype=LD) / det


def fit_bounds(ref, c):
    """(bound on a, bound on b, bound on objective_bits) of a device fit whose sums each carry an error below c eps sum |terms|
    (include/xvec_calib.h): in standardised coordinates the parameters move by at most
        4 ||H^-1||_inf c eps max(sum |g_a terms|, sum |g_b terms|)  (+ what the restatement's own gradient leaves),
    a = a' / sd and b = b' - a' mu / sd carry that over with the factors 1 / sd and 1 + |mu| / sd, plus four roundings of
    their own; J moves by its own sum's error plus the gradient sums' size times the parameters' movement."""
    t = ref["abs_terms"]
    h_norm = float(np.abs(ref["H_inv"]).sum(axis=1).max())
    gmax = float(max(t["ga"], t["gb"]))
    std = 4.0 * h_norm * c * EPS * gmax + h_norm * float(ref["grad"])
    sd, mu = float(ref["sd"]), float(ref["mu"])
    a_std, b_std = (abs(float(v)) for v in ref["ab_std"])
    bound_a = std / sd + 4 * EPS * a_std / sd
    bound_b = std * (1 + abs(mu) / sd) + 4 * EPS * (b_std + a_std * abs(mu) / sd)
    bound_j = (c * EPS * float(t["j"]) + 2 * gmax * std) / float(LN2)
    return bound_a, bound_b, bound_j


# ---------------------------------------------------------------- Cllr and the actual DCF

def cllr(llrs, tgt):
    l = np.asarray(llrs, dtype=LD)
    tgt = np.asarray(tgt).astype(bool)
    with np.errstate(over="ignore", invalid="ignore"):
        return (softplus(-l[tgt]).mean() + softplus(l[~tgt]).mean()) / (2 * LN2)


def cllr_abs_terms(llrs, tgt):
    """sum |terms| of Cllr's two means as the device weights them: what its summation bound multiplies."""
    l = np.asarray(llrs, dtype=LD)
    tgt = np.asarray(tgt).astype(bool)
    return float((softplus(-l[tgt]).mean() + softplus(l[~tgt]).mean()) / (2 * LN2))


def bayes_threshold(c_miss, c_fa, p_target):
    return float(np.log((1.0 - p_target) * c_fa) - np.log(p_target * c_miss))


def act_dcf(llrs, tgt, c_miss=1.0, c_fa=1.0, p_target=0.5):
    """(act_dcf, p_miss, p_fa): a trial is rejected iff llr <= the Bayes threshold."""
    l = np.asarray(llrs, dtype=np.float64)
    tgt = np.asarray(tgt).astype(bool)
    t = bayes_threshold(c_miss, c_fa, p_target)
    p_miss = float((l[tgt] <= t).sum()) / float(tgt.sum())
    p_fa = float((l[~tgt] > t).sum()) / float((~tgt).sum())
    return c_miss * p_miss * p_target + c_fa * p_fa * (1.0 - p_target), p_miss, p_fa


def min_dcf(scores, tgt, c_miss=1.0, c_fa=1.0, p_target=0.5):
    """The minimum over the distinct fp32 scores as thresholds (include/xvec_eval.h), in exact counts."""
    s = np.asarray(scores, dtype=np.float32).astype(np.float64)
    tgt = np.asarray(tgt).astype(bool)
    P, N = tgt.sum(), (~tgt).sum()
    best = np.inf
    for u in np.unique(s):
        frr, far = (s[tgt] <= u).sum() / P, (s[~tgt] > u).sum() / N
        best = min(best, c_miss * frr * p_target + c_fa * far * (1.0 - p_target))
    return float(best)


# ---------------------------------------------------------------- PAV

def pav(scores, tgt):
    """The segments of the greatest convex minorant of the cumulative-sum diagram of the target bit over the fp32-rounded scores
    in rising order, one point per group of equal scores: (k_end, tp_end) int64 arrays.  Collinear interior vertices are
    dropped.  Exact: Python integers."""
    s = np.asarray(scores, dtype=np.float64).astype(np.float32)
    tgt = np.asarray(tgt).astype(bool)
    order = np.argsort(s, kind="stable")
    s, t = s[order], tgt[order]
    ends = np.nonzero(np.append(s[1:] != s[:-1], True))[0]           # -0.0 == +0.0: one group, as the keys have it
    tp = np.cumsum(t)
    stack = [(0, 0)]
    for i in ends.tolist():
        p = (i + 1, int(tp[i]))
        while len(stack) >= 2:
            (ax, ay), (bx, by) = stack[-2], stack[-1]
            if (bx - ax) * (p[1] - ay) - (by - ay) * (p[0] - ax) <= 0:
                stack.pop()
            else:
                break
        stack.append(p)
    seg = np.array(stack[1:], dtype=np.int64).reshape(-1, 2)
    return seg[:, 0].copy(), seg[:, 1].copy()


def pav_values(k_end, tp_end):
    """The fitted value (the share of targets of its segment) of every trial in sorted order."""
    k0, t0 = np.concatenate([[0], k_end[:-1]]), np.concatenate([[0], tp_end[:-1]])
    return np.repeat((tp_end - t0).astype(LD) / (k_end - k0).astype(LD), k_end - k0)


def segment_llrs(k_end, tp_end):
    k0, t0 = np.concatenate([[0], k_end[:-1]]), np.concatenate([[0], tp_end[:-1]])
    t, f = (tp_end - t0).astype(LD), ((k_end - k0) - (tp_end - t0)).astype(LD)
    P, N = LD(tp_end[-1]), LD(k_end[-1] - tp_end[-1])
    with np.errstate(divide="ignore"):
        return np.log(t / np.where(f > 0, f, 1)) - np.log(P / N) + np.where(f > 0, 0, np.inf), t, f, P, N


def min_cllr_from_segments(k_end, tp_end):
    """(minCllr, sum |terms|) over the segments, in longdouble; a segment with no target or no non-target contributes 0."""
    llr, t, f, P, N = segment_llrs(k_end, tp_end)
    ok = (t > 0) & (f > 0)
    terms = (t[ok] / P * softplus(-llr[ok]) + f[ok] / N * softplus(llr[ok])) / (2 * LN2)
    return terms.sum(), float(np.abs(terms).sum())


def min_cllr_from_values(values, tgt_sorted):
    """minCllr trial by trial from isotonic fitted values p (posterior of the target at the data's own prior): the LLR of a
    trial is logit(p) - logit(P / (P + N)); trials with p = 0 or 1 on the right side of it cost nothing."""
    p = np.asarray(values, dtype=LD)
    t = np.asarray(tgt_sorted).astype(bool)
    P, N = LD(t.sum()), LD((~t).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        llr = np.log(p / (1 - p)) - np.log(P / N)
        ct = np.where(p[t] >= 1, 0, softplus(-llr[t]))
        cn = np.where(p[~t] <= 0, 0, softplus(llr[~t]))
    return (ct.sum() / P + cn.sum() / N) / (2 * LN2)


# ---------------------------------------------------------------- shared cases

def planted(n_speakers, per_speaker, dim, seed):
    """(x [n, dim] float64, labels [n]): speakers around planted centres, close enough for the scores to overlap."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_speakers, dim))
    labels = np.repeat(np.arange(n_speakers), per_speaker)
    return centres[labels] + 1.6 * rng.standard_normal((len(labels), dim)), labels


def planted_scores(x):
    """A PLDA-like symmetric score matrix of the vectors: 30 cos - 12."""
    u = x / np.linalg.norm(x, axis=1, keepdims=True)
    return 30.0 * (u @ u.T) - 12.0


def grid_llrs(rng, n_target, n_nontarget):
    """(llrs, target): overlapping LLRs on the grid 2^-10 (exact in fp32), in shuffled order."""
    l = np.concatenate([rng.normal(1.5, 2.0, n_target), rng.normal(-2.0, 2.0, n_nontarget)])
    tgt = np.concatenate([np.ones(n_target, bool), np.zeros(n_nontarget, bool)])
    order = rng.permutation(len(l))
    return np.round(l[order] * 1024) / 1024, tgt[order]
