"""The numpy oracle of the GMM-UBM unit (include/xvec_gmm.h): every call restated in the expanded form ll = g + (x, x^2) . P,
with a `dtype` switch (np.float64 | np.longdouble) that covers every sum.  The inputs are always read as float64 values (an
fp32 feature is widened first), so the two runs differ by the rounding of the arithmetic alone; the distance between them is
what the GPU tests take their bars from."""
import numpy as np

EPS10 = 10 * np.finfo(np.float64).eps


def _a(v, dtype):
    return np.asarray(v, dtype=np.float64).astype(dtype)


def prepare(w, mu, v, dtype=np.float64):
    """(P [C, 2D], g [C])."""
    w, mu, v = _a(w, dtype), _a(mu, dtype), _a(v, dtype)
    D = mu.shape[1]
    P = np.concatenate([mu / v, dtype(-0.5) / v], axis=1)
    log_2pi = np.log(dtype(2) * np.arccos(dtype(-1)))
    with np.errstate(divide="ignore"):
        g = np.log(w) - dtype(0.5) * (dtype(D) * log_2pi + np.log(v).sum(axis=1) + (mu * mu / v).sum(axis=1))
    return P, g


def frame_rows(utt_first, utt_count):
    """(rows [n_total], utt [n_total]): the row and the utterance of every frame, utterance after utterance."""
    rows = [np.arange(a, a + n, dtype=np.int64) for a, n in zip(utt_first, utt_count)]
    utt = [np.full(n, u, dtype=np.int64) for u, n in enumerate(utt_count)]
    return (np.concatenate(rows) if rows else np.zeros(0, np.int64)), (np.concatenate(utt) if utt else np.zeros(0, np.int64))


def loglik(x, w, mu, v, utt_first=None, utt_count=None, dtype=np.float64):
    """dict: lse [n_total] (as computed, also for bad frames), good [n_total], gamma [n_total, C] (zeros for bad frames),
    utt_llsum [U], utt_frames [U], n_bad, X [n_total, D] (the frames, zeros for bad ones)."""
    x = np.asarray(x)
    if utt_first is None:
        utt_first, utt_count = [0], [x.shape[0]]
    rows, utt = frame_rows(utt_first, utt_count)
    U = len(utt_first)
    X = x[rows].astype(np.float64).astype(dtype)
    P, g = prepare(w, mu, v, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        ll = np.concatenate([X, X * X], axis=1) @ P.T + g[None, :]
        m = ll.max(axis=1) if ll.shape[0] else np.zeros(0, dtype)
        ms = np.where(np.isfinite(m), m, 0)
        lse = ms + np.log(np.exp(ll - ms[:, None]).sum(axis=1))
        lse = np.where(np.isnan(ll).any(axis=1), np.nan, lse)
    good = np.isfinite(lse)
    with np.errstate(invalid="ignore", over="ignore"):
        gamma = np.where(good[:, None], np.exp(ll - np.where(good, lse, 0)[:, None]), 0)
    Xg = np.where(good[:, None], X, 0)
    llsum = np.array([lse[good & (utt == u)].sum() for u in range(U)], dtype=dtype)
    frames = np.array([(good & (utt == u)).sum() for u in range(U)], dtype=np.int64)
    return dict(lse=lse, good=good, gamma=gamma, utt_llsum=llsum, utt_frames=frames, n_bad=int((~good).sum()), X=Xg, utt=utt)


def accumulate(x, w, mu, v, utt_first=None, utt_count=None, per_utt=False, dtype=np.float64):
    """Global form: dict n [C], f [C, D], s [C, D], llsum, n_frames, n_bad.  Per utterance: n [U, C], f [U, C, D], llsum [U],
    n_frames [U], n_bad."""
    r = loglik(x, w, mu, v, utt_first, utt_count, dtype)
    gam, X = r["gamma"], r["X"]
    if not per_utt:
        return dict(n=gam.sum(axis=0), f=gam.T @ X, s=gam.T @ (X * X), llsum=r["utt_llsum"].sum(), n_frames=int(r["utt_frames"].sum()),
                    n_bad=r["n_bad"])
    U = len(r["utt_frames"])
    sel = [r["utt"] == u for u in range(U)]
    n = np.stack([gam[k].sum(axis=0) for k in sel])
    f = np.stack([gam[k].T @ X[k] for k in sel])
    return dict(n=n, f=f, llsum=r["utt_llsum"], n_frames=r["utt_frames"], n_bad=r["n_bad"])


def mstep(n, f, s, n_frames, mu_old, v_old, reg_covar=1e-6, var_floor=0.0, min_count=0.0, dtype=np.float64):
    """(w, mu, v): scikit-learn's _estimate_gaussian_parameters for 'diag' and the renormalisation of _m_step."""
    n, f, s = _a(n, dtype), _a(f, dtype), _a(s, dtype)
    nk = n + dtype(EPS10)
    w = nk / dtype(n_frames)
    w = w / w.sum()
    mu = f / nk[:, None]
    v = s / nk[:, None] - mu * mu + dtype(reg_covar)
    v = np.maximum(v, dtype(var_floor))
    keep = n < dtype(min_count)
    mu = np.where(keep[:, None], _a(mu_old, dtype), mu)
    v = np.where(keep[:, None], _a(v_old, dtype), v)
    return w, mu, v


def em(x, w, mu, v, max_iter, tol=0.0, utt_first=None, utt_count=None, reg_covar=1e-6, var_floor=0.0, min_count=0.0, dtype=np.float64):
    """(w, mu, v, lower_bounds [n_iter], n_iter): the parameters are rounded to float64 between the iterations, as the device
    holds them."""
    lbs, prev = [], -np.inf
    for _ in range(max_iter):
        st = accumulate(x, w, mu, v, utt_first, utt_count, False, dtype)
        w, mu, v = mstep(st["n"], st["f"], st["s"], st["n_frames"], mu, v, reg_covar, var_floor, min_count, dtype)
        lb = st["llsum"] / dtype(st["n_frames"])
        lbs.append(lb)
        if abs(lb - prev) < tol:
            break
        prev = lb
    return w, mu, v, np.array(lbs, dtype=dtype), len(lbs)


def map_means(n, f, mu, relevance=16.0, dtype=np.float64):
    """[M, C, D]; n = 0 gives mu exactly."""
    n, f, mu = _a(n, dtype), _a(f, dtype), _a(mu, dtype)
    pos = n > 0
    ns = np.where(pos, n, 1)
    alpha = ns / (ns + dtype(relevance))
    hat = alpha[:, :, None] * (f / ns[:, :, None]) + (1 - alpha)[:, :, None] * mu[None]
    return np.where(pos[:, :, None], hat, mu[None])


def linear_scores(mu_hat, n, f, mu, v, dtype=np.float64):
    """[M, U]; a test row without frames scores 0."""
    mu_hat, n, f, mu, v = _a(mu_hat, dtype), _a(n, dtype), _a(f, dtype), _a(mu, dtype), _a(v, dtype)
    M, U = mu_hat.shape[0], n.shape[0]
    model = ((mu_hat - mu[None]) / v[None]).reshape(M, -1)
    tot = n.sum(axis=1)
    ts = np.where(tot > 0, tot, 1)
    test = ((f - n[:, :, None] * mu[None]) / ts[:, None, None]).reshape(U, -1)
    test = np.where((tot > 0)[:, None], test, 0)
    return model @ test.T


def llr(x, w, mu, v, mu_hat, utt_first=None, utt_count=None, dtype=np.float64):
    """[M, U]: the exact average LLR per good frame of every adapted model against the UBM."""
    base = loglik(x, w, mu, v, utt_first, utt_count, dtype)
    out = []
    for m in range(len(mu_hat)):
        r = loglik(x, w, mu_hat[m], v, utt_first, utt_count, dtype)
        out.append((r["utt_llsum"] - base["utt_llsum"]) / base["utt_frames"].astype(dtype))
    return np.stack(out)


def plan(n_total, C, D, n_utts=1, per_utt=False, n_slices=0):
    """csrc/gmm_plan.h restated: what xvec_gmm_plan_host reports."""
    up = lambda a, b: -(-a // b)
    ctiles = up(C, 64)
    ytiles = up(1 + D if per_utt else 1 + 2 * D, 64)
    if per_utt:
        slices, per = 0, 0
    else:
        slices = n_slices or max(1, min(1024 // (ctiles * up(1 + 2 * D, 64)), up(n_total, 1024), 1024))
        per = up(up(n_total, slices), 64) * 64 or 64
    kp = up(2 * D, 4) * 4
    return dict(frame_tile=64, comp_tile=64, comp_tiles=ctiles, col_tiles=ytiles, slices=slices, slice_frames=per, k_pad=kp,
                k_chunks=up(kp, 16), slab_doubles=slices * ctiles * ytiles * 4096, blocks=(n_utts if per_utt else slices) * ctiles * ytiles)
