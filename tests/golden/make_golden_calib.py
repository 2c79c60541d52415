"""Writes tests/golden/g12_calib.npz from scipy and scikit-learn themselves (1.15.3 and 1.7.2 when the committed file was made):
2000 overlapping target and non-target scores on a PLDA-like scale (mean around -40, spread around 30, a tenth of them on a
grid of 0.5 so that there are exact ties), the minimiser of the prior-weighted logistic objective of include/xvec_calib.h at
p_target = 0.5 and 0.01 from scipy.optimize.minimize with the gradient it stopped at, and sklearn's isotonic regression of the
target bit against the fp32-rounded scores.  Needs scipy and scikit-learn; the tests need only the file.

    python tests/golden/make_golden_calib.py
"""
import os

import numpy as np
import scipy
import sklearn
from scipy.optimize import minimize
from scipy.special import expit
from sklearn.isotonic import IsotonicRegression

N_TARGET, N_NONTARGET = 600, 1400


def objective(ab, s, tgt, p):
    """J, its gradient and its Hessian at (a, b) in float64."""
    x = ab[0] * s + ab[1] + np.log(p / (1 - p))
    u = np.where(tgt, -x, x)
    w = np.where(tgt, p / tgt.sum(), (1 - p) / (~tgt).sum())
    j = (w * np.logaddexp(0.0, u)).sum()
    dj = np.where(tgt, -1.0, 1.0) * w * expit(u)
    h = w * expit(u) * expit(-u)
    grad = np.array([(dj * s).sum(), dj.sum()])
    hess = np.array([[(h * s * s).sum(), (h * s).sum()], [(h * s).sum(), h.sum()]])
    return j, grad, hess


def main():
    rng = np.random.default_rng(12)
    s = np.concatenate([rng.normal(-22.0, 24.0, N_TARGET), rng.normal(-50.0, 27.0, N_NONTARGET)])
    tgt = np.concatenate([np.ones(N_TARGET, bool), np.zeros(N_NONTARGET, bool)])
    order = rng.permutation(len(s))
    s, tgt = s[order], tgt[order]
    ties = rng.random(len(s)) < 0.1
    s[ties] = np.round(s[ties] * 2) / 2
    out = {"scipy_version": np.array(scipy.__version__), "sklearn_version": np.array(sklearn.__version__), "scores": s,
           "is_target": tgt.astype(np.uint8)}
    for name, p in (("05", 0.5), ("001", 0.01)):
        res = minimize(lambda ab: objective(ab, s, tgt, p)[0], np.array([0.05, 1.0]), jac=lambda ab: objective(ab, s, tgt, p)[1],
                       hess=lambda ab: objective(ab, s, tgt, p)[2], method="trust-exact", options={"gtol": 1e-14})
        grad = objective(res.x, s, tgt, p)[1]
        print(f"p_target {p}: a, b = {res.x}, J = {res.fun}, |grad| = {np.abs(grad).max():.3e}, {res.message}")
        out[f"ab_{name}"] = res.x
        out[f"grad_{name}"] = grad
    s32 = s.astype(np.float32)
    # (the rounded scores held as float64: sklearn computes in the dtype of X)
    out["isotonic"] = IsotonicRegression(increasing=True).fit_transform(s32.astype(np.float64), tgt.astype(np.float64))      # in trial order
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g12_calib.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", int((np.unique(s32, return_counts=True)[1] > 1).sum()), "tie groups")


if __name__ == "__main__":
    main()
