"""Writes tests/golden/g13_gmm.npz from scikit-learn itself: GaussianMixture(covariance_type='diag', tol=0, max_iter=k,
weights_init, means_init, precisions_init) on N = 333, C = 5, D = 7 planted data -- score_samples and predict_proba of the
initial model, and the parameters and the lower bound after 1 and 10 iterations.  Run once where scikit-learn is installed:

    python tests/golden/make_golden_gmm.py

The tests read the fixture only."""
import os
import warnings

import numpy as np
import sklearn
from sklearn.mixture import GaussianMixture

N, C, D = 333, 5, 7


def planted(seed=13):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 3.0, (C, D))
    scales = rng.uniform(0.5, 1.5, (C, D))
    comp = rng.integers(0, C, N)
    x = centres[comp] + scales[comp] * rng.normal(size=(N, D))
    w0 = rng.uniform(0.5, 1.5, C)
    w0 /= w0.sum()
    mu0 = x[rng.choice(N, C, replace=False)] + 0.1 * rng.normal(size=(C, D))
    v0 = np.tile(x.var(axis=0), (C, 1)) * rng.uniform(0.8, 1.2, (C, D))
    return x, w0, mu0, v0


def fitted(x, w0, mu0, v0, k):
    gm = GaussianMixture(n_components=C, covariance_type="diag", tol=0.0, max_iter=k, reg_covar=1e-6, weights_init=w0, means_init=mu0,
                         precisions_init=1.0 / v0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (tol = 0 never "converges")
        gm.fit(x)
    return gm


def initial(w0, mu0, v0):
    """A GaussianMixture that holds the initial model without a fit."""
    gm = GaussianMixture(n_components=C, covariance_type="diag")
    gm.weights_, gm.means_, gm.covariances_ = w0, mu0, v0
    gm.precisions_cholesky_ = 1.0 / np.sqrt(v0)
    return gm


if __name__ == "__main__":
    x, w0, mu0, v0 = planted()
    g0, g1, g10 = initial(w0, mu0, v0), fitted(x, w0, mu0, v0, 1), fitted(x, w0, mu0, v0, 10)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g13_gmm.npz")
    np.savez(out, x=x, w0=w0, mu0=mu0, v0=v0, score_samples=g0.score_samples(x), predict_proba=g0.predict_proba(x),
             w1=g1.weights_, mu1=g1.means_, v1=g1.covariances_, lb1=np.float64(g1.lower_bound_),
             w10=g10.weights_, mu10=g10.means_, v10=g10.covariances_, lb10=np.float64(g10.lower_bound_),
             sklearn_version=np.array(sklearn.__version__))
    print("wrote", out, os.path.getsize(out), "bytes; scikit-learn", sklearn.__version__)
