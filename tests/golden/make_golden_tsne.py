"""Writes tests/golden/g11_tsne.npz from scikit-learn itself (1.7.2 when the committed file was made): the pieces of
TSNE(method='exact') that include/xvec_tsne.h restates, on N = 65 points of D = 16 at perplexity 5, and the PCA the reference
plots.  Needs scikit-learn; the tests need only the file.

    python tests/golden/make_golden_tsne.py
"""
import os

import numpy as np
import sklearn
from scipy.spatial.distance import squareform
from sklearn.decomposition import PCA
from sklearn.manifold import _t_sne
from sklearn.metrics import pairwise_distances
from sklearn.preprocessing import StandardScaler

N, D, PERPLEXITY, EXAGGERATION, LEARNING_RATE, ITERS = 65, 16, 5.0, 12.0, 50.0, 10      # 'auto': max(65 / 12 / 4, 50) = 50


def descent(p0, P, momentum):
    """ITERS iterations of scikit-learn's _gradient_descent from p0 (its update starts at 0 and its gains at 1); the KL value
    is the one of the last iteration."""
    p, kl, it = _t_sne._gradient_descent(_t_sne._kl_divergence, p0.ravel().copy(), it=0, max_iter=ITERS, n_iter_check=ITERS,
                                         momentum=momentum, learning_rate=LEARNING_RATE, args=[P, 1.0, N, 2])
    assert it == ITERS - 1
    return p.reshape(N, 2), kl


def main():
    rng = np.random.default_rng(11)
    centres = 3.0 * rng.standard_normal((5, D))
    x = (centres[np.arange(N) % 5] + rng.standard_normal((N, D))).astype(np.float32)
    d2 = pairwise_distances(x.astype(np.float64), metric="euclidean", squared=True).astype(np.float32)
    P = _t_sne._joint_probabilities(d2, PERPLEXITY, 0)                       # condensed
    y_grad = rng.standard_normal((N, 2))
    kl, grad = _t_sne._kl_divergence(y_grad.ravel().copy(), P, 1.0, N, 2)
    y0 = 1e-4 * rng.standard_normal((N, 2))
    y1, kl1 = descent(y0, P * EXAGGERATION, 0.5)
    y2, kl2 = descent(y1, P, 0.8)
    x_pca = x.astype(np.float64)
    x_pca[:, 3] = 0.7                                                        # a constant column: StandardScaler leaves it alone
    pca = PCA(n_components=2).fit_transform(StandardScaler().fit_transform(x_pca))
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g11_tsne.npz")
    np.savez_compressed(out, sklearn_version=np.array(sklearn.__version__), x=x, d2=d2, perplexity=np.float64(PERPLEXITY),
                        P=squareform(P), y_grad=y_grad, kl=np.float64(kl), grad=grad.reshape(N, 2),
                        exaggeration=np.float64(EXAGGERATION), learning_rate=np.float64(LEARNING_RATE), y0=y0, y1=y1,
                        kl1=np.float64(kl1), y2=y2, kl2=np.float64(kl2), x_pca=x_pca, pca=pca)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
