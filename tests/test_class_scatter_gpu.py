"""xvec_plda_stats and xvec_lda_stats run the same statistics kernels (csrc/class_scatter.h): on an input where the two calls
ask for the same numbers they must return the same bits.

n = 32 float64 rows, every row its own class.  Both class sums are x exactly and both means come from the same walk over them;
LDA's class means are x / 1, so its within-class rows centre to exactly zero and its between-class product is over the rows of
x centred by the mean -- PLDA's sigma_obs times n.  Both slice plans give one slice of 32 rows (32 <= 32 for LDA, 32 <= 256 for
PLDA); LDA's weight 1.0 makes its A image equal its B image, so PLDA's single-operand diagonal tile (PER_ROW = false) feeds the
MFMAs the operands LDA's two images (PER_ROW = true) do; the division by 32 and the multiplication back are exact.  dim = 64
stages by 16-byte loads and has the diagonal tile alone; dim = 65 stages element by element and adds an off-diagonal tile
and a diagonal tile one column wide."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("dim", [64, 65])
def test_plda_and_lda_statistics_agree_bit_for_bit(dim):
    from xvector_amd import lda, plda
    n = 32
    x = np.random.default_rng(dim).normal(1.0, 1.0, (n, dim))
    labels = np.arange(n)
    xt = torch.from_numpy(x).to(DEV)
    p = plda.PldaStats(xt, labels, scaling_factor=1.0)
    s = lda.LdaStats(xt, labels)
    print(f"dim {dim}: mean differs in {int((p.mean != s.mean).sum())} elements, sigma_obs * n from s_between in "
          f"{int((p.sigma_obs * n != s.s_between).sum())} (largest {np.abs(p.sigma_obs * n - s.s_between).max():.3e}), "
          f"largest |s_within| {np.abs(s.s_within).max():.3e}")
    assert np.array_equal(p.mean, s.mean)
    assert np.array_equal(p.sigma_obs * 32, s.s_between)
    assert not s.s_within.any()
