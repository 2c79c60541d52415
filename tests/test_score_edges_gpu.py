"""The scoring back end (csrc/score.hip) at its tile boundaries, through the C ABI, every element against np.longdouble.

Reference.  The kernels' own formulas in np.longdouble on the operands the kernels are given (so the host algebra that derives
them, pinned by tests/test_scoring.py, is not part of what is compared):
  dense     e = x - mean;  s = scaling (e Psi t' + 0.5 e Phi e' + 0.5 t Phi t' + cst)
  low rank  y = (x - mean) L;  s = scaling ((y_e W) y_t' + 0.5 y_e (-Z) y_e' + 0.5 y_t (-Z) y_t' + cst), L, W, Z of scoring.plda_lowrank
  cosine    s = <a / |a|, b / |b|>, a zero row normalised to zero

Bar, per element: |got - ref| <= gamma S.  S is the sum of the absolute values of every elementary term that enters the
element -- sum |e_k| |Psi_kl| |t_l|, the two halves 0.5 sum |e_k| |Phi_kl| |e_l| and |cst|, times |scaling| (the chains
|e| |L| |W| |L'| |t'| and |e| |L| |Z| |L'| |e'| in the low-rank form, sum |a_k| |b_k| / (|a| |b|) for the cosine) -- and
gamma = (n_ops + 2) 2^-53, n_ops the largest number of roundings one elementary term passes through in the kernels (every
rounding multiplies the term by (1 + d), |d| <= 2^-53; n of them by at most 1 + n 2^-53 / (1 - n 2^-53); the 2 on top pays
for that denominator and for the reference's own 2^-64 roundings).  Counted in csrc/score.hip:
  centring          1 per vector (x - mean while the chunk is staged); a quadratic form holds the same vector twice: 2 either way
  a product         K: one fused multiply-add per k in the MFMA accumulation over the 16-wide K chunks (zero padding adds none)
  a row dot         2 (one fma per column block of the lane) + 4 (the shuffle sum of a 16-lane group) + parts - 1 (the sum
                    of the row's partials in the score product's epilogue); the factor 0.5 is exact
  epilogue          3 additions (row term, column term, constant) and the scaling: 4
  dense     cross term 2 + dim + dim + 4;  quadratic term 2 + dim + 6 + parts - 1 + 4        n_ops = the larger
  low rank  cross term 2 + 2 dim + 2 rank + 4;  quadratic term 2 + 2 dim + rank + 6 + parts - 1 + 4
  cosine    per row: ceil(dim / 64) fmas and 6 shuffle additions for |a|^2, 2 for the square root (the device's expansion is
            good to one ulp, not half), the reciprocal, the product: ceil(dim / 64) + 10; two rows, dim for the product, 4
parts = ceil(N / 32) - dot_col0 / 32 of the prelude launch (gemm_nt): N = 2 dim, dot_col0 = dim for the stacked [Psi ; Phi]
and the [W ; -Z] products, N = dim, dot_col0 = 0 where the quadratic form has a product of its own.
Every case prints its largest error / bound; profiles/backend_edges.txt holds the figures of one run.

Cases: the two-product branch of xvec_plda_score (psi_t and phi_t in separate buffers) against the stacked call; the stacked
dense and low-rank forms at dims and ranks around a wave's 32 columns and the 64-wide tile; the symmetric tile walk at
its band edges (T = 1, 2, 8, 9, 16, 17, 18 tiles) on NaN-filled outputs; the persistent loop of the symmetric walk on both
tile sizes (asserted through tests/score_support.py's restatement of the tile-size rule, on the device the test runs on);
cosine at dims below, at and beside the 64 lanes of its row loop with zero rows; every scorer inside a workspace window of
exactly the reported size.  Every call runs twice and must give the same bits."""
import numpy as np
import pytest
import torch

import plda_oracle as po
import score_support as ss

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -53
LD = np.longdouble
DIMS = [25, 31, 32, 33, 63, 64, 65, 96, 200]
NAN = float("nan")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _need_form(M, N, K, sym, want, persistent=None):
    """The score product of this shape must take the tile form the case is about on this device, or the case is skipped."""
    cus = _cus()
    got = ss.gemm_tile_size(M, N, K, sym, False, cus)
    if got != want:
        pytest.skip(f"{cus} CUs send the {M} x {N}, K = {K} product to {got} x {got} tiles, the case is about {want} x {want}")
    if persistent is not None and ss.is_persistent(M, N, K, sym, cus) != persistent:
        pytest.skip(f"{cus} CUs: the {M} x {N} product {'does not walk' if persistent else 'walks'} more than one tile per block")


def _xvecs(n, dim, seed, mean=None):
    x = np.random.default_rng(seed).normal(0, 1, (n, dim))
    return x if mean is None else x + mean


class Model:
    """A PLDA model with the operands of both forms on the device: [Psi^T ; Phi^T] stacked AND in two buffers of their own."""

    def __init__(self, dim, rank, scaling=1.0, seed=0):
        from xvector_amd import scoring
        self.dim, self.rank, self.scale = dim, rank, float(scaling)
        self.mean, F, Sigma = po.make_plda(dim, rank, seed=1000 * dim + rank + seed)
        self.phi, self.psi, self.cst = scoring.plda_constants(F, Sigma, scaling)
        self.L, self.W, self.Z, _ = scoring.plda_lowrank(F, Sigma, scaling)
        self.mean_d = _dev(self.mean)
        self.stacked_d = _dev(np.concatenate([self.psi.T, self.phi.T], 0))
        self.phi_t_d, self.psi_t_d, self._spare = _dev(self.phi.T), _dev(self.psi.T), []
        while self.phi_t_d.data_ptr() == self.psi_t_d.data_ptr() + 8 * dim * dim:       # two buffers that happen to touch
            self._spare.append(self.phi_t_d)
            self.phi_t_d = _dev(self.phi.T)
        self.l_t_d = _dev(self.L.T)
        self.wz_t_d = _dev(np.concatenate([self.W.T, -self.Z.T], 0))

    def parts(self, kind, separate=False):
        """The largest count of row-dot partials a quadratic term of this form is summed from."""
        if kind == "dense":
            return -(-self.dim // 32) if separate else max(-(-2 * self.dim // 32) - self.dim // 32, -(-self.dim // 32))
        return max(-(-2 * self.rank // 32) - self.rank // 32, -(-self.rank // 32))

    def n_ops(self, kind, separate=False):
        d, r, p = self.dim, self.rank, self.parts(kind, separate)
        if kind == "dense":
            return max(2 + d + d + 4, 2 + d + 6 + p - 1 + 4)
        return max(2 + 2 * d + 2 * r + 4, 2 + 2 * d + r + 6 + p - 1 + 4)


def cosine_n_ops(dim):
    return 2 * (-(-dim // 64) + 10) + dim + 4


# ---------------------------------------------------------------- references (np.longdouble) and the sums S (float64)

def _quad(A, M):
    return np.einsum("ik,ik->i", A @ M, A)


def ref_dense(m, e, t=None):
    E = e.astype(LD) - m.mean.astype(LD)
    T = E if t is None else t.astype(LD) - m.mean.astype(LD)
    psi, phi = m.psi.astype(LD), m.phi.astype(LD)
    ref = LD(m.scale) * ((E @ psi) @ T.T + 0.5 * _quad(E, phi)[:, None] + 0.5 * _quad(T, phi)[None, :] + LD(m.cst))
    Ea, Ta, psia, phia = (np.abs(v).astype(np.float64) for v in (E, T, psi, phi))
    S = abs(m.scale) * ((Ea @ psia) @ Ta.T + 0.5 * _quad(Ea, phia)[:, None] + 0.5 * _quad(Ta, phia)[None, :] + abs(m.cst))
    return ref, S


def ref_lowrank(m, e, t=None):
    L, W, Zn = m.L.astype(LD), m.W.astype(LD), -m.Z.astype(LD)
    Ye = (e.astype(LD) - m.mean.astype(LD)) @ L
    Yt = Ye if t is None else (t.astype(LD) - m.mean.astype(LD)) @ L
    ref = LD(m.scale) * ((Ye @ W) @ Yt.T + 0.5 * _quad(Ye, Zn)[:, None] + 0.5 * _quad(Yt, Zn)[None, :] + LD(m.cst))
    La, Wa, Za = np.abs(m.L), np.abs(m.W), np.abs(m.Z)
    Ya = np.abs(e - m.mean) @ La
    Yta = Ya if t is None else np.abs(t - m.mean) @ La
    S = abs(m.scale) * ((Ya @ Wa) @ Yta.T + 0.5 * _quad(Ya, Za)[:, None] + 0.5 * _quad(Yta, Za)[None, :] + abs(m.cst))
    return ref, S


def _unit_rows(x, dtype):
    x = x.astype(dtype)
    norm = np.sqrt((x * x).sum(1, keepdims=True))
    return np.divide(x, norm, out=np.zeros_like(x), where=norm > 0)


def ref_cosine(e, t=None, dtype=LD, rows=None):
    A = _unit_rows(e, dtype)
    B = A if t is None else _unit_rows(t, dtype)
    if rows is not None:
        A = A[rows]
    return A @ B.T, np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64).T


# ---------------------------------------------------------------- the calls

def call(kind, m, e_d, t_d=None, separate=False, ws=None):
    """One scorer through the C ABI on a NaN-filled output: (return code, scores).  ws = (pointer, bytes) or an ample
    0xFF-filled buffer."""
    from xvector_amd import hip
    ne, dim = e_d.shape
    nt = ne if t_d is None else t_d.shape[0]
    if ws is None:
        need = int(hip.lib.xvec_score_workspace_bytes(ne, 0 if t_d is None else nt, dim))
        assert need > 0
        buf = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device=DEV)
        ws = (buf.data_ptr(), buf.numel())
    out = torch.full((ne, nt), NAN, dtype=torch.float64, device=DEV)
    tp = None if t_d is None else t_d.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    if kind == "dense":
        psi = m.psi_t_d.data_ptr() if separate else m.stacked_d.data_ptr()
        phi = m.phi_t_d.data_ptr() if separate else psi + 8 * dim * dim
        assert (phi != psi + 8 * dim * dim) == separate
        rc = hip.lib.xvec_plda_score(e_d.data_ptr(), ne, tp, nt, dim, m.mean_d.data_ptr(), psi, phi, m.cst, m.scale,
                                     out.data_ptr(), ws[0], ws[1], stream)
    elif kind == "lowrank":
        rc = hip.lib.xvec_plda_score_lowrank(e_d.data_ptr(), ne, tp, nt, dim, m.rank, m.mean_d.data_ptr(), m.l_t_d.data_ptr(),
                                             m.wz_t_d.data_ptr(), m.cst, m.scale, out.data_ptr(), ws[0], ws[1], stream)
    else:
        rc = hip.lib.xvec_cosine_score(e_d.data_ptr(), ne, tp, nt, dim, out.data_ptr(), ws[0], ws[1], stream)
    torch.cuda.synchronize()
    return rc, out


def scores(kind, m, e_d, t_d=None, separate=False):
    """The scores as numpy; the call runs twice and must give the same bits."""
    from xvector_amd import hip
    rc, out = call(kind, m, e_d, t_d, separate)
    assert rc == 0, hip.lib.xvec_score_last_error()
    rc2, again = call(kind, m, e_d, t_d, separate)
    assert rc2 == 0 and torch.equal(out.view(torch.int64), again.view(torch.int64)), f"{kind}: a repeated call differs"
    return out.cpu().numpy()


def inside(got, ref, S, n_ops, what):
    """Every element inside (n_ops + 2) 2^-53 S; prints and returns (bound, largest error / bound)."""
    assert got.shape == ref.shape == S.shape
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} elements were never written"
    bound = (n_ops + 2) * U * S
    err = np.abs(got - ref).astype(np.float64)
    bad = err > bound
    np.divide(err, bound, out=err, where=bound > 0)          # (bound = 0: a zero row of the cosine; any error there is in `bad`)
    ratio = float(err.max())
    print(f"score edges {what}: largest error / bound = {ratio:.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the bound, largest error / bound {ratio:.3f}, first at {np.argwhere(bad)[0]}"
    return bound


def reference(kind, m, e, t=None):
    return ref_dense(m, e, t) if kind == "dense" else ref_lowrank(m, e, t) if kind == "lowrank" else ref_cosine(e, t)


def n_ops_of(kind, m, dim, separate=False):
    return cosine_n_ops(dim) if kind == "cosine" else m.n_ops(kind, separate)


# ---------------------------------------------------------------- psi_t and phi_t in buffers of their own

@pytest.mark.parametrize("dim", DIMS)
def test_separate_psi_and_phi_buffers(dim):
    """xvec_plda_score's two-product branch (phi_t != psi_t + dim dim): e Psi stored by one prelude launch, the row dots of
    e Phi written over the other half of the row by a second; self and two sets, against the reference and the stacked call."""
    m = Model(dim, max(1, dim // 3), scaling=0.5 if dim % 2 else 1.0)
    e, t = _xvecs(65, dim, dim, m.mean), _xvecs(129, dim, dim + 1, m.mean)
    e_d, t_d = _dev(e), _dev(t)
    for what, td, th in (("two sets", t_d, t), ("self", None, None)):
        ref, S = ref_dense(m, e, th)
        sep = scores("dense", m, e_d, td, separate=True)
        bound = inside(sep, ref, S, m.n_ops("dense", True), f"dense, separate buffers, dim {dim}, {what}")
        stacked = scores("dense", m, e_d, td)
        inside(stacked, ref, S, m.n_ops("dense"), f"dense, stacked, dim {dim}, {what}")
        assert (np.abs(sep - stacked) <= 2 * bound).all()
        if td is None:
            assert np.array_equal(sep, sep.T) and np.array_equal(stacked, stacked.T)


# ---------------------------------------------------------------- stacked dense and low-rank forms

@pytest.mark.parametrize("dim", DIMS)
def test_dense_and_lowrank_forms_around_the_wave_and_tile_widths(dim):
    """ranks 1, 31, 32, 33 and dim (the row-dot slots of the [W ; -Z] product straddle a wave's 32 columns at 31 and 33);
    sizes under, at and over one 64 x 64 tile; scaling factor 0.5 at the odd ranks, 1 at the even ones."""
    for rank in sorted({r for r in (1, 31, 32, 33, dim) if r <= dim}):
        for scaling in ((0.5,) if rank % 2 else (1.0,)):
            m = Model(dim, rank, scaling)
            for ne, nt in ((1, 1), (63, 65), (64, 64), (65, 129)):
                e, t = _xvecs(ne, dim, ne + rank, m.mean), _xvecs(nt, dim, nt + rank + 7, m.mean)
                e_d, t_d = _dev(e), _dev(t)
                for kind in ("dense", "lowrank"):
                    what = f"{kind}, dim {dim}, rank {rank}, scaling {scaling}, {ne} x {nt}"
                    inside(scores(kind, m, e_d, t_d), *reference(kind, m, e, t), m.n_ops(kind), what)
                    own = scores(kind, m, e_d)
                    inside(own, *reference(kind, m, e), m.n_ops(kind), what + " self")
                    assert np.array_equal(own, own.T)


# ---------------------------------------------------------------- the symmetric walk at its band edges

@pytest.mark.parametrize("dim", [24, 25])
@pytest.mark.parametrize("n", [64, 65, 449, 512, 513, 1024, 1025, 1089])
def test_symmetric_walk_at_band_edges(n, dim):
    """T = 1, 2, 8, 8, 9, 16, 17, 18 tiles of 64: a lone diagonal tile, a full band, a band of one row tile, two full bands and
    what follows them.  The output is NaN before the call: a tile the walk misses cannot pass.  dim 24 / rank 16 take the
    16-byte loads, dim 25 / rank 17 the 8-byte ones."""
    m = Model(dim, dim - 8, scaling=0.5 if n % 2 else 1.0)
    e = _xvecs(n, dim, n + dim, m.mean)
    e_d, copy_d = _dev(e), _dev(e)
    for kind in ("dense", "lowrank", "cosine"):
        K = m.rank if kind == "lowrank" else dim
        _need_form(n, n, K, True, 64)
        what = f"{kind}, symmetric walk, n {n}, dim {dim}"
        own = scores(kind, m, e_d)
        bound = inside(own, *reference(kind, m, e), n_ops_of(kind, m, dim), what)
        assert np.array_equal(own, own.T)
        two = scores(kind, m, e_d, copy_d)
        assert (np.abs(two - own) <= 2 * bound).all(), f"{what}: the two-set call on the same vectors differs"


# ---------------------------------------------------------------- the persistent loop of the symmetric walk

@pytest.mark.parametrize("kind", ["cosine", "lowrank"])
def test_persistent_symmetric_walk_on_64_tiles(kind):
    """The smallest n whose upper triangle of 64 x 64 tiles exceeds the 4 blocks per CU (n = 2817 on 256 CUs): every block
    slot's second tile goes through the `more` branch (prefetch under the epilogue, sums in the reused LDS buffer)."""
    slots, T = 4 * _cus(), 1
    while T * (T + 1) // 2 <= slots:
        T += 1
    n, dim = 64 * (T - 1) + 1, 24
    m = Model(dim, 16)
    _need_form(n, n, m.rank if kind == "lowrank" else dim, True, 64, persistent=True)
    e = _xvecs(n, dim, n, m.mean)
    own = scores(kind, m, _dev(e))
    inside(own, *reference(kind, m, e), n_ops_of(kind, m, dim), f"{kind}, persistent symmetric walk, n {n}, dim {dim}")
    assert np.array_equal(own, own.T)


def test_persistent_symmetric_walk_on_128_tiles():
    """n = 5600, K = 258, cosine: 990 tiles of 128 x 128 on two blocks per CU.  The whole matrix against numpy float64 inside
    the same bound, 200 sampled rows against np.longdouble."""
    n, dim = 5600, 258
    _need_form(n, n, dim, True, 128, persistent=True)
    e = _xvecs(n, dim, 5600)
    own = scores("cosine", None, _dev(e))
    inside(own, *ref_cosine(e, dtype=np.float64), cosine_n_ops(dim), "cosine, 128 x 128 symmetric walk, n 5600, K 258 (float64 reference)")
    assert np.array_equal(own, own.T)
    rows = np.sort(np.random.default_rng(1).choice(n, 200, replace=False))
    rows[0], rows[-1] = 0, n - 1
    inside(own[rows], *ref_cosine(e, rows=rows), cosine_n_ops(dim), "cosine, 128 x 128 symmetric walk, 200 rows (longdouble reference)")


# ---------------------------------------------------------------- cosine

@pytest.mark.parametrize("dim", [1, 2, 25, 63, 64, 65, 130])
def test_cosine_dims_and_zero_rows(dim):
    """The row loop of normalize_rows_kernel strides by 64 lanes: dims under, at and over one and two strides, odd dims (the
    8-byte loads of the product).  One all-zero row in each set: its scores are exactly 0.0 and nothing is NaN."""
    e, t = _xvecs(65, dim, dim), _xvecs(129, dim, dim + 50)
    e[17], t[100] = 0.0, 0.0
    e_d, t_d = _dev(e), _dev(t)
    got = scores("cosine", None, e_d, t_d)
    inside(got, *ref_cosine(e, t), cosine_n_ops(dim), f"cosine, dim {dim}, 65 x 129")
    assert not got[17].any() and not got[:, 100].any() and not np.signbit(got[17]).any() and not np.signbit(got[:, 100]).any()
    own = scores("cosine", None, e_d)
    inside(own, *ref_cosine(e), cosine_n_ops(dim), f"cosine, dim {dim}, 65 self")
    assert np.array_equal(own, own.T) and not own[17].any() and not own[:, 17].any()


@pytest.mark.parametrize("dim", [1, 2, 25, 63, 64, 65, 130])
def test_cosine_self_diagonal_within_one_ulp_of_one(dim):
    """The diagonal of a self call within 2^-52 of 1 for the non-zero rows, 0.0 for the zero row.  The product of the rounded
    unit rows alone misses this bar from dim 2 on: it carries twice the relative error of 1 / |a| plus the roundings of dim
    fused multiply-adds.  Largest |diagonal - 1| over 64 rows of the two-set call on the same vectors, which still takes its
    diagonal from the product (MI355X, in units of 2^-52; numpy float64 gives the same 2.0 ... 4.5):
        dim      1     2     25    63    64    65    130
                 1.00  2.00  2.00  2.50  2.50  3.00  4.50
    The self call therefore writes the exact 1.0 over every positive diagonal element (unit_diagonal_kernel of csrc/score.hip),
    which is inside this file's bound of the product as well; the two-set figure is printed beside it."""
    e = _xvecs(65, dim, dim)
    e[17] = 0.0
    e_d = _dev(e)
    own = scores("cosine", None, e_d)
    keep = np.arange(65) != 17
    worst = float(np.abs(np.diag(own)[keep] - 1.0).max())
    two = float(np.abs(np.diag(scores("cosine", None, e_d, _dev(e)))[keep] - 1.0).max())
    print(f"score edges cosine, dim {dim}: largest |diagonal - 1| = {worst / 2.0 ** -52:.2f} x 2^-52 (two sets: {two / 2.0 ** -52:.2f})")
    assert worst <= 2.0 ** -52
    assert own[17, 17] == 0.0 and not np.signbit(own[17, 17])


# ---------------------------------------------------------------- workspace

@pytest.mark.parametrize("kind", ["dense", "lowrank", "cosine"])
@pytest.mark.parametrize("two_sets", [False, True])
def test_workspace_window_of_exactly_the_reported_size(kind, two_sets):
    """The call inside a 0xFF-filled window of xvec_score_workspace_bytes bytes cut from a guarded buffer: the guards stay, the
    scores are those of a call with room to spare; one byte less is refused before anything is launched."""
    from xvector_amd import hip
    dim = 33
    m = Model(dim, 17, scaling=0.5)
    e_d = _dev(_xvecs(65, dim, 1, m.mean))
    t_d = _dev(_xvecs(129, dim, 2, m.mean)) if two_sets else None
    need = int(hip.lib.xvec_score_workspace_bytes(65, 129 if two_sets else 0, dim))
    assert need > 0
    ample = scores(kind, m, e_d, t_d)
    big, off = ss.window(need, DEV)
    rc, out = call(kind, m, e_d, t_d, ws=(big.data_ptr() + off, need))
    assert rc == 0, hip.lib.xvec_score_last_error()
    assert ss.guards_intact(big, off, need)
    assert np.array_equal(out.cpu().numpy(), ample)
    big, off = ss.window(need, DEV)
    rc, out = call(kind, m, e_d, t_d, ws=(big.data_ptr() + off, need - 1))
    assert rc == hip.ERR_WORKSPACE and b"workspace too small" in hip.lib.xvec_score_last_error()
    assert bool(torch.isnan(out).all()), "a refused call wrote scores"
    assert bool((big[off:off + need] == 0xFF).all()) and ss.guards_intact(big, off, need), "a refused call touched its workspace"
