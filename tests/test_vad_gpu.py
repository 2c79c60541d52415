"""Energy VAD, sliding CMVN and the selection of voiced frames on the device (csrc/vad.hip, include/xvec_vad.h) against the numpy
restatement tests/vad_ref.py, through the C ABI unless a test says otherwise.

Decisions (mask, counts, threshold) must be EQUAL: the header fixes the order of the energy sum, and both sides round every
operation on its own.

Normalised values are held to a bound derived here, not tuned.  The kernel forms the window sums of a run's first frame in
fp64, one addition after the other, and slides them over the run's other frames (the header's order): a frame's sum has been
through k operations -- the first window's additions, and an addition or a subtraction per row that entered or left since --
each rounding a partial sum of values of the rows between the first window's start and this window's end, so none larger than
their sum|x|: the result is off by at most k u sum|x| (u = 2^-53).  The tile and the run length come from vad_ref.tile_plan,
which tests/test_vad.py holds against csrc/vad_plan.h.  The quotient by n adds u |mean|, the difference x - mean adds
u |x - mean|: that is `bound` of vad_ref.sliding_cmvn for the mean alone.  With norm_vars the sum of squares (the squares of fp32 values are exact in fp64) is
off by k u sumsq (of the same rows), its quotient, the product mean * mean and their difference round once each, and the
mean's own error enters twice over (2 |mean| dmean + dmean^2): dvar.  The scale var^-1/2 then lies between the scales of var - dvar and var + dvar
(both floored like var itself), three more roundings (root, reciprocal, product) apart, and the product rule carries the two
errors into y.  vad_ref works in np.longdouble (u there counts its own rounding too) and does not round to fp32; the kernel
does, once: 2^-24 (|y| + bound), and 2^-149 where the result is subnormal.  Every element must lie inside
bound + 2^-24 (|y| + bound) + 2^-149.

Every call here passes strides larger than the extent, inputs whose padding and frames at or past the lengths are NaN, and
outputs filled with a sentinel: the padding must come back untouched (buffers exactly as large as the extent hide
writes past it)."""
import numpy as np
import pytest
import torch

import score_support as ss
import vad_ref
from conftest import assert_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
LANES, TILE = 256, 256          # XVEC_VAD_LANES; the tile of the plans of the values test (whole rows of 5 channels)
SENTINEL = -777.25
RECIPE = vad_ref.RECIPE_VAD


# ---------------------------------------------------------------- calls

def _stream():
    return torch.cuda.current_stream().cuda_stream


def _poisoned(x, lengths):
    """A copy of x [B, T, C] with NaN in every frame at or past its utterance's length."""
    x = np.array(x, dtype=np.float32)
    if lengths is not None:
        for b, L in enumerate(lengths):
            x[b, L:] = NAN
    return x


def _strided(host, rs, us):
    """(flat buffer, view [B, T, C] with row stride rs and utterance stride us): NaN everywhere outside the values."""
    B, T, C = host.shape
    flat = torch.full((B * us + 8,), NAN, dtype=torch.float32, device=DEV)
    view = flat.as_strided((B, T, C), (us, rs, 1))
    view.copy_(torch.from_numpy(host))
    return flat, view


def _lens(lengths):
    return None if lengths is None else torch.tensor([int(v) for v in lengths], dtype=torch.int32, device=DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Out:
    """Sentinel-filled outputs with strides larger than the extent; `check()` asserts the padding is untouched."""

    def __init__(self, B, T, C, yrs=None, yus=None, ms=None):
        self.B, self.T, self.C = B, T, C
        self.yrs = C + 2 if yrs is None else yrs
        self.yus = T * self.yrs + 3 if yus is None else yus
        self.ms = T + 7 if ms is None else ms
        self.y = torch.full((B * self.yus + 8,), SENTINEL, dtype=torch.float32, device=DEV)
        self.mask = torch.full((B * self.ms + 8,), 0xAB, dtype=torch.uint8, device=DEV)
        self.counts = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        self.new_len = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        self.thr = torch.full((B,), 7.5, dtype=torch.float64, device=DEV)

    def y_view(self):
        return self.y.as_strided((self.B, self.T, self.C), (self.yus, self.yrs, 1))

    def mask_view(self):
        return self.mask.as_strided((self.B, self.T), (self.ms, 1))

    def check(self, y=True, mask=True):
        if y:
            pad = self.y.clone()
            pad.as_strided((self.B, self.T, self.C), (self.yus, self.yrs, 1)).fill_(SENTINEL)
            assert bool((pad == SENTINEL).all()), "y: written outside the rows"
            assert not bool((self.y_view() == SENTINEL).any()), "y: an element was not written"
        if mask:
            pad = self.mask.clone()
            pad.as_strided((self.B, self.T), (self.ms, 1)).fill_(0xAB)
            assert bool((pad == 0xAB).all()), "mask: written outside the rows"
            assert bool((self.mask_view() <= 1).all()), "mask: an entry was not written"


def _vopt(opts):
    from xvector_amd import hip
    o = {**vad_ref.VAD_DEFAULTS, **opts}
    return hip.VadOptions(o["energy_threshold"], o["energy_mean_scale"], o["proportion_threshold"], o["frames_context"], o["energy_col"])


def _copt(opts):
    from xvector_amd import hip
    return None if opts is None else hip.CmvnOptions(opts["cmn_window"], opts["min_window"], int(opts["center"]), int(opts["norm_vars"]))


def _input(x, lengths, rs, us):
    B, T, C = x.shape
    rs = C + 3 if rs is None else rs
    us = T * rs + 5 if us is None else us
    flat, _ = _strided(_poisoned(x, lengths), rs, us)
    return flat, rs, us


def _energy(x, lengths=None, rs=None, us=None, **opts):
    """xvec_vad_energy -> (mask [B, T] uint8, counts, thr) as numpy."""
    from xvector_amd import hip
    B, T, C = x.shape
    flat, rs, us = _input(x, lengths, rs, us)
    out, lens = _Out(B, T, C), _lens(lengths)
    rc = hip.lib.xvec_vad_energy(flat.data_ptr(), B, T, C, rs, us, _ptr(lens), _vopt(opts), out.mask.data_ptr(), out.ms,
                                 out.counts.data_ptr(), out.thr.data_ptr(), _stream())
    assert rc == 0, hip.lib.xvec_vad_last_error()
    torch.cuda.synchronize()
    out.check(y=False)
    return out.mask_view().cpu().numpy(), out.counts.cpu().numpy(), out.thr.cpu().numpy()


def _workspace(B, T):
    from xvector_amd import hip
    need = int(hip.lib.xvec_vad_workspace_bytes(B, T))
    assert need > 0 and need % 256 == 0
    return torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV), need


def _cmvn(x, lengths=None, cmvn=None, mask=None, rs=None, us=None, yrs=None, yus=None):
    """xvec_cmvn_sliding -> (y [B, T, C] float32, new_lengths) as numpy.  mask: numpy [B, T] or None."""
    from xvector_amd import hip
    B, T, C = x.shape
    flat, rs, us = _input(x, lengths, rs, us)
    out, lens = _Out(B, T, C, yrs, yus), _lens(lengths)
    if mask is not None:
        out.mask_view().copy_(torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)))
    ws, need = _workspace(B, T)
    rc = hip.lib.xvec_cmvn_sliding(flat.data_ptr(), B, T, C, rs, us, _ptr(lens), _copt(cmvn), None if mask is None else out.mask.data_ptr(),
                                   out.ms, out.y.data_ptr(), out.yrs, out.yus, out.new_len.data_ptr(), ws.data_ptr(), need, _stream())
    assert rc == 0, hip.lib.xvec_vad_last_error()
    torch.cuda.synchronize()
    out.check(mask=False)
    return out.y_view().cpu().numpy(), out.new_len.cpu().numpy()


def _fused(x, lengths, vad, cmvn, select=1, ws=None, need=None):
    """xvec_vad_cmvn -> (mask, counts, thr, y, new_lengths) as numpy."""
    from xvector_amd import hip
    B, T, C = x.shape
    flat, rs, us = _input(x, lengths, None, None)
    out, lens = _Out(B, T, C), _lens(lengths)
    if ws is None:
        buf, need = _workspace(B, T)
        ws = buf.data_ptr()
    rc = hip.lib.xvec_vad_cmvn(flat.data_ptr(), B, T, C, rs, us, _ptr(lens), _vopt(vad), _copt(cmvn), select, out.mask.data_ptr(),
                               out.ms, out.counts.data_ptr(), out.thr.data_ptr(), out.y.data_ptr(), out.yrs, out.yus,
                               out.new_len.data_ptr(), ws, need, _stream())
    assert rc == 0, hip.lib.xvec_vad_last_error()
    torch.cuda.synchronize()
    out.check()
    return (out.mask_view().cpu().numpy(), out.counts.cpu().numpy(), out.thr.cpu().numpy(), out.y_view().cpu().numpy(),
            out.new_len.cpu().numpy())


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_decisions(got, x, lengths, what, **opts):
    ref = vad_ref.energy_vad(x, lengths, **opts)
    assert np.array_equal(got[0], ref[0]), (what, "mask", int((got[0] != ref[0]).sum()))
    assert np.array_equal(got[1], ref[1]), (what, "counts", got[1], ref[1])
    assert _same_bits(got[2], ref[2]) or np.array_equal(got[2], ref[2], equal_nan=True), (what, "thr", got[2], ref[2])


def _energies(B, T, C, seed, col=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    x[:, :, col] = rng.normal(10.0, 3.0, (B, T)).astype(np.float32)
    return x


# ---------------------------------------------------------------- VAD decisions, exact

@pytest.mark.parametrize("ctx", [0, 2, 7])
def test_decisions_equal_the_restatement_at_every_length(ctx):
    lengths = sorted({0, 1, 2, max(ctx, 1), ctx + 1, 2 * ctx + 1, LANES - 1, LANES, LANES + 1, 2 * LANES + 1})
    T = max(lengths)
    x = _energies(len(lengths), T, 3, seed=100 + ctx)
    opts = dict(RECIPE, frames_context=ctx)
    _assert_decisions(_energy(x, lengths, **opts), x, lengths, f"ctx {ctx}", **opts)
    opts = dict(energy_threshold=5.0, energy_mean_scale=0.5, frames_context=ctx, proportion_threshold=0.6)
    got = _energy(x, lengths, **opts)
    _assert_decisions(got, x, lengths, f"ctx {ctx}, defaults", **opts)
    assert 0 < got[1][-1] < T and np.isnan(got[2][0]) and got[1][0] == 0          # an empty utterance: 0 / 0, nothing voiced
    # no lengths: every utterance has T frames
    _assert_decisions(_energy(x, None, **opts), x, None, f"ctx {ctx}, full", **opts)


@pytest.mark.parametrize("B,T,C,col", [(1, 61, 1, 0), (3, 300, 23, 22), (3, 257, 24, 5), (300, 61, 24, 0), (2, 40, 1024, 1023)])
def test_decisions_over_batch_sizes_widths_and_energy_columns(B, T, C, col):
    x = _energies(B, T, C, seed=B + T + C, col=col)
    lengths = [int(v) for v in np.random.default_rng(B).integers(0, T + 1, B)]
    lengths[0], lengths[-1] = T, (0 if B > 1 else T)
    opts = dict(RECIPE, energy_col=col)
    got = _energy(x, lengths, **opts)
    _assert_decisions(got, x, lengths, (B, T, C, col), **opts)
    assert got[1].sum() > 0
    # the same rows under other strides: the same bits
    again = _energy(x, lengths, rs=C + 9, us=T * (C + 9) + 64, **opts)
    assert all(_same_bits(a, b) for a, b in zip(got, again))


def test_decisions_at_the_edges_of_the_rules():
    T = 40
    x = np.zeros((1, T, 2), dtype=np.float32)
    x[0, :, 0] = np.arange(T, dtype=np.float32)
    # all hot, none hot
    for thr, n in ((-1.0, T), (1e9, 0)):
        opts = dict(energy_threshold=thr, energy_mean_scale=0.0, frames_context=2, proportion_threshold=0.6)
        got = _energy(x, **opts)
        _assert_decisions(got, x, None, ("all or none", thr), **opts)
        assert got[1][0] == n and got[2][0] == thr
    # strict: with no mean scale the frame whose energy EQUALS the threshold is cold
    opts = dict(energy_threshold=17.0, energy_mean_scale=0.0, frames_context=0, proportion_threshold=0.6)
    got = _energy(x, **opts)
    _assert_decisions(got, x, None, "strict", **opts)
    assert got[0][0, 17] == 0 and got[0][0, 18] == 1 and got[1][0] == T - 18
    # a proportion tie: den = 4 at the right edge (t = T - 2 with context 2), two of them hot, threshold 0.5: voiced
    e = np.zeros((1, T, 2), dtype=np.float32)
    e[0, T - 4:T - 2, 0] = 9.0
    opts = dict(energy_threshold=5.0, energy_mean_scale=0.0, frames_context=2, proportion_threshold=0.5)
    got = _energy(e, **opts)
    _assert_decisions(got, e, None, "tie", **opts)
    assert got[0][0, T - 2] == 1 and got[0][0, T - 1] == 0 and got[0][0, T - 7] == 0      # (t = T - 1: one hot of three)
    # a NaN energy: that frame is cold; with a mean scale the threshold is NaN and nothing is voiced
    e = _energies(1, T, 2, seed=9)
    e[0, 11, 0] = NAN
    opts = dict(energy_threshold=5.0, energy_mean_scale=0.0, frames_context=0, proportion_threshold=0.6)
    got = _energy(e, **opts)
    _assert_decisions(got, e, None, "NaN frame", **opts)
    assert got[0][0, 11] == 0 and got[1][0] > 0
    got = _energy(e, **dict(opts, energy_mean_scale=0.5))
    assert got[1][0] == 0 and not got[0].any() and np.isnan(got[2][0])


# ---------------------------------------------------------------- CMVN values

CMVN_LENGTHS = lambda w: sorted({1, max(w - 1, 0), w, w + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1})


def _cmvn_input(w):
    """[B, T, 5] for the lengths of window w: N(0, 1); a constant (the variance floor); mean 1e4 and deviation 1; N(10, 3);
    small values."""
    lengths = CMVN_LENGTHS(w)
    rng = np.random.default_rng(300 + w)
    T = max(lengths)
    x = rng.standard_normal((len(lengths), T, 5)).astype(np.float32)
    x[:, :, 1] = 1.5
    x[:, :, 2] += 1e4
    x[:, :, 3] = x[:, :, 3] * 3 + 10
    x[:, :, 4] *= 1e-3
    return x, lengths


def _assert_values(y, x, lengths, opts, what):
    worst = 0.0
    tile, _, run = vad_ref.tile_plan(x.shape[2], vad_ref.span(**opts))
    for b, L in enumerate(lengths):
        ref, bound = vad_ref.sliding_cmvn(x[b, :L], tile=tile, run=run, **opts)
        tol = bound + np.longdouble(2.0) ** -24 * (np.abs(ref) + bound) + np.longdouble(2.0) ** -149
        err = np.abs(y[b, :L].astype(np.longdouble) - ref)
        assert np.isfinite(y[b, :L]).all(), (what, L)
        bad = err > tol
        assert not bad.any(), (what, L, int(bad.sum()), np.argwhere(bad)[:3].tolist(), float(err[bad].max()), float(tol[bad].min()))
        assert not y[b, L:].any(), (what, L, "rows at or past the length are zeros")
        if L:
            worst = max(worst, float((err / tol).max()))
    return worst


@pytest.mark.parametrize("norm_vars", [False, True])
@pytest.mark.parametrize("center,min_window", [(True, 100), (False, 1), (False, TILE + 1), (False, 600)])
@pytest.mark.parametrize("w", [1, 2, 7, 300])
def test_cmvn_values_lie_inside_the_derived_bound(w, center, min_window, norm_vars):
    x, lengths = _cmvn_input(w)
    opts = dict(cmn_window=w, min_window=min_window, center=center, norm_vars=norm_vars)
    y, new_len = _cmvn(x, lengths, opts)
    assert new_len.tolist() == lengths
    worst = _assert_values(y, x, lengths, opts, (w, center, min_window, norm_vars))
    print(f"[cmvn] w = {w}, center = {center}, min_window = {min_window}, norm_vars = {norm_vars}: worst error / bound {worst:.3f}")
    if norm_vars:
        assert not y[:, :, 1].any()                   # the constant channel: x - mean is 0 whatever the floored variance
        if w == 1 and center:
            assert not y.any()                        # n = 1 everywhere: zeros
    elif w == 1 and center:
        assert not y.any()                            # a frame minus itself


@pytest.mark.parametrize("C,opts,lengths", [
    # rows that do not fit whole: groups of 10 channels (tests/test_vad.py: tile 256 x 10 at a span of 601)
    (80, dict(cmn_window=600, min_window=100, center=False, norm_vars=True), [2 * TILE + 1, 300]),
    # the largest window: the smallest tile, 16 frames of 8 channels, the last group with a single channel
    (25, dict(cmn_window=1900, min_window=1901, center=False, norm_vars=False), [70, 33, 16, 17]),
    (25, dict(cmn_window=1900, min_window=1, center=True, norm_vars=True), [70, 33, 16, 17]),
])
def test_cmvn_with_split_channels_and_with_the_smallest_tile(C, opts, lengths):
    rng = np.random.default_rng(C)
    T = max(lengths)
    x = (rng.standard_normal((len(lengths), T, C)) * 2 + rng.standard_normal(C) * 5).astype(np.float32)
    y, new_len = _cmvn(x, lengths, opts)
    assert new_len.tolist() == lengths
    _assert_values(y, x, lengths, opts, (C, opts))
    # selected through the fused call: the same rows, bit for bit, at their ranks
    mask, counts, _, sel, n = _fused(x, lengths, dict(energy_threshold=0.0, energy_mean_scale=1.0, frames_context=1,
                                                      proportion_threshold=0.5), opts)
    assert 0 < counts[0] < lengths[0]
    for b in range(len(lengths)):
        assert _same_bits(sel[b], vad_ref.select(y[b], mask[b])[0]) and n[b] == counts[b], b


# ---------------------------------------------------------------- purity

def test_an_utterance_has_the_same_bits_wherever_it_stands():
    rng = np.random.default_rng(77)
    L, C = 300, 24
    u = _energies(1, L, C, seed=78)[0]
    vad, cmvn = dict(RECIPE), dict(cmn_window=100, min_window=40, center=False, norm_vars=True)
    alone = _fused(u[None], None, vad, cmvn)
    for pos, T, others in ((0, 300, 1.0), (2, 333, 1.0), (2, 513, 50.0)):
        x = (rng.standard_normal((3, T, C)) * others).astype(np.float32)
        x[pos, :L] = u
        lengths = [T, T // 2, T - 1]
        lengths[pos] = L
        got = _fused(x, lengths, vad, cmvn)
        assert _same_bits(got[0][pos, :L], alone[0][0]) and got[1][pos] == alone[1][0] and _same_bits(got[2][pos:pos + 1], alone[2])
        assert _same_bits(got[3][pos, :L], alone[3][0]) and not got[3][pos, L:].any() and got[4][pos] == alone[4][0]
        # the separate calls, under two other row strides: the same bits again
        for rs in (C, C + 40):
            y, _ = _cmvn(x, lengths, cmvn, rs=rs, us=T * rs + 1, yrs=C + 5)
            sel, n = vad_ref.select(y[pos], got[0][pos])
            assert n == alone[4][0] and _same_bits(sel[:L], alone[3][0])
    assert all(_same_bits(a, b) for a, b in zip(alone, _fused(u[None], None, vad, cmvn)))          # run to run


# ---------------------------------------------------------------- select

def test_select_copies_the_voiced_rows_bit_for_bit_and_zeroes_the_tail():
    B, T, C = 5, 2 * LANES + 1, 24
    x = _energies(B, T, C, seed=55)
    lengths = [T, T, T - 3, T, 40]
    mask = np.zeros((B, T), dtype=np.uint8)
    mask[0] = 1                                       # all
    mask[2, ::2] = 1                                  # alternating (its last frames lie past the length: they do not count)
    mask[3, 2 * LANES - 5:] = 7                       # voiced only in the last chunks; any nonzero entry counts
    mask[4, 10:60] = 1                                # cut by the length
    y, new_len = _cmvn(x, lengths, None, mask)
    for b in range(B):
        m = mask[b].copy()
        m[lengths[b]:] = 0
        ref, n = vad_ref.select(x[b], m)
        assert new_len[b] == n and _same_bits(y[b], ref), b
    assert new_len.tolist() == [T, 0, (T - 3 + 1) // 2, 6, 30]
    # without a mask and without normalisation: the rows below the length, zeros behind
    y, new_len = _cmvn(x, lengths, None, None)
    assert new_len.tolist() == lengths
    for b, L in enumerate(lengths):
        assert _same_bits(y[b, :L], x[b, :L]) and not y[b, L:].any()
    # normalised and selected: the selection of the normalised rows
    cmvn = dict(cmn_window=7, min_window=3, center=True, norm_vars=False)
    plain, _ = _cmvn(x, lengths, cmvn, None)
    y, new_len = _cmvn(x, lengths, cmvn, mask)
    for b in range(B):
        m = mask[b].copy()
        m[lengths[b]:] = 0
        assert _same_bits(y[b], vad_ref.select(plain[b], m)[0]), b


# ---------------------------------------------------------------- the fused call

@pytest.mark.parametrize("cmvn", [None, dict(cmn_window=300, min_window=100, center=True, norm_vars=False),
                                  dict(cmn_window=7, min_window=100, center=False, norm_vars=True),
                                  dict(cmn_window=2, min_window=1, center=False, norm_vars=False)])
@pytest.mark.parametrize("select", [1, 0])
def test_fused_call_equals_the_two_separate_calls(cmvn, select):
    B, T, C = 3, 300, 24
    x = _energies(B, T, C, seed=21)
    lengths = [T, 257, 16]
    for vad in (dict(RECIPE), dict(energy_threshold=9.0, energy_mean_scale=0.0, frames_context=0, proportion_threshold=0.6)):
        mask, counts, thr, y, new_len = _fused(x, lengths, vad, cmvn, select)
        sep = _energy(x, lengths, **vad)
        assert _same_bits(mask, sep[0]) and _same_bits(counts, sep[1]) and _same_bits(thr, sep[2])
        y2, n2 = _cmvn(x, lengths, cmvn, sep[0] if select else None)
        assert _same_bits(y, y2) and _same_bits(new_len, n2)
        assert new_len.tolist() == (counts.tolist() if select else lengths)
        assert 0 < counts[0] < T


# ---------------------------------------------------------------- resources

def test_inside_a_workspace_window_of_the_reported_size():
    from xvector_amd import hip
    B, T, C = 4, 2 * LANES + 9, 24
    x = _energies(B, T, C, seed=31)
    lengths = [T, 300, 0, 17]
    need = int(hip.lib.xvec_vad_workspace_bytes(B, T))
    cmvn = dict(cmn_window=50, min_window=20, center=True, norm_vars=True)
    big, off = ss.window(need, DEV)                  # the window holds 0xFF bytes: nothing is read unwritten
    got = _fused(x, lengths, dict(RECIPE), cmvn, 1, ws=big.data_ptr() + off, need=need)
    assert ss.guards_intact(big, off, need)
    want = _fused(x, lengths, dict(RECIPE), cmvn, 1)
    assert all(_same_bits(a, b) for a, b in zip(got, want))
    _assert_decisions(got[:3], x, lengths, "window", **RECIPE)


def test_runs_under_graph_capture():
    from xvector_amd import hip
    B, T, C = 3, 300, 24
    lengths = [T, 200, 99]
    vad, cmvn = dict(RECIPE), dict(cmn_window=30, min_window=10, center=False, norm_vars=False)
    hosts = [_energies(B, T, C, seed=s) for s in (41, 42)]
    static = torch.from_numpy(hosts[0]).to(DEV)
    lens = _lens(lengths)
    out = _Out(B, T, C)
    ws, need = _workspace(B, T)
    vo, co = _vopt(vad), _copt(cmvn)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = hip.lib.xvec_vad_cmvn(static.data_ptr(), B, T, C, C, T * C, lens.data_ptr(), vo, co, 1, out.mask.data_ptr(), out.ms,
                                   out.counts.data_ptr(), out.thr.data_ptr(), out.y.data_ptr(), out.yrs, out.yus,
                                   out.new_len.data_ptr(), ws.data_ptr(), need, _stream())
    assert rc == 0, hip.lib.xvec_vad_last_error()
    for host in hosts + hosts[:1]:                   # the first input again: the same bits as its first replay
        static.copy_(torch.from_numpy(host))
        g.replay()
        torch.cuda.synchronize()
        out.check()
        got = (out.mask_view().cpu().numpy(), out.counts.cpu().numpy(), out.thr.cpu().numpy(), out.y_view().cpu().numpy(),
               out.new_len.cpu().numpy())
        want = _fused(host, lengths, vad, cmvn, 1)
        assert all(_same_bits(a, b) for a, b in zip(got, want))


# ---------------------------------------------------------------- through Python

def _planted(B, T, C, silence, seed):
    """Features whose energy (column 0) is 12 in speech and 0 in the `silence` stretches [(utt, start, end)]."""
    x = np.random.default_rng(seed).standard_normal((B, T, C)).astype(np.float32)
    x[:, :, 0] = 12.0
    for u, a, b in silence:
        x[u, a:b, 0] = 0.0
    return x


def test_module_calls_equal_the_abi_and_feed_the_extractor(gpu_model):
    from xvector_amd import vad
    B, T, C = 3, 61, 24
    x = _planted(B, T, C, [(0, 0, 9), (0, 30, 41), (1, 50, 61), (2, 20, 25)], seed=61)
    x[:, :, 0] += np.random.default_rng(62).normal(0, 0.5, (B, T)).astype(np.float32)
    lengths = [61, 61, 40]
    xd = torch.from_numpy(_poisoned(x, lengths)).to(DEV)
    opts = dict(RECIPE, frames_context=0, proportion_threshold=0.5)
    v = vad.energy_vad(xd, lengths, **opts)
    ref = vad_ref.energy_vad(x, lengths, **opts)
    assert np.array_equal(v.mask.cpu().numpy(), ref[0]) and np.array_equal(v.counts.cpu().numpy(), ref[1])
    assert _same_bits(v.threshold.cpu().numpy(), ref[2])
    assert ref[1].tolist() == [61 - 9 - 11, 50, 40 - 5]
    cm = dict(cmn_window=300, center=True, norm_vars=False)
    prep = vad.VadCmvn(vad=opts, **cm)
    p = prep(xd, lengths)
    assert isinstance(p.lengths, list) and p.lengths == ref[1].tolist() and min(p.lengths) >= 15
    assert torch.equal(p.mask, v.mask)
    y = vad.sliding_cmvn(xd, lengths, min_window=100, **cm)
    sel, n = vad.select_voiced(y, v.mask, lengths)
    assert torch.equal(sel, p.feats) and n.tolist() == p.lengths
    assert torch.equal(vad.VadCmvn(vad=None, **cm)(xd, lengths), y)                    # CMVN alone: a bare tensor
    q = prep.with_select(False)(xd, lengths)
    assert torch.equal(q.feats, y) and q.lengths == lengths and torch.equal(q.mask, v.mask)
    # a view with padded rows goes through without a copy and gives the same bits
    wide = torch.full((B, T, C + 8), NAN, device=DEV)
    wide[:, :, :C] = xd
    assert torch.equal(prep(wide[:, :, :C], lengths).feats, p.feats)
    # the extractor on the prepared batch against each utterance's restatement-normalised voiced frames alone
    got = gpu_model.extract_x_vec(p.feats, p.lengths)
    for b, L in enumerate(lengths):
        norm, _ = vad_ref.sliding_cmvn(x[b, :L], min_window=100, **cm)
        rows = norm.astype(np.float32)[ref[0][b, :L] != 0]
        alone = gpu_model.extract_x_vec(torch.from_numpy(rows[None]).to(DEV))
        assert_parity(got[b:b + 1], alone, 1e-4, f"utterance {b}")


def test_diarizer_windows_lie_inside_the_speech_runs(synth):
    import xvector_amd as xa
    from xvector_amd import diarize, vad
    cin, hid, xv, nc = 24, 72, 16, 3
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in
          synth.make_state_dict(706, input_size=cin, hidden_size=hid, num_classes=nc, x_vector_size=xv).items()}
    model = xa.XVectorModel(input_size=cin, hidden_size=hid, num_classes=nc, x_vector_size=xv)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    lengths = [400, 300]
    silence = [(0, 0, 30), (0, 150, 200), (0, 380, 400), (1, 100, 104), (1, 200, 260)]
    x = _planted(2, 400, cin, silence, seed=71)
    who = (np.arange(400) // 100) % 2                # two speakers taking turns of 100 frames
    shift = np.random.default_rng(72).standard_normal(cin).astype(np.float32) * 1.5
    shift[0] = 0.0
    x += np.where(who[None, :, None] == 0, shift, -shift)
    xd = torch.from_numpy(_poisoned(x, lengths)).to(DEV)
    front = vad.VadCmvn(cmn_window=300, center=True, vad=dict(RECIPE, frames_context=0, proportion_threshold=0.5))
    win, hop, gap = 60, 30, 5
    d = diarize.Diarizer(model, "cosine", win=win, hop=hop, device=DEV, frontend=front, max_gap=gap)
    res = d.diarize(xd, lengths=lengths, n_speakers=2)
    speech = np.ones((2, 400), dtype=np.uint8)
    for u, a, b in silence:
        speech[u, a:b] = 0
    speech[1, 300:] = 0
    p = front.with_select(False)(xd, lengths)
    assert np.array_equal(p.mask.cpu().numpy(), speech)
    runs = vad.speech_runs(speech, lengths, gap, win)
    assert runs.tolist() == [[0, 30, 120], [0, 200, 180], [1, 0, 200]]      # the 4 silent frames of recording 1 are bridged
    assert np.array_equal(res.windows, vad.run_windows(runs, win, hop))
    for u, s, n in res.windows.tolist():
        assert any(u == ru and rs <= s and s + n <= rs + rn for ru, rs, rn in runs.tolist())
        quiet = np.flatnonzero(np.diff(np.concatenate([[1], speech[u, s:s + n], [1]])))       # falls and rises inside the window
        assert all(b - a <= gap for a, b in zip(quiet[0::2], quiet[1::2]))
    # the vectors are those of the windows of the normalised recordings, in the recordings' own frames
    vecs = model.extract_segments(p.feats, res.windows, lengths=lengths)
    S = xa.scoring.cosine_scores(vecs.double(), device=DEV)
    counts = [int((res.windows[:, 0] == u).sum()) for u in range(2)]
    cl = diarize.cluster(S, np.concatenate([[0], np.cumsum(counts)]), n_speakers=2)
    assert np.array_equal(res.labels, cl.labels.cpu().numpy()) and res.n_clusters.tolist() == [2, 2]
    # turns in ORIGINAL frames: none inside the long silences, recording 0 from its first speech frame
    t = res.turns
    assert t[t[:, 0] == 0][0, 1] == 30 and t[t[:, 0] == 1][0, 1] == 0
    for u, a, b, _ in t.tolist():
        assert any(u == ru and rs <= a and b <= rs + rn for ru, rs, rn in runs.tolist())
    # without a front end the same Diarizer windows the whole recordings, silence included
    plain = diarize.Diarizer(model, "cosine", win=win, hop=hop, device=DEV).diarize(xd.nan_to_num(), lengths=lengths, n_speakers=2)
    assert len(plain.windows) > len(res.windows) and plain.windows[0].tolist() == [0, 0, win]
