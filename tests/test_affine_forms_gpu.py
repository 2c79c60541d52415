"""The segment-layer GEMMs (csrc/affine.hip) in every kernel form launch_affine_f32 dispatches to (csrc/affine_plan.h), through
xvec_segment_layer -- the call the whole path makes, on a caller-given x and scratch window -- against x.double() @ W.double().T
+ b on the CPU.  Every case asserts the form and the number of K ranges it was written for (xvec_get_affine_dispatch): a case
that silently ran another form is the failure this file exists to prevent.  tests/test_affine_plan.py pins the same plans on
the CPU.

Outputs and scratch sit in NaN-filled windows between NaN guards.  The scratch window is exactly the bytes passed and is
NaN-filled before every call: a partial that is read but never written surfaces as a NaN in y, a write past S M N floats, past
row M or past column N in a guard or in the part of the scratch the plan leaves alone.

Bars: the ones tests/test_parity_gpu.py::test_segment_layers_inside_the_path applies to every precision, 3e-5 for layer 6 and
1e-4 for layer 7 and output; none is introduced here.  The measured errors are printed per form and precision
(XVEC_AFFINE_ERRORS_LOG=<file> appends them to a file: profiles/affine_forms_errors.txt is such a log of one full run)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from conftest import assert_parity
from tdnn_support import DEV, make_model

pytestmark = pytest.mark.gpu
GUARD = 1024                          # floats on either side of every window (a multiple of 4: the windows stay 16-byte aligned)
BAR = {6: 3e-5, 7: 1e-4, 8: 1e-4}     # test_segment_layers_inside_the_path's
K6 = 3000
AMPLE = 20                            # scratch in units of M N floats that limits no plan (16 ranges at most)
# (x_vector_size, num_classes) of the handles; the frame-level stack is narrow, it never runs here
CFG = {"full": (512, 1212), "full1211": (512, 1211), "x448": (448, 60), "x200": (200, 8), "x252": (252, 8), "x64": (64, 8),
       "x66": (66, 10)}
L6_ROWS = 4100                        # layer 6's operand and fp64 reference are made once for the largest M and cut


class Window:
    """A NaN-poisoned device buffer of exactly `shape` between two NaN guards (as tests/test_train_gpu.py's)."""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        self.t = self.buf[GUARD: GUARD + n].view(*shape)
        assert self.t.data_ptr() % 16 == 0

    def poison(self):
        self.buf.fill_(float("nan"))

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[self.buf.numel() - GUARD:]).all())


@functools.lru_cache(maxsize=None)
def handle(cfg):
    """(model, handle) of CFG[cfg] whose segment layers are re-loaded with weights N(0, 1) / sqrt(in) and biases N(0, 1): a
    dropped bias is far outside any bar.  The weights stay on the host in fp64 for the reference."""
    from xvector_amd import hip, synth
    from xvector_amd._device import stream
    xv, nc = CFG[cfg]
    kw = dict(input_size=24, hidden_size=32, num_classes=nc, x_vector_size=xv)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict(seed=3, **kw).items()}
    m = make_model(sd, **kw)
    eng = m._engine(torch.device(DEV))
    rng = np.random.default_rng(1000 + xv + nc)
    params = {}
    for which, (n, k) in ((6, (xv, K6)), (7, (xv, xv)), (8, (nc, xv))):
        W = torch.from_numpy((rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32))
        b = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
        Wd, bd = W.to(DEV), b.to(DEV)
        hip.check(hip.lib.xvec_load_affine(eng.h, which, Wd.data_ptr(), bd.data_ptr(), stream(DEV)))
        torch.cuda.synchronize()
        params[which] = (W.double(), b.double())
    return m, eng, params


@functools.lru_cache(maxsize=None)
def operand(cfg, which, rows):
    """x[rows, in] ~ N(0, 1) and its fp64 pre-activation reference, made once per (handle, layer) and left unchanged."""
    W, b = handle(cfg)[2][which]
    x = torch.from_numpy(np.random.default_rng(77 * which + rows).standard_normal((rows, W.shape[1]), dtype=np.float32))
    return x, x.double() @ W.t() + b


def _note(form, S, dtype, got, ref, what=""):
    d = (got.double().cpu() - ref).abs()
    row = (d.norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)).max().item()
    elem = (d.max() / ref.abs().mean()).item()
    line = f"[affine forms] {form:>20} S={S:<2} {'bf16' if dtype else 'fp32'}: worst row-wise {row:.3e}, worst element / mean|ref| {elem:.3e}  ({what})"
    print(line)
    if os.environ.get("XVEC_AFFINE_ERRORS_LOG"):
        with open(os.environ["XVEC_AFFINE_ERRORS_LOG"], "a") as f:
            f.write(line + "\n")


def run_case(cfg, which, M, units, form, S, dtype_name, rows=None):
    """Layer `which` of handle `cfg` on M rows with a scratch window of floor(units M N) floats (None: AMPLE M N; a negative
    count of floats is taken off: -1 is one float short of 2 M N with units = 2): the form and S asserted, then parity, ReLU,
    repeatability and the row permutation, with and without ReLU."""
    from xvector_amd import hip
    from xvector_amd._device import stream
    m, eng, params = handle(cfg)
    dtype = {"fp32": hip.F32, "bf16": hip.BF16}[dtype_name]
    x_all, ref_all = operand(cfg, which, rows or M)
    x_cpu, ref = x_all[:M], ref_all[:M]
    N, K = params[which][0].shape
    n_scr = AMPLE * M * N if units is None else int(units * M * N) if units >= 0 else 2 * M * N + int(units)
    x = x_cpu.to(DEV)
    perm = torch.from_numpy(np.random.default_rng(M).permutation(M))
    xp = x_cpu[perm].to(DEV)
    y, scr = Window(M, N), Window(max(n_scr, 4))
    x3 = dtype == hip.BF16 and K % 4 == 0 and form in ("splitk", "direct")
    want = (form + "_bf16x3" if x3 else form, S)
    what0 = f"{cfg} layer {which} M={M} scratch={n_scr} {dtype_name}"

    def call(xd, relu):
        y.poison()
        scr.poison()
        hip.check(hip.lib.xvec_segment_layer(eng.h, which, xd.data_ptr(), M, relu, dtype, y.ptr(), scr.ptr(), 4 * n_scr, stream(DEV)))
        torch.cuda.synchronize()
        got = hip.affine_dispatch(eng.h)[which - 6]
        assert got == want, f"{what0}: ran {got}, the case was written for {want}"
        assert y.guards_intact(), f"{what0}: a write outside y[M, N]"
        assert scr.guards_intact(), f"{what0}: a write outside the scratch window"
        used = S * M * N if want[0].startswith("splitk") else 0
        assert torch.isnan(scr.t[used:n_scr]).all() and torch.isnan(scr.t[n_scr:]).all(), f"{what0}: a write past S M N floats of scratch"
        assert torch.isfinite(scr.t[:used]).all(), f"{what0}: a partial was not written"
        assert torch.isfinite(y.t).all(), f"{what0}: y not fully written"
        return y.t.clone()

    for relu in (0, 1):
        what = f"{what0} relu={relu}"
        got = call(x, relu)
        want_ref = torch.relu(ref) if relu else ref
        _note(want[0], S, dtype, got, want_ref, f"{cfg} layer {which} M={M} relu={relu}")
        assert_parity(got, want_ref, BAR[which], what)
        if relu:
            g = got.cpu()
            assert (g >= 0).all(), f"{what}: a negative output behind the ReLU"
            off = ref < -1e-3 * ref.abs().mean()
            assert off.any() and (g[off] == 0).all(), f"{what}: not exactly 0 where the reference is clearly negative"
        for _ in range(2):
            assert torch.equal(call(x, relu), got), f"{what}: a repeat call gives other bits"
        gp = call(xp, relu)
        assert torch.equal(gp, got[perm.to(DEV)]), f"{what}: permuting the rows of x does not permute the rows of y bit for bit"


DTYPES = ["fp32", "bf16"]

# layer 6 (N = 512, K = 3000, 47 trips): every range count the plan gives it.  Last ranges of 2, 3, 5, 7, 11, 15 and 23 trips.
RANGE_COUNTS = [(1, None, 16), (63, None, 16), (65, None, 16), (256, None, 16), (257, None, 12), (448, None, 10), (449, None, 8),
                (641, None, 6), (1025, None, 4), (2049, None, 2), (4032, None, 2), (500, 2, 2), (500, 3, 3), (500, 5, 5), (500, 7, 7)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,units,S", RANGE_COUNTS)
def test_layer6_range_counts(M, units, S, dtype):
    """The unrolled reduce (S = 16), its 4-wide loop (12, 8, 4; 10, 6, 5, 7 with a tail) and its tail loop alone (2, 3)."""
    run_case("full", 6, M, units, "splitk", S, dtype, rows=L6_ROWS)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layer6_scratch_one_float_short_of_two_partials(dtype):
    run_case("full", 6, 500, -1, "tile16", 1, dtype, rows=L6_ROWS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,S", [("x448", 3), ("full", 4), ("x200", 2), ("x252", 2)])
def test_layer7_one_trip_last_range_and_short_k(cfg, S, dtype):
    """x_vector_size 448: seven trips in ranges of 3, 3 and 1; 512: four ranges of two; 200 and 252: K tails of 8 and 60 past a
    trip (and N tails of 8 and 60 past a tile), two ranges of two trips."""
    run_case(cfg, 7, 37, None, "splitk", S, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [65, 95, 96, 97, 127, 128])
def test_m_tails_split_k(M, dtype):
    """M mod 64 in {1, 31, 32, 33, 63, 0}: the clamped rows min(row, M - 1) must not leak into stored rows, the 32-row wave
    quadrants are stored under row < M."""
    run_case("full", 6, M, None, "splitk", 16, dtype, rows=L6_ROWS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [1985, 2015, 2016, 2017, 2047, 2048])
def test_m_tails_direct(M, dtype):
    run_case("full", 6, M, -1, "direct", 1, dtype, rows=L6_ROWS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,form,S", [("full", "splitk", 4), ("full1211", "tile16", 1), ("x448", "splitk", 3)])
def test_output_n_tails(cfg, form, S, dtype):
    """num_classes 1212: 19 column tiles, the last one 60 wide; 1211: N % 4 != 0, tile16; 60 classes at x_vector_size 448: one
    column tile of 60."""
    run_case(cfg, 8, 37, None, form, S, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,which,M,units,form", [("full", 6, 4033, None, "direct"), ("full", 6, 1985, -1, "direct"),
                                                    ("full", 6, 1984, -1, "tile16"), ("x64", 7, 16321, None, "direct"),
                                                    ("x64", 7, 16320, None, "tile16")])
def test_direct_forms_and_their_thresholds(cfg, which, M, units, form, dtype):
    """256 tiles of 64 x 64 and no split: the direct form (4033 rows with ample scratch: 64 x 8 tiles, one range; 1985 rows
    with less than two partials of scratch: 32 x 8; 16321 rows at width 64: 256 x 1 tiles of one trip); one row fewer than the
    last two and it is tile16."""
    run_case(cfg, which, M, units, form, 1, dtype, rows=L6_ROWS if which == 6 else None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [7, 8])
def test_elementwise_tile16_at_k_not_a_multiple_of_4(which, dtype):
    """x_vector_size 66: K % 4 != 0, the handle has no bf16 pairs of these weights, and XVEC_BF16 must report the fp32 form."""
    run_case("x66", which, 37, None, "tile16_elementwise", 1, dtype)


@pytest.mark.parametrize("which", [6, 7])
def test_elementwise_tile16_on_an_x_off_16_bytes(which):
    """xvec_affine on an x that starts 4 bytes into its allocation: the element-wise kernel, the same values and the same order
    of operations as the 16-byte loads of the aligned call -- the same bits."""
    from xvector_amd import hip
    from xvector_amd._device import stream
    m, eng, params = handle("full")
    M = 37
    x_cpu, ref = (t[:M] for t in operand("full", which, L6_ROWS if which == 6 else M))
    N, K = params[which][0].shape
    buf = torch.zeros(M * K + 4, device=DEV)
    off = buf[1: 1 + M * K].view(M, K)
    off.copy_(x_cpu)
    x = x_cpu.to(DEV)
    assert off.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
    out = {}
    for relu in (0, 1):
        for name, xd, form in (("aligned", x, "tile16"), ("off", off, "tile16_elementwise")):
            y = Window(M, N)
            hip.check(hip.lib.xvec_affine(eng.h, which, xd.data_ptr(), M, relu, y.ptr(), stream(DEV)))
            torch.cuda.synchronize()
            assert hip.affine_dispatch(eng.h)[which - 6] == (form, 1)
            assert y.guards_intact() and torch.isfinite(y.t).all()
            out[name] = y.t.clone()
            _note(form, 1, 0, out[name], torch.relu(ref) if relu else ref, f"xvec_affine layer {which} M={M} relu={relu} x {name}")
            assert_parity(out[name], torch.relu(ref) if relu else ref, BAR[which], f"xvec_affine layer {which} {name} relu={relu}")
        assert torch.equal(out["off"], out["aligned"]), "the element-wise kernel disagrees with the 16-byte loads"


def test_argument_errors_of_the_entry():
    from xvector_amd import hip
    m, eng, params = handle("x64")
    x, y = torch.zeros(4, 64, device=DEV), torch.zeros(4, 64, device=DEV)
    scr = torch.zeros(64, device=DEV)
    call = hip.lib.xvec_segment_layer
    assert call(None, 7, x.data_ptr(), 4, 0, hip.F32, y.data_ptr(), None, 0, None) == hip.ERR_ARG
    assert call(eng.h, 9, x.data_ptr(), 4, 0, hip.F32, y.data_ptr(), None, 0, None) == hip.ERR_ARG
    assert call(eng.h, 7, x.data_ptr(), 0, 0, hip.F32, y.data_ptr(), None, 0, None) == hip.ERR_ARG
    assert call(eng.h, 7, x.data_ptr(), 4, 0, 3, y.data_ptr(), None, 0, None) == hip.ERR_ARG
    assert call(eng.h, 7, x.data_ptr(), 4, 0, hip.F32, y.data_ptr(), None, 64, None) == hip.ERR_ARG
    assert call(eng.h, 7, x.data_ptr(), 4, 0, hip.F32, y.data_ptr(), scr.data_ptr() + 4, 64, None) == hip.ERR_ARG
    n = ctypes.c_int(0)
    assert hip.lib.xvec_get_affine_dispatch(eng.h, None, None, ctypes.byref(n)) == hip.ERR_ARG
