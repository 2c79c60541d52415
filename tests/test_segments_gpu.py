"""x-vectors over sliding windows and segments of recordings (XVectorModel.extract_segments / extract_windows,
xvec_forward_segments): every segment's result against the reference's arithmetic on the crop alone (oracle) and against the
model's own whole-utterance path on the crops, in all three precisions and all four modes; the call planner's cuts, the
large-batch kernels, the workspace bound and the handle's state.  Bars: the project's (1e-4 fp32 / bf16x3, 1e-2 with
elem_tol 2e-2 bf16).  The pooled statistics are checked against the oracle too: the means everywhere, the whole rows element
by element except the stds that the oracle's own layer-5 frames show to be ill-conditioned -- a channel that is on in one to seven
of a crop's frames, or whose std is tiny (conftest.nearly_off_channels); those are listed, their share is bounded, and the
x-vectors made from them are checked in full."""
import ctypes

import numpy as np
import pytest
import torch

import xvector_oracle as oracle
from conftest import assert_parity, assert_parity_masked, float_params, nearly_off_channels
from tdnn_support import DEV, make_model

pytestmark = pytest.mark.gpu
LENS = [47, 120, 333]
ILL_STD_SHARE = 1.0e-2          # 1.5 x the 0.65e-2 of a pooled row the oracle's own frames list on the crops of 40 frames and more (refs)
BARS = {"fp32": dict(tol=1e-4), "bf16x3": dict(tol=1e-4), "bf16": dict(tol=1e-2, elem_tol=2e-2)}


@pytest.fixture(scope="module")
def recs(synth):
    """Three recordings, zero-padded to [3, 333, 24] (host), with garbage behind the short ones' ends."""
    x = torch.as_tensor(synth.make_mfcc(3, max(LENS), seed=21)).clone()
    return x


@pytest.fixture(scope="module")
def segments():
    from xvector_amd import sliding_windows
    win = sliding_windows(LENS, 40, 13, min_tail=16)
    hand = np.asarray([(1, 50, 16), (0, 0, 47), (2, 7, 55), (2, 7, 55), (2, 318, 15), (1, 104, 16)], dtype=np.int32)
    return np.concatenate([hand[:2], win, hand[2:]])


@pytest.fixture(scope="module")
def crops(recs, segments):
    return [recs[u, s:s + n] for u, s, n in segments.tolist()]


@pytest.fixture(scope="module")
def refs(sd42, crops):
    """The reference's results on every crop alone (fp32 oracle on the CPU), computed once."""
    p = float_params(sd42)
    with torch.no_grad():
        frames = [oracle.time_context_layers(c[None], p)[0] for c in crops]          # layer 5's output, [len - 14, 1500] each
        pooled = torch.cat([oracle.stat_pool(f[None]) for f in frames])
        # the ReLU output in front of layer 5's BatchNorm (tdnn_layer.py:36-39 inverted): which channels are on in which frames
        k = "time_context_layers.4.norm."
        sc = sd42[k + "weight"].double() / torch.sqrt(sd42[k + "running_var"].double() + 1e-5)
        sh = sd42[k + "bias"].double() - sd42[k + "running_mean"].double() * sc
        ill = torch.cat([nearly_off_channels(((f.double() - sh) / sc)[None], r[None, 1500:])
                         for f, r in zip(frames, pooled)])
        return {"ill_std": ill, "xvec6": torch.cat([oracle.extract_x_vec(c[None], p) for c in crops]),
                "xvec7": torch.cat([oracle.extract_x_vec(c[None], p, layer=7) for c in crops]),
                "logits": torch.cat([oracle.forward(c[None], p) for c in crops]),
                "pooled": pooled}


@pytest.fixture(scope="module")
def models(sd42):
    return {prec: make_model(sd42, precision=prec) for prec in BARS}


def _padded(recs):
    x = recs.clone()
    for u, n in enumerate(LENS):
        x[u, n:] = 1e3          # what lies behind a recording's end must not matter
    return x.to(DEV)


@pytest.mark.parametrize("precision", list(BARS))
def test_segments_against_the_oracle_on_the_crops(models, recs, segments, crops, refs, precision):
    m, bar = models[precision], BARS[precision]
    x = _padded(recs)
    one = segments[:, 2] == 15                       # one pooled frame: NaN std (torch.std), so NaN results
    assert one.sum() == 1
    got = m.extract_segments(x, segments, lengths=LENS)
    assert got.shape == (len(segments), 512)
    assert torch.isnan(got[one]).all() and torch.isnan(refs["xvec6"][one]).all()
    assert_parity(got[~one], refs["xvec6"][~one], what=f"{precision} layer 6 vs oracle", **bar)
    dup = [i for i, s in enumerate(segments.tolist()) if s == [2, 7, 55]]
    assert len(dup) == 2 and torch.equal(got[dup[0]], got[dup[1]]), "duplicates give identical rows"
    # logits, layer 7, pooled
    assert_parity(m.extract_segments(x, segments, lengths=LENS, logits=True)[~one], refs["logits"][~one],
                  what=f"{precision} logits vs oracle", **bar)
    m.x_vec_extract_layer = 7
    try:
        assert_parity(m.extract_segments(x, segments, lengths=LENS)[~one], refs["xvec7"][~one],
                      what=f"{precision} layer 7 vs oracle", **bar)
    finally:
        m.x_vec_extract_layer = 6
    pooled = m.extract_segments(x, segments, lengths=LENS, pooled=True)
    assert pooled.shape == (len(segments), 3000)
    assert torch.isnan(pooled[one][:, 1500:]).all() and torch.isfinite(pooled[one][:, :1500]).all()
    assert_parity(pooled[:, :1500], refs["pooled"][:, :1500], what=f"{precision} pooled means vs oracle", **bar)
    # the whole rows, means and stds, against the oracle at the path's bar -- except the listed ill-conditioned stds, on the
    # crops of 40 frames and more (26 pooled frames: "on in fewer than 8 frames" says nothing about a crop that has 2).
    # The list and its share are the oracle's own.
    long = torch.from_numpy(segments[:, 2] >= 40)
    assert long.sum() == 34
    ill = torch.cat([torch.zeros_like(refs["ill_std"]), refs["ill_std"]], 1)
    assert_parity_masked(pooled[long], refs["pooled"][long], bar["tol"], f"{precision} pooled vs oracle",
                         bar.get("elem_tol", bar["tol"]), ill[long], max_excluded=ILL_STD_SHARE)
    # the model's own whole-utterance path on the crops: equal-length crops stacked, the others through lengths=
    full = segments[:, 2] == 40
    stack = torch.stack([c for c, f in zip(crops, full) if f]).to(DEV)
    assert len(stack) > 25
    assert_parity(got[full], m.extract_x_vec(stack), what=f"{precision} vs extract_x_vec on the stacked crops", **bar)
    assert_parity(pooled[full], m.pooled(stack), what=f"{precision} pooled vs pooled() on the stacked crops", **bar)
    rest = [i for i in np.flatnonzero(~full & ~one)]
    pad = torch.zeros(len(rest), 60, 24)
    for k, i in enumerate(rest):
        pad[k, :len(crops[i])] = crops[i]
    assert_parity(got[rest], m.extract_x_vec(pad.to(DEV), lengths=[len(crops[i]) for i in rest]),
                  what=f"{precision} tails vs extract_x_vec(lengths=)", **bar)


@pytest.mark.parametrize("precision", list(BARS))
def test_whole_recordings_packed_and_padded_forms(models, recs, precision):
    m, bar = models[precision], BARS[precision]
    x = _padded(recs)
    whole = [(u, 0, n) for u, n in enumerate(LENS)]
    got = m.extract_segments(x, whole, lengths=LENS)
    assert_parity(got, m.extract_x_vec(x, lengths=LENS), what=f"{precision} one segment per recording", **bar)
    # packed rows with offsets: the same call after the host plan -> bit-identical
    packed = torch.cat([recs[u, :n] for u, n in enumerate(LENS)]).to(DEV)
    offs = np.concatenate([[0], np.cumsum(LENS)]).tolist()
    from xvector_amd import sliding_windows
    seg = sliding_windows(LENS, 40, 13, min_tail=16)
    a = m.extract_segments(x, seg, lengths=LENS)
    b = m.extract_segments(packed, seg, offsets=offs)
    assert torch.equal(a, b), "packed and padded input forms must agree"
    v, w = m.extract_windows(x, 40, 13, lengths=LENS, min_tail=16)
    assert np.array_equal(w, seg) and torch.equal(v, a)
    # any order: the rows follow the caller's list
    perm = np.random.default_rng(2).permutation(len(seg))
    c = m.extract_segments(x, seg[perm], lengths=LENS)
    assert_parity(c, a[torch.from_numpy(perm).to(DEV)], what=f"{precision} permuted list", **bar)


@pytest.mark.parametrize("precision", list(BARS))
def test_long_recording_cut_into_pieces(models, synth, precision):
    """2000 frames with max_frames = 600: five calls on overlapping pieces (tests/test_segments.py has the cuts by hand)
    against the uncut call."""
    from xvector_amd import sliding_windows
    m, bar = models[precision], BARS[precision]
    x = torch.as_tensor(synth.make_mfcc(1, 2000, seed=23)).to(DEV)
    seg = sliding_windows([2000], 300, 75, min_tail=20)
    uncut = m.extract_segments(x, seg)
    cut = m.extract_segments(x, seg, max_frames=600)
    assert_parity(cut, uncut, what=f"{precision} cut vs uncut", **bar)
    rev = m.extract_segments(x, seg[::-1].copy(), max_frames=600)
    assert torch.equal(rev.flip(0), cut), "results return in the caller's order"
    with pytest.raises(ValueError, match="max_frames"):
        m.extract_segments(x, seg, max_frames=299)


def test_too_large_splits_by_segments_where_frames_cannot_halve(models, recs, monkeypatch):
    """A library that takes at most 10 segments a call (stood in for: XVEC_ERR_TOO_LARGE above that, nothing enqueued): dense
    and repeated segments over 60 frames, where half the frames would no longer hold the longest segment, still come out,
    in the caller's order and equal to the single call at the path's bar (the pieces are other hulls)."""
    from xvector_amd import hip
    m = models["fp32"]
    x = recs[2:3, :60].to(DEV)
    seg = np.asarray([(0, s, 40 + s % 3) for s in range(18)] + [(0, 5, 55)] * 4 + [(0, 0, 60)], dtype=np.int32)
    seg = seg[np.random.default_rng(5).permutation(len(seg))]
    whole = m.extract_segments(x, seg)
    real, sizes = hip.lib.xvec_forward_segments, []

    def limited(*a):
        sizes.append(a[7])
        return hip.ERR_TOO_LARGE if a[7] > 10 else real(*a)
    monkeypatch.setattr(hip.lib, "xvec_forward_segments", limited)
    got = m.extract_segments(x, seg)
    assert sizes[0] == len(seg) and max(sizes[1:]) <= 12 and sum(n for n in sizes if n <= 10) == len(seg), sizes
    assert_parity(got, whole, what="split by segments vs one call", **BARS["fp32"])


EXPECT_KERNELS = {"fp32": ["tile128"] * 5, "bf16": ["first", "pp", "pp", "pp", "pp"],
                  # bf16x3 layer 5 writes fp32 rows, which only the 128x128 kernel does (csrc/xvec_api.hip, plan_layer)
                  "bf16x3": ["first", "pp", "pp", "pp", "tile128"]}


@pytest.mark.parametrize("precision", list(BARS))
def test_large_batch_kernels(models, synth, precision):
    """8 recordings of 9000 frames, win 300 / hop 75: the frame-level layers take their large-batch kernels and forms, and
    a seeded sample of 64 windows agrees with the existing path on the crops."""
    m, bar = models[precision], BARS[precision]
    x = torch.as_tensor(synth.make_mfcc(8, 9000, seed=29)).to(DEV)
    v, w = m.extract_windows(x, 300, 75)
    assert v.shape == (8 * 117, 512) and torch.isfinite(v).all()
    assert m.last_dispatch() == EXPECT_KERNELS[precision], m.last_dispatch()
    if precision == "fp32":
        assert m.last_forms() == ["direct", "winograd_f23", "winograd_f23", "bf16_split3", "bf16_split3"], m.last_forms()
        assert m.last_operands()[1:] == ["bf16_split3"] * 4, m.last_operands()
    idx = np.sort(np.random.default_rng(31).choice(len(w), 64, replace=False))
    crops = torch.stack([x[u, s:s + n] for u, s, n in w[idx].tolist()])
    assert_parity(v[torch.from_numpy(idx).to(DEV)], m.extract_x_vec(crops), what=f"{precision} sampled windows", **bar)


@pytest.mark.parametrize("precision", list(BARS))
def test_workspace_bound_and_handle_state(models, recs, precision):
    from xvector_amd import hip, sliding_windows
    from xvector_amd._device import stream
    m = models[precision]
    x = _padded(recs)
    before = m.extract_x_vec(x, lengths=LENS)
    seg = sliding_windows(LENS, 40, 13, min_tail=16)
    packed = torch.cat([recs[u, :n] for u, n in enumerate(LENS)]).to(DEV)
    offs = (ctypes.c_int64 * 4)(0, *np.cumsum(LENS).tolist())
    eng = m._engine(torch.device(DEV))
    need = int(hip.lib.xvec_segments_workspace_bytes(eng.h, sum(LENS), 3, len(seg)))
    assert need > int(hip.lib.xvec_workspace_bytes(eng.h, sum(LENS), 3)) and need % 256 == 0
    guard = 4096
    buf = torch.empty(need + guard, dtype=torch.uint8, device=DEV)
    buf[need:] = 0xFF                                   # NaN bit patterns behind the workspace
    sd = torch.from_numpy(np.ascontiguousarray(seg.T)).to(DEV)
    out = torch.empty(len(seg), 512, device=DEV)
    dt = {"fp32": hip.F32, "bf16": hip.BF16, "bf16x3": hip.BF16X3}[precision]

    def call(nbytes, n_seg=len(seg), s0=sd[0].data_ptr()):
        return hip.lib.xvec_forward_segments(eng.h, packed.data_ptr(), offs, 3, s0, sd[1].data_ptr(), sd[2].data_ptr(), n_seg,
                                             hip.MODE_XVEC6, dt, out.data_ptr(), buf.data_ptr(), nbytes, stream(DEV))
    assert call(need - 1) == hip.ERR_WORKSPACE
    most = 65535 * 16                                   # ceil(M / 16) blocks on grid.y in the segment layers' direct form
    assert call(need, n_seg=most + 1) == hip.ERR_TOO_LARGE and "segments per call" in hip.last_error()
    assert hip.lib.xvec_segments_workspace_bytes(eng.h, sum(LENS), 3, most) > need
    assert hip.lib.xvec_segments_workspace_bytes(eng.h, sum(LENS), 3, most + 1) == 0
    assert call(need, n_seg=0) == hip.ERR_ARG and call(need, s0=None) == hip.ERR_ARG
    hip.check(call(need))
    torch.cuda.synchronize()
    assert (buf[need:] == 0xFF).all(), "the call wrote behind xvec_segments_workspace_bytes"
    assert torch.equal(out, m.extract_segments(x, seg, lengths=LENS))
    # a segment the host cannot see to be bad gives a NaN row, its neighbours stay
    bad = seg.copy()
    bad[3] = (1, 100, 40)                               # leaves its recording of 120 frames
    sd.copy_(torch.from_numpy(np.ascontiguousarray(bad.T)))
    good = out.clone()
    hip.check(call(need))
    torch.cuda.synchronize()
    keep = [i for i in range(len(seg)) if i != 3]
    assert torch.isnan(out[3]).all() and torch.equal(out[keep], good[keep])
    # the handle is as it was: the whole-utterance path gives the same bits
    assert torch.equal(m.extract_x_vec(x, lengths=LENS), before)


# ---------------------------------------------------------------------------------- many segments over few frames
# The segment layers split K into the dead activation buffers, whose size follows the recording's FRAMES, while their M is the
# number of SEGMENTS: one 333-frame recording offers 648 rows x 512 channels x 2 buffers = 663 552 floats, which holds two
# partial results of 500 segments (split-K, two ranges), not two of 1000 (tile16: 16 x 8 = 128 tiles of 64 x 64) and not
# two of 4100 either, where the 65 x 8 = 520 tiles fill the chip without a split (the direct form).  csrc/affine_plan.h;
# tests/test_affine_forms_gpu.py runs the same forms on operands of their own.  None of the three lists is cut by the planner.
DOZEN = np.asarray([(0, 0, 40), (0, 293, 40), (0, 0, 333), (0, 7, 55), (0, 100, 150), (0, 150, 16), (0, 33, 300), (0, 200, 99),
                    (0, 61, 17), (0, 250, 83), (0, 120, 64), (0, 1, 128)], dtype=np.int32)
MANY = {500: ("splitk", 2), 1000: ("tile16", 1), 4100: ("direct", 1)}


@pytest.fixture(scope="module")
def dozen_refs(sd42, recs):
    p = float_params(sd42)
    with torch.no_grad():
        return torch.cat([oracle.extract_x_vec(recs[2, s:s + n][None], p) for _, s, n in DOZEN.tolist()])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_many_segments_of_one_short_recording(models, recs, dozen_refs, precision):
    from xvector_amd import hip, plan_segment_calls
    m, bar = models[precision], BARS[precision]
    assert LENS[2] == 333
    x = recs[2:3].to(DEV)
    eng = m._engine(torch.device(DEV))
    base = m.extract_segments(x, DOZEN)
    assert_parity(base, dozen_refs, what=f"{precision} the dozen windows vs oracle", **bar)
    for n, (form, S) in MANY.items():
        idx = np.random.default_rng(n).permutation(np.arange(n) % len(DOZEN))
        seg = DOZEN[idx]
        calls = plan_segment_calls(seg, 262144)
        assert len(calls) == 1 and calls[0].pieces == [(0, 0, 333)], "the list is one call over the whole recording"
        got = m.extract_segments(x, seg)
        x3 = precision == "bf16" and form != "tile16"
        assert hip.affine_dispatch(eng.h)[0] == (form + "_bf16x3" if x3 else form, S), (n, hip.affine_dispatch(eng.h))
        assert got.shape == (n, 512)
        first = np.asarray([int(np.flatnonzero(idx == k)[0]) for k in range(len(DOZEN))])
        distinct = got[torch.from_numpy(first).to(DEV)]
        assert torch.equal(got, distinct[torch.from_numpy(idx).to(DEV)]), f"{n} segments: duplicates of a window give different rows"
        assert_parity(distinct, base, what=f"{precision} {n} segments vs the dozen windows alone", **bar)
