"""CPU-only checks of energy VAD and sliding CMVN (include/xvec_vad.h): the host-only plan (csrc/vad_plan.h) through its dump
program against the numpy restatement tests/vad_ref.py, the restatement's fixed-order threshold against an independent one
from math.fsum, the C ABI's argument errors (each returns before the library touches a device), the module's constants against
the header, `speech_runs` / `run_windows` on hand-made masks, and the error channel."""
import ctypes
import os
import re
import threading

import numpy as np
import pytest

import vad_ref
from conftest import ROOT
from hipcc_support import header_constants, host_program, needs_host_cxx

P = 0x1000          # a pointer that is never followed: every call here fails its argument checks first
NAN = float("nan")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return host_program("vad_plan_dump", tmp_path_factory.mktemp("vad_plan"))


# ---------------------------------------------------------------- the host-only plan against the restatement

@needs_host_cxx
def test_window_of_every_frame_equals_the_restatement_and_keeps_its_promises(plan):
    cases = [(L, w, m, c) for L in (1, 2, 3, 7, 16, 39) for w in (1, 2, 3, 7, 12, 24) for m in (1, 2, 5, 16, 29, 45)
             for c in (0, 1)]
    cases += [(700, 300, 100, 1), (700, 600, 100, 0), (299, 300, 100, 1), (301, 300, 400, 0)]
    got = plan([f"window {L} {w} {m} {c}" for L, w, m, c in cases])
    for (L, w, m, c), line in zip(cases, got):
        v = [int(x) for x in line.split()[1:]]
        lo, hi = np.array(v[0::2]), np.array(v[1::2])
        want = [vad_ref.window(t, L, w, m, bool(c)) for t in range(L)]
        assert list(zip(lo.tolist(), hi.tolist())) == want, (L, w, m, c)
        t = np.arange(L)
        assert (0 <= lo).all() and (lo <= t).all() and (t < hi).all() and (hi <= L).all(), (L, w, m, c)
        assert (hi - lo <= (w if c else max(w + 1, m))).all(), (L, w, m, c)
        # what the kernel's staging relies on: from t to t + 1 lo rises by 0 or 1 and hi never falls
        assert np.isin(np.diff(lo), (0, 1)).all() and (np.diff(hi) >= 0).all(), (L, w, m, c)


@needs_host_cxx
def test_tile_plan_layout_and_refusals_at_the_limits(plan):
    from xvector_amd import hip, vad
    budget, wmax = vad.LDS_BYTES, vad.MAX_WINDOW
    got = plan(["span off", "span 300 100 1", "span 300 100 0", "span 7 100 0", f"span {wmax} 1 0"])
    assert got == ["span 1", "span 300", "span 301", "span 100", f"span {wmax + 1}"]
    # the bench batch and the recipe's window: whole rows, the tallest tile
    assert plan(["tile 24 300"]) == [f"tile 256 24 555 {555 * 24 * 4} 26"]              # 10 runs of 26 frames
    # no normalisation: the tile's own rows
    assert plan(["tile 24 1", "tile 1 1"]) == [f"tile 256 24 256 {256 * 24 * 4} 26", "tile 256 1 256 1024 1"]
    # a window that whole rows cannot hold: the channels halve, never below GROUP_MIN
    assert plan(["tile 80 601"]) == [f"tile 256 10 856 {856 * 10 * 4} 11"]
    assert plan([f"tile {vad.MAX_CHANNELS} 601", "tile 24 1200"]) == [f"tile 256 16 856 {856 * 16 * 4} 16", f"tile 256 8 1455 {1455 * 8 * 4} 8"]
    # the largest window: the smallest tile of the smallest group, and one frame more is refused
    rows = vad.TILE_MIN - 1 + wmax + 1
    assert plan([f"tile 24 {wmax + 1}", f"tile 8 {wmax + 1}", f"tile 3 {wmax + 1}"]) == [
        f"tile {vad.TILE_MIN} 8 {rows} {rows * 32} 1", f"tile {vad.TILE_MIN} 8 {rows} {rows * 32} 1",
        f"tile 256 3 {255 + wmax + 1} {(255 + wmax + 1) * 12} 4"]
    assert rows * 32 <= budget < (2 * vad.TILE_MIN - 1 + wmax + 1) * 32
    over = budget // 32 - vad.TILE_MIN + 2
    assert plan([f"tile 24 {over}", f"tile 24 {over - 1}"]) == ["refused", f"tile {vad.TILE_MIN} 8 {budget // 32} {budget // 32 * 32} 1"]
    for C in (1, 5, 24, 80, 257, vad.MAX_CHANNELS):          # every plan inside the budget, tiles inside a chunk
        for s in (1, 2, 100, 301, 601, 1000, wmax + 1):
            f, ch, r, lds, run = (int(v) for v in plan([f"tile {C} {s}"])[0].split()[1:])
            assert lds == r * ch * 4 <= budget and r == f - 1 + s and vad.LANES % f == 0 and vad.TILE_MIN <= f <= vad.TILE_MAX
            assert min(C, vad.GROUP_MIN) <= ch <= C
            # the runs cover the tile, and the block has a thread per (channel, run) wherever the group fits it
            assert 1 <= run <= f and (ch > vad.LANES or -(-f // run) * ch <= vad.LANES)
            assert vad_ref.tile_plan(C, s) == (f, ch, run), (C, s)          # the restatement the GPU test's bound reads
    assert vad_ref.tile_plan(24, over) is None
    assert plan(["grid 256 299 24 300", "grid 3 513 80 601", "grid 1 1 1 1"]) == ["grid 512", f"grid {3 * 3 * 8}", "grid 1"]
    # the workspace: the leading counts of every chunk, then the counts, 256-byte aligned; what the library reports
    for B, T in ((1, 1), (3, 256), (3, 257), (300, 513), (64, 3000)):
        prefix, count, total = (int(v) for v in plan([f"layout {B} {T}"])[0].split()[1:])
        chunks = -(-T // vad.LANES)
        assert prefix == 0 and count % 256 == 0 and total % 256 == 0
        assert count >= 4 * B * chunks and total >= count + 4 * B and total < 4 * B * (chunks + 1) + 512
        assert hip.lib.xvec_vad_workspace_bytes(B, T) == total
    assert plan(["layout 0 5", "layout 5 0"]) == ["layout 0 0 0"] * 2
    assert hip.lib.xvec_vad_workspace_bytes(0, 5) == 0 and hip.lib.xvec_vad_workspace_bytes(5, -1) == 0
    got = plan(["shape 3 61 24 24 1464", "shape 3 61 24 23 1464", "shape 3 61 24 32 1943", "shape 3 61 24 32 1944", "shape 0 61 24 24 9999",
                f"shape 1 1 {vad.MAX_CHANNELS + 1} 2000 2000", "maskstride 60 61", "maskstride 61 61", "vad null",
                "vad 5 0.5 0.6 0 0 24", "vad nan 0.5 0.6 0 0 24", "vad 5 nan 0.6 0 0 24", "vad 5 0.5 1 0 0 24", "vad 5 0.5 0 0 0 24",
                "vad 5 0.5 nan 0 0 24", "vad 5 0.5 0.6 -1 0 24", "vad 5 0.5 0.6 0 24 24", "vad 5 0.5 0.6 0 -1 24",
                "cmvn 600 100", "cmvn 0 100", f"cmvn {wmax + 1} 100", "cmvn 600 0", f"cmvn 600 {wmax + 2}", f"cmvn {wmax} {wmax + 1}"])
    assert got == ["ok", "refused x: row stride 23 is smaller than C = 24",
                   "refused x: utterance stride 1943 is smaller than the 1944 floats of an utterance", "ok",
                   "refused B = 0, T = 61, C = 24: every one must be at least 1",
                   f"refused C = {vad.MAX_CHANNELS + 1} is over XVEC_VAD_MAX_CHANNELS = {vad.MAX_CHANNELS}",
                   "refused mask stride 60 is smaller than T = 61", "ok", "refused null pointer: vad options", "ok",
                   "refused energy_threshold or energy_mean_scale is NaN", "refused energy_threshold or energy_mean_scale is NaN",
                   "refused proportion_threshold = 1 must lie strictly between 0 and 1",
                   "refused proportion_threshold = 0 must lie strictly between 0 and 1",
                   "refused proportion_threshold = nan must lie strictly between 0 and 1",
                   "refused frames_context = -1 must not be negative", "refused energy_col = 24 must lie in 0 .. C - 1 = 23",
                   "refused energy_col = -1 must lie in 0 .. C - 1 = 23", "ok",
                   f"refused cmn_window = 0 must lie in 1 .. XVEC_CMVN_MAX_WINDOW = {wmax}",
                   f"refused cmn_window = {wmax + 1} must lie in 1 .. XVEC_CMVN_MAX_WINDOW = {wmax}",
                   f"refused min_window = 0 must lie in 1 .. XVEC_CMVN_MAX_WINDOW + 1 = {wmax + 1}",
                   f"refused min_window = {wmax + 2} must lie in 1 .. XVEC_CMVN_MAX_WINDOW + 1 = {wmax + 1}", "ok"]


# ---------------------------------------------------------------- the restatement against itself

def test_fixed_order_threshold_decides_as_the_fsum_threshold():
    """The decisions from the header's fixed-order sum equal those from the correctly rounded sum on every frame further than
    1e-9 max(1, |thr|) from the threshold -- and no frame of these utterances is that close (cap 0)."""
    rng = np.random.default_rng(7)
    opts = vad_ref.RECIPE_VAD
    for L in (1, 2, 5, 61, 299, 300, 301, 777):
        e = rng.normal(10.0, 3.0, L).astype(np.float32)
        thr, thr_f = vad_ref.threshold(e, **opts), vad_ref.threshold_fsum(e, **opts)
        assert abs(float(thr) - thr_f) <= (L // vad_ref.LANES + 12) * 2.0 ** -53 * abs(thr_f), (L, thr, thr_f)
        close = np.abs(e.astype(np.float64) - thr_f) <= 1e-9 * max(1.0, abs(thr_f))
        assert int(close.sum()) == 0, L
        hot = e.astype(np.float64) > thr
        assert np.array_equal(hot, e.astype(np.float64) > thr_f), L
        assert np.array_equal(vad_ref.decide(e, thr, **opts), vad_ref.decide(e, thr_f, **opts)), L
        share = hot.mean()
        print(f"[vad] L = {L}: thr {float(thr):.6f}, {100 * share:.0f} % hot")
        # thr is about 5.5 + 0.5 * 10, a sixth of a standard deviation above the mean: 43 % hot, to four binomial deviations
        assert share == 0 if L == 1 else L < 61 or abs(share - 0.43) <= 4 * (0.43 * 0.57 / L) ** 0.5, (L, share)


def test_restatement_rules_on_hand_written_energies():
    e = np.array([1, 9, 1, 1, 9, 9, 1, 1], dtype=np.float32)
    assert vad_ref.fixed_order_sum(e) == 32.0 and vad_ref.threshold(e, 5.0, 0.5) == 7.0
    assert vad_ref.threshold(e, 5.0, 0.0) == 5.0 and np.isnan(vad_ref.threshold(e[:0], 5.0, 0.5))
    hot = vad_ref.decide(e, 7.0, 0, 0.6)
    assert hot.tolist() == [0, 1, 0, 0, 1, 1, 0, 0]
    # context 1, half of the frames: the edges vote over two frames
    assert vad_ref.decide(e, 7.0, 1, 0.5).tolist() == [1, 0, 0, 0, 1, 1, 0, 0]
    # a tie: den = 4 at the right edge (t = 6, context 2 of 8 frames is 4 .. 7), num = 2 -> voiced at 0.5
    assert vad_ref.decide(e, 7.0, 2, 0.5)[6] == 1 and vad_ref.decide(e, 7.0, 2, 0.51)[6] == 0
    # strict: a frame AT the threshold is cold; NaN is cold, and a NaN threshold makes nothing hot
    assert vad_ref.decide(e, 9.0, 0, 0.6).sum() == 0
    assert vad_ref.decide(np.array([NAN, 9], np.float32), 7.0, 0, 0.6).tolist() == [0, 1]
    assert vad_ref.decide(e, NAN, 0, 0.6).sum() == 0
    y, bound = vad_ref.sliding_cmvn(np.arange(12, dtype=np.float32).reshape(6, 2), cmn_window=3, min_window=1, center=True)
    assert np.array_equal(y[:, 0].astype(np.float64), [-2, 0, 0, 0, 0, 2]) and (bound < 1e-14).all()
    y, _ = vad_ref.sliding_cmvn(np.full((5, 1), 1.5, np.float32), cmn_window=2, min_window=1, norm_vars=True)
    assert (y == 0).all()                              # n = 1 at t = 0, a constant channel behind it: the floor, and 0 / floor


# ---------------------------------------------------------------- the header, the module and the C ABI without a device

def test_module_restates_the_header_constants_and_refuses_the_cpu():
    import torch
    import xvector_amd
    from xvector_amd import hip, vad
    hdr = open(os.path.join(ROOT, "include", "xvec_vad.h")).read()
    consts = header_constants("xvec_vad.h", "XVEC_")
    assert consts == {"VAD_LANES": vad.LANES, "VAD_MAX_CHANNELS": vad.MAX_CHANNELS, "CMVN_MAX_WINDOW": vad.MAX_WINDOW,
                      "CMVN_TILE_MAX": vad.TILE_MAX, "CMVN_TILE_MIN": vad.TILE_MIN, "CMVN_GROUP_MIN": vad.GROUP_MIN,
                      "CMVN_LDS_BYTES": vad.LDS_BYTES}
    assert vad.LANES == vad_ref.LANES and vad.VAD_DEFAULTS == vad_ref.VAD_DEFAULTS
    # the structs, field by field in the header's order
    for name, cls in (("xvec_vad_options", hip.VadOptions), ("xvec_cmvn_options", hip.CmvnOptions)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        fields = re.findall(r"^\s*(double|int32_t) (\w+);", body, re.M)
        assert [(n, {"double": ctypes.c_double, "int32_t": ctypes.c_int32}[t]) for t, n in fields] == cls._fields_
    exports = {"xvec_vad_last_error", "xvec_vad_workspace_bytes", "xvec_vad_energy", "xvec_cmvn_sliding", "xvec_vad_cmvn"}
    assert exports <= set(hip.EXPORTS) and all(hasattr(hip.lib, n) for n in exports)
    for name in ("VadCmvn", "energy_vad", "sliding_cmvn", "select_voiced", "speech_runs", "run_windows"):
        assert getattr(xvector_amd, name) is getattr(vad, name) and name in xvector_amd.__all__
    cpu = torch.zeros(2, 20, 4)
    for call in (lambda: vad.energy_vad(cpu), lambda: vad.sliding_cmvn(cpu), lambda: vad.VadCmvn()(cpu),
                 lambda: vad.select_voiced(cpu, torch.ones(2, 20, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()
    with pytest.raises(TypeError, match="unknown VAD option"):
        vad.VadCmvn(vad=dict(energy_treshold=5.0))
    with pytest.raises(TypeError, match="unknown CMVN option"):
        vad.sliding_cmvn(cpu, window=3)
    with pytest.raises(TypeError, match="frontend must be a vad.VadCmvn"):
        xvector_amd.Diarizer(None, "cosine", threshold=0.0, frontend=object())
    assert vad.VadCmvn(select=True).with_select(False).select is False


def test_c_abi_argument_errors_return_before_any_device_call():
    from xvector_amd import hip, vad
    lib, err = hip.lib, lambda: hip.lib.xvec_vad_last_error().decode()
    B, T, C = 3, 61, 24
    need = lib.xvec_vad_workspace_bytes(B, T)
    good = dict(x=P, B=B, T=T, C=C, rs=C, us=T * C, lengths=None, vad=hip.VadOptions(5.0, 0.5, 0.6, 0, 0),
                cmvn=hip.CmvnOptions(600, 100, 0, 0), select=1, mask=P, ms=T, counts=P, thr=None, y=P, yrs=C, yus=T * C,
                new_len=P, ws=P, ws_bytes=need)

    def energy(a):
        return lib.xvec_vad_energy(*[a[k] for k in ("x", "B", "T", "C", "rs", "us", "lengths", "vad", "mask", "ms", "counts", "thr")],
                                   None)

    def sliding(a):
        return lib.xvec_cmvn_sliding(*[a[k] for k in ("x", "B", "T", "C", "rs", "us", "lengths", "cmvn", "mask", "ms", "y", "yrs",
                                                      "yus", "new_len", "ws", "ws_bytes")], None)

    def fused(a):
        return lib.xvec_vad_cmvn(*[a[k] for k in ("x", "B", "T", "C", "rs", "us", "lengths", "vad", "cmvn", "select", "mask", "ms",
                                                  "counts", "thr", "y", "yrs", "yus", "new_len", "ws", "ws_bytes")], None)

    V, W = hip.VadOptions, hip.CmvnOptions
    shape = [
        (dict(B=0), hip.ERR_ARG, "B = 0, T = 61, C = 24: every one must be at least 1"),
        (dict(T=-1), hip.ERR_ARG, "B = 3, T = -1, C = 24: every one must be at least 1"),
        (dict(C=0), hip.ERR_ARG, "B = 3, T = 61, C = 0: every one must be at least 1"),
        (dict(C=vad.MAX_CHANNELS + 1, rs=4096, us=61 * 4096), hip.ERR_ARG,
         f"C = {vad.MAX_CHANNELS + 1} is over XVEC_VAD_MAX_CHANNELS = {vad.MAX_CHANNELS}"),
        (dict(rs=23), hip.ERR_ARG, "x: row stride 23 is smaller than C = 24"),
        (dict(us=T * C - 1), hip.ERR_ARG, f"x: utterance stride {T * C - 1} is smaller than the {T * C} floats of an utterance"),
    ]
    decide = [
        (dict(vad=None), hip.ERR_ARG, "null pointer: vad options"),
        (dict(vad=V(NAN, 0.5, 0.6, 0, 0)), hip.ERR_ARG, "energy_threshold or energy_mean_scale is NaN"),
        (dict(vad=V(5.0, NAN, 0.6, 0, 0)), hip.ERR_ARG, "energy_threshold or energy_mean_scale is NaN"),
        (dict(vad=V(5.0, 0.5, 0.0, 0, 0)), hip.ERR_ARG, "proportion_threshold = 0 must lie strictly between 0 and 1"),
        (dict(vad=V(5.0, 0.5, 1.0, 0, 0)), hip.ERR_ARG, "proportion_threshold = 1 must lie strictly between 0 and 1"),
        (dict(vad=V(5.0, 0.5, 0.6, -2, 0)), hip.ERR_ARG, "frames_context = -2 must not be negative"),
        (dict(vad=V(5.0, 0.5, 0.6, 0, C)), hip.ERR_ARG, f"energy_col = {C} must lie in 0 .. C - 1 = {C - 1}"),
        (dict(vad=V(5.0, 0.5, 0.6, 0, -1)), hip.ERR_ARG, f"energy_col = -1 must lie in 0 .. C - 1 = {C - 1}"),
        (dict(ms=T - 1), hip.ERR_ARG, f"mask stride {T - 1} is smaller than T = {T}"),
        (dict(x=None), hip.ERR_ARG, "null pointer: x / mask / counts"),
        (dict(mask=None), hip.ERR_ARG, "null pointer: x / mask / counts"),
        (dict(counts=None), hip.ERR_ARG, "null pointer: x / mask / counts"),
    ]
    normalise = [
        (dict(yrs=23), hip.ERR_ARG, "y: row stride 23 is smaller than C = 24"),
        (dict(yus=T * C - 1), hip.ERR_ARG, f"y: utterance stride {T * C - 1} is smaller than the {T * C} floats of an utterance"),
        (dict(cmvn=W(0, 100, 0, 0)), hip.ERR_ARG, f"cmn_window = 0 must lie in 1 .. XVEC_CMVN_MAX_WINDOW = {vad.MAX_WINDOW}"),
        (dict(cmvn=W(vad.MAX_WINDOW + 1, 100, 0, 0)), hip.ERR_ARG,
         f"cmn_window = {vad.MAX_WINDOW + 1} must lie in 1 .. XVEC_CMVN_MAX_WINDOW = {vad.MAX_WINDOW}"),
        (dict(cmvn=W(600, 0, 0, 0)), hip.ERR_ARG, f"min_window = 0 must lie in 1 .. XVEC_CMVN_MAX_WINDOW + 1 = {vad.MAX_WINDOW + 1}"),
        (dict(y=None), hip.ERR_ARG, "null pointer: x / y"),
        (dict(ws=None), hip.ERR_ARG, "null pointer: workspace"),
        (dict(ws_bytes=need - 1), hip.ERR_WORKSPACE, f"workspace too small: {need - 1} < {need} bytes"),
    ]
    for entry, cases in ((energy, shape + decide), (sliding, shape + normalise), (fused, shape + decide + normalise)):
        for kwargs, code, text in cases:
            assert entry({**good, **kwargs}) == code, (entry.__name__, kwargs)
            assert err() == text, (entry.__name__, kwargs)
    assert sliding({**good, "x": None}) == hip.ERR_ARG and err() == "null pointer: x / y"
    assert sliding({**good, "ms": T - 1}) == hip.ERR_ARG and err() == f"mask stride {T - 1} is smaller than T = {T}"
    assert sliding({**good, "new_len": None}) == hip.ERR_ARG and err() == "null pointer: new_lengths (optional only without a mask)"


def test_vad_error_channel_is_its_own_and_per_thread():
    from xvector_amd import hip
    lib = hip.lib
    assert lib.xvec_mfcc_create(None, None) == hip.ERR_ARG
    assert lib.xvec_vad_energy(None, 0, 1, 1, 1, 1, None, None, None, 1, None, None, None) == hip.ERR_ARG
    want = "B = 0, T = 1, C = 1: every one must be at least 1"
    assert lib.xvec_vad_last_error().decode() == want and lib.xvec_mfcc_last_error().decode() == "null argument"
    assert lib.xvec_mfcc_create(None, None) == hip.ERR_ARG               # a later MFCC error leaves the VAD text alone
    assert lib.xvec_vad_last_error().decode() == want
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.xvec_vad_last_error().decode()))
    t.start()
    t.join()
    assert seen == [""] and lib.xvec_vad_last_error().decode() == want


# ---------------------------------------------------------------- speech runs and the windows inside them

def test_speech_runs_close_gaps_before_they_drop_short_runs():
    from xvector_amd.vad import speech_runs
    m = np.zeros((3, 40), dtype=np.uint8)
    m[0, 0:10] = 1            # a run at the utterance's start ...
    m[0, 12:20] = 1           # ... a gap of 2 ...
    m[0, 30:40] = 1           # ... and a run up to its end
    m[2, 5:9] = 1
    assert speech_runs(m, min_len=1).tolist() == [[0, 0, 10], [0, 12, 8], [0, 30, 10], [2, 5, 4]]
    assert speech_runs(m, min_len=9).tolist() == [[0, 0, 10], [0, 30, 10]]
    # gaps close FIRST: 10 + 2 + 8 = 20 frames survive min_len = 15, which neither part does alone
    assert speech_runs(m, max_gap=2, min_len=15).tolist() == [[0, 0, 20]]
    assert speech_runs(m, max_gap=1, min_len=15).tolist() == []
    assert speech_runs(m, max_gap=10, min_len=1).tolist() == [[0, 0, 40], [2, 5, 4]]
    # the lengths cut a run; frames at or past them never count, whatever the mask holds
    assert speech_runs(m, [35, 40, 7], min_len=1).tolist() == [[0, 0, 10], [0, 12, 8], [0, 30, 5], [2, 5, 2]]
    assert speech_runs(m, [0, 0, 0], min_len=1).shape == (0, 3)
    empty = speech_runs(np.zeros((2, 9), dtype=np.uint8))
    assert empty.shape == (0, 3) and empty.dtype == np.int32
    assert speech_runs(np.ones((1, 20), dtype=bool)).tolist() == [[0, 0, 20]]
    with pytest.raises(ValueError, match="lengths has 2 entries"):
        speech_runs(m, [1, 2])


def test_run_windows_are_sliding_windows_inside_every_run():
    from xvector_amd.vad import run_windows
    runs = [(0, 100, 400), (0, 700, 150), (2, 10, 149), (2, 500, 240)]
    w = run_windows(runs, 150, 75)
    assert w.dtype == np.int32
    assert w.tolist() == [[0, 100, 150], [0, 175, 150], [0, 250, 150], [0, 325, 150], [0, 700, 150], [2, 500, 150], [2, 575, 150]]
    # a tail: the frames past the last full window, and a run shorter than a window as one window
    w = run_windows(runs, 150, 75, min_tail=20)
    assert w.tolist() == [[0, 100, 150], [0, 175, 150], [0, 250, 150], [0, 325, 150], [0, 400, 100], [0, 700, 150], [2, 10, 149],
                          [2, 500, 150], [2, 575, 150], [2, 650, 90]]
    for u, s, n in w.tolist():                               # every window inside one of the runs
        assert any(u == ru and rs <= s and s + n <= rs + rn for ru, rs, rn in runs)
    assert run_windows(np.zeros((0, 3), dtype=np.int32), 150, 75).shape == (0, 3)
    assert run_windows([(1, 0, 100)], 150, 75).shape == (0, 3)
