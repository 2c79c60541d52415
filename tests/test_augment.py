"""Waveform augmentation, the parts that need no GPU: tests/augment_ref.py against the reference's own run
(tests/golden/g9_augment.npz, made by make_golden_augment.py), AugmentPlan.draw fed the reference's recorded draws, the C ABI's
argument errors through ctypes (return code, message, a channel of its own), and the header <-> export agreement.

Bars.  mix and normalize: bit for bit (augment_ref makes the reference's float64 operations in the reference's order).
reverb: 1e-12 of the peak with augment_ref's `fft` form (scipy's fftconvolve on the float32 response, as the reference calls
it); the exact float64 convolution, which the kernels are held to, is checked against the fixture at a bar derived from the
reference's own single-precision transform of that response (it measures 3e-8 of the peak)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import augment_ref as ar
from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def g9():
    return load_golden("g9_augment.npz")


class _Replay:
    """A `random` that hands out recorded draws and insists on being asked for exactly them, in order."""

    def __init__(self, draws):
        self.draws = [tuple(int(v) for v in d) for d in draws]

    def choice(self, seq):
        _, call, a, _, got = self.draws.pop(0)
        assert call == 0 and a == len(seq) and got in list(seq), (call, a, len(seq))
        return got

    def randint(self, lo, hi):
        _, call, a, b, got = self.draws.pop(0)
        assert call == 1 and (a, b) == (lo, hi), (call, a, b, lo, hi)
        return got


def _plan_of_case(g9, case):
    from xvector_amd.augment import AugmentPlan
    kind = str(g9["kinds"][int(g9["case_kind"][case])])
    rng = _Replay(g9["draws"][g9["draws"][:, 0] == case])
    plan = AugmentPlan.draw([kind], int(g9["n"]), g9["music_rows"], g9["speech_rows"], g9["noise_rows"], len(g9["rir_len"]),
                            samplerate=int(g9["samplerate"]), rng=rng, pool_len=g9["pool_len"])
    assert rng.draws == [], f"case {case} ({kind}): {len(rng.draws)} recorded draws were not asked for"
    return kind, plan


def _ref_of_case(g9, case, plan, fft=True):
    x = g9["inputs"][case][None]
    y, gains = ar.mix(x, g9["pool"], g9["pool_len"], plan.ops, plan.srcs)
    y = ar.reverb(y, g9["rirs"], g9["rir_len"], plan.rir_index, fft=fft)
    return ar.normalize(y)[0], gains


def test_fixture_covers_the_kinds_and_both_crop_sides(g9):
    assert list(g9["kinds"]) == ["none", "music", "speech", "noise", "rir"]
    assert sorted(set(g9["case_kind"].tolist())) == [0, 1, 2, 3, 4]
    n, sr = int(g9["n"]), int(g9["samplerate"])
    assert g9["inputs"].shape == g9["outputs"].shape == (15, n)
    lens = g9["pool_len"]
    for rows, crop in ((g9["music_rows"], n), (g9["speech_rows"], n), (g9["noise_rows"], sr)):
        assert lens[rows].min() < crop < lens[rows].max()          # padded clips and cropped clips
    assert np.array_equal(g9["inputs"], np.trunc(g9["inputs"]))    # integer-valued inputs
    assert g9["outputs"].min() == 0.0 and g9["outputs"].max() == 1.0


def test_planner_and_reference_arithmetic_reproduce_the_reference(g9):
    """AugmentPlan.draw, fed the draws the reference made, asks for exactly those draws and yields ops with which
    augment_ref reproduces what the reference returned."""
    n, sr = int(g9["n"]), int(g9["samplerate"])
    seen = set()
    for case in range(len(g9["inputs"])):
        kind, plan = _plan_of_case(g9, case)
        seen.add(kind)
        n_ops = {"none": 0, "music": 1, "speech": 1, "noise": 3, "rir": 0}[kind]
        assert len(plan.ops) == n_ops and (plan.rir_index[0] >= 0) == (kind == "rir")
        if kind == "noise":
            assert plan.ops["offset"].tolist() == [0, 1, 2] and plan.ops["length"].tolist() == [sr] * 3
            assert plan.ops["n_src"].tolist() == [1, 1, 1]
        elif n_ops:
            assert plan.ops["offset"].tolist() == [0] and plan.ops["length"].tolist() == [n]
            assert (kind == "music" and plan.ops["n_src"][0] == 1) or (kind == "speech" and 3 <= plan.ops["n_src"][0] <= 7)
        assert np.array_equal(plan.ops["snr_ratio"], [10 ** (s / 10) for s in plan.snr_db.tolist()])
        got, _ = _ref_of_case(g9, case, plan)
        want = g9["outputs"][case]
        if kind == "rir":
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (case, np.abs(got - want).max())
            # ... and the exact convolution, which the kernels are checked against, within the reference's OWN error: it
            # transforms the float32 response in single precision.  |x * dh| <= |x|_2 |dh|_2 with |dh|_2 <= log2(N) 2^-24 |h|_2
            # for an N-point FFT; that error E of c enters y = x + c s three times at most (c itself, the peak in s twice
            # over, |c| <= peak), and an error d of y enters (y - min) / (max - min) four times at most (y, min, and the
            # range twice over a value <= 1).
            x, h = g9["inputs"][case], g9["rirs"][plan.rir_index[0]][:g9["rir_len"][plan.rir_index[0]]].astype(np.float64)
            c = ar.conv_full(x, h)
            E = np.log2(2 ** np.ceil(np.log2(c.size))) * 2.0 ** -24 * np.linalg.norm(x) * np.linalg.norm(h)
            y = x + c[:x.size] * (np.abs(x).max() / np.abs(c).max())
            bar = 4 * 3 * E * (np.abs(x).max() / np.abs(c).max()) / (y.max() - y.min())
            exact, _ = _ref_of_case(g9, case, plan, fft=False)
            print(f"case {case}: exact convolution vs the reference {np.abs(exact - want).max():.3e}, bar {bar:.3e}")
            assert np.abs(exact - want).max() <= bar, (case, np.abs(exact - want).max(), bar)
        else:
            assert np.array_equal(got, want), (case, kind, np.abs(got - want).max())
    assert seen == {"none", "music", "speech", "noise", "rir"}


def test_planner_with_a_seeded_random_and_offsets_in_seconds(g9):
    import random
    from xvector_amd.augment import AugmentPlan
    kinds = ["noise", "none", "speech", "rir", "music"]
    args = (kinds, 2400, g9["music_rows"], g9["speech_rows"], g9["noise_rows"], 3)
    a = AugmentPlan.draw(*args, samplerate=800, rng=random.Random(3), pool_len=g9["pool_len"])
    b = AugmentPlan.draw(*args, samplerate=800, rng=random.Random(3), pool_len=g9["pool_len"])
    s = AugmentPlan.draw(*args, samplerate=800, rng=random.Random(3), pool_len=g9["pool_len"], noise_offsets="seconds")
    assert np.array_equal(a.ops, b.ops) and np.array_equal(a.srcs, b.srcs)
    assert a.ops["utt"].tolist() == sorted(a.ops["utt"].tolist()) and len(a) == 5
    assert a.ops["offset"][:3].tolist() == [0, 1, 2] and s.ops["offset"][:3].tolist() == [0, 800, 1600]
    assert a.rir_index.tolist()[:3] == [-1, -1, -1] and 0 <= a.rir_index[3] < 3 and a.rir_index[4] == -1
    for o in a.ops:                                              # every crop start keeps the clip inside its length
        for src in a.srcs[o["first_src"]:o["first_src"] + o["n_src"]]:
            have = g9["pool_len"][src["row"]]
            assert src["start"] == 0 if have < o["length"] else src["start"] + o["length"] <= have
    with pytest.raises(ValueError):
        AugmentPlan.draw(["echo"], 2400, [0], [0], [0], 1, pool_len=[10])
    with pytest.raises(ValueError):
        AugmentPlan.draw(["noise"], 801, [0], [0], [0], 1, samplerate=800, pool_len=[10])


# ---------------------------------------------------------------- the C ABI without a device

def _header_functions(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(xvec_[a-z_0-9]+)\s*\(", src)))


def test_header_and_binding_agree_on_the_augment_symbols():
    from xvector_amd import hip
    declared = _header_functions(os.path.join(ROOT, "include", "xvec_augment.h"))
    assert declared == ["xvec_aug_last_error", "xvec_aug_mix", "xvec_aug_mix_workspace_bytes", "xvec_aug_normalize",
                        "xvec_aug_reverb", "xvec_aug_reverb_workspace_bytes"]
    assert sorted(n for n in hip.EXPORTS if n.startswith("xvec_aug_")) == declared
    lib = C.CDLL(hip.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name


def test_record_layouts_match_the_header():
    from xvector_amd import augment
    assert augment.OP_DTYPE.itemsize == 32 and augment.OP_DTYPE.fields["snr_ratio"][1] == 24
    assert augment.SRC_DTYPE.itemsize == 8


def _ops(*rows):
    from xvector_amd.augment import OP_DTYPE
    return np.array([(u, off, ln, f, k, 0, r) for u, off, ln, f, k, r in rows], dtype=OP_DTYPE)


def test_argument_errors_without_gpu():
    """Every refusal below happens before the library touches a device; `one` stands in for device pointers."""
    from xvector_amd import hip
    L = hip.lib
    err = lambda: L.xvec_aug_last_error().decode()
    one = 256
    assert L.xvec_aug_mix_workspace_bytes(0, 100, 1) == 0 and L.xvec_aug_mix_workspace_bytes(2, 0, 1) == 0
    assert L.xvec_aug_mix_workspace_bytes(2, 100, -1) == 0 and L.xvec_aug_reverb_workspace_bytes(2, 100, 0) == 0
    need = L.xvec_aug_mix_workspace_bytes(2, 100, 3)
    assert need >= 2 * 100 * 8 + 3 * 32
    rneed = L.xvec_aug_reverb_workspace_bytes(2, 100, 50)
    assert rneed >= 2 * 100 * 4 + 2 * 4

    def mix(waves=one, ld=100, batch=2, n=100, pool=one, dtype=0, n_rows=4, m_max=64, src_len=one, ops=None, srcs=one,
            n_srcs=5, gains=one, status=one, ws=one, ws_bytes=need):
        ops = _ops((0, 0, 100, 0, 1, 2.0)) if ops is None else ops
        return L.xvec_aug_mix(waves, ld, batch, n, pool, dtype, n_rows, m_max, src_len, ops.ctypes.data_as(C.c_void_p), len(ops),
                              srcs, n_srcs, gains, status, ws, ws_bytes, None)

    assert mix(waves=None) == hip.ERR_ARG and "null pointer: waves" in err()
    assert mix(pool=None) == hip.ERR_ARG and "null pointer" in err()
    assert mix(gains=None) == hip.ERR_ARG and "gains_out" in err()
    assert mix(n=0) == hip.ERR_ARG and "n = 0: need at least one sample" in err()
    assert mix(batch=0) == hip.ERR_ARG and "batch = 0" in err()
    assert mix(ld=99) == hip.ERR_ARG and "ld = 99 is smaller than n = 100" in err()
    assert mix(dtype=7) == hip.ERR_ARG and "pool_dtype = 7" in err()
    assert mix(n=2 ** 28 + 1, ld=2 ** 28 + 1) == hip.ERR_TOO_LARGE
    assert mix(ops=_ops((0, 1, 100, 0, 1, 2.0))) == hip.ERR_ARG and "op 0: the slice [1, 101) leaves the row of 100" in err()
    assert mix(ops=_ops((0, -1, 10, 0, 1, 2.0))) == hip.ERR_ARG and "leaves the row" in err()
    assert mix(ops=_ops((0, 0, 0, 0, 1, 2.0))) == hip.ERR_ARG and "leaves the row" in err()
    assert mix(ops=_ops((2, 0, 100, 0, 1, 2.0))) == hip.ERR_ARG and "utt = 2 is outside the batch of 2" in err()
    assert mix(ops=_ops((1, 0, 100, 0, 1, 2.0), (0, 0, 100, 0, 1, 2.0))) == hip.ERR_ARG and "not sorted by utterance" in err()
    assert mix(ops=_ops((0, 0, 100, 3, 3, 2.0))) == hip.ERR_ARG and "sources [3, 6) lie outside the source list of 5" in err()
    assert mix(ops=_ops((0, 0, 100, 0, 1, 0.0))) == hip.ERR_ARG and "snr_ratio" in err()
    assert mix(ws_bytes=need - 1) == hip.ERR_WORKSPACE and "workspace too small" in err()
    assert mix(ws=None) == hip.ERR_ARG

    def reverb(waves=one, ld=100, batch=2, n=100, rirs=one, n_rirs=3, l_max=50, rir_len=one, idx=one, status=one, ws=one,
               ws_bytes=rneed):
        return L.xvec_aug_reverb(waves, ld, batch, n, rirs, n_rirs, l_max, rir_len, idx, status, ws, ws_bytes, None)

    assert reverb(waves=None) == hip.ERR_ARG and "null pointer: waves" in err()
    assert reverb(idx=None) == hip.ERR_ARG and "rir_of_utt" in err()
    assert reverb(n=0) == hip.ERR_ARG and reverb(n_rirs=0) == hip.ERR_ARG and reverb(l_max=0) == hip.ERR_ARG
    assert reverb(l_max=2 ** 24 + 1) == hip.ERR_TOO_LARGE
    assert reverb(ws_bytes=rneed - 1) == hip.ERR_WORKSPACE and "workspace too small" in err()
    assert L.xvec_aug_normalize(None, 100, 2, 100, None) == hip.ERR_ARG and "null pointer: waves" in err()
    assert L.xvec_aug_normalize(one, 100, 2, 0, None) == hip.ERR_ARG
    assert L.xvec_aug_normalize(one, 50, 2, 100, None) == hip.ERR_ARG and "ld = 50" in err()


def test_error_channel_is_its_own():
    """The augment unit's message lives apart from the four other channels (csrc/host_support.h: one ErrorChannel per unit)."""
    from xvector_amd import hip
    L = hip.lib
    assert L.xvec_eval_trials(None, 0, 0, 0, None, None, None, 0, 1.0, 1.0, 0.5, None, None, 0, None) == hip.ERR_ARG
    assert L.xvec_mfcc_create(None, None) == hip.ERR_ARG
    assert L.xvec_gemm_nt_f64(None, 0, None, 0, -1, 0, 1, None, None, 0.0, 1.0, None, 0, None) == hip.ERR_ARG
    assert L.xvec_plda_stats(None, hip.PLDA_X_F64, 1, 4, None, None, 1, 1.0, None, None, None, None, None, None, 0,
                             None) == hip.ERR_ARG
    others = {f: getattr(L, f)().decode() for f in ("xvec_eval_last_error", "xvec_mfcc_last_error", "xvec_score_last_error",
                                                    "xvec_plda_last_error", "xvec_last_error")}
    assert L.xvec_aug_normalize(None, 1, 1, 1, None) == hip.ERR_ARG
    assert L.xvec_aug_last_error().decode() == "null pointer: waves"
    for f, text in others.items():
        assert getattr(L, f)().decode() == text and text != "null pointer: waves", f


def test_no_cpu_path():
    import torch
    from xvector_amd.augment import WaveAugmenter
    with pytest.raises(RuntimeError):
        WaveAugmenter(device="cpu")
