#!/usr/bin/env python3
"""Generate g9_augment.npz by running the REFERENCE's own Dataset.augment_data (dataset.py:185-396).

Runs only where the reference checkout is present (as make_golden.py, whose stand-ins for the third-party packages that are
not installed are reused).  `resampy.resample` becomes `np.asarray(x, float64)` (every clip is written at the data set's own
rate, so the reference's resampling would be the identity up to resampy's filter: that part stays unpinned);
`python_speech_features.mfcc` is not called on this path.  The script writes small wav trees in the layout the reference
globs (int16 clips under musan/{music,speech,noise}, float32 responses under RIRS_NOISES/simulated_rirs; clip lengths on
both sides of every crop length), builds `Dataset(sampling_rate=800, data_folder_path=tmp)`, replaces `dataset.random` by a
proxy around a seeded random.Random that records every draw, has `glob.glob` return its list sorted (os.listdir's order is
not defined), and calls the reference's `augment_data` unmodified for each of the five kinds on three integer-valued inputs
(as long as the crop, shorter: padded, longer: cropped at a drawn start).  Nothing of the reference is copied: the fixture
holds the inputs, the clips, the recorded draws and the reference's outputs.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_augment.py

g9_augment.npz
  samplerate 800, n 2400, kinds [5]
  pool int16 [R, m_max], pool_len [R], music_rows / speech_rows / noise_rows (pool rows in the reference's file order)
  rirs float32 [3, l_max], rir_len [3]
  inputs float64 [n_cases, n]   the input of every case AFTER the reference's crop / pad (case = kind-major, input-minor)
  case_kind [n_cases]           index into kinds
  draws int64 [n_draws, 5]      (case, call, a, b, result) in call order, the crop of the input left out:
                                call 0 = choice(seq): a = len(seq), result = the POOL ROW (or rir row) of the chosen file
                                call 1 = randint(a, b)
  outputs float64 [n_cases, n]  what augment_data returned
"""
import importlib
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

SR, N = 800, 2400
KINDS = ("none", "music", "speech", "noise", "rir")
SEED_DATA, SEED_DRAWS = 90, 9
MUSIC_LEN = (3000, 2000, 3500)            # one shorter than the 2400-sample crop
SPEECH_LEN = (2000, 2900, 3800, 2400)     # shorter, longer, exactly the crop
NOISE_LEN = (500, 900, 1300)              # around the 800-sample crop
RIR_LEN = (301, 1001, 1701)
INPUT_LEN = (2400, 2000, 2900)


class _Recorder:
    """What the reference calls on its `random`: choice and randint, recorded."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.calls = []

    def choice(self, seq):
        got = self.rng.choice(seq)
        self.calls.append(("choice", len(seq), 0, got))
        return got

    def randint(self, a, b):
        got = self.rng.randint(a, b)
        self.calls.append(("randint", a, b, got))
        return got


class _SortedGlob:
    def __init__(self, real):
        self._real = real

    def glob(self, pattern):
        return sorted(self._real.glob(pattern))


def main_():
    assert os.path.isdir(mg.REF), "reference not present: fixtures can only be generated next to a reference checkout"
    mg.install_stubs()
    sys.modules["resampy"].resample = lambda x, sr_orig, sr_new: np.asarray(x, dtype=np.float64)
    sys.path.insert(0, mg.REF)
    from scipy.io import wavfile
    dataset = importlib.import_module("dataset")
    dataset.glob = _SortedGlob(importlib.import_module("glob"))

    rng = np.random.default_rng(SEED_DATA)
    clips, row_of, groups = [], {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for kind, lens in (("music", MUSIC_LEN), ("speech", SPEECH_LEN), ("noise", NOISE_LEN)):
            groups[kind] = []
            for i, m in enumerate(lens):
                path = f"{tmp}/musan/{kind}/a/{kind[0]}{i}.wav"
                os.makedirs(os.path.dirname(path), exist_ok=True)
                clip = (rng.standard_normal(m) * 3000).astype(np.int16)
                wavfile.write(path, SR, clip)
                row_of[path] = len(clips)
                groups[kind].append(len(clips))
                clips.append(clip)
        rirs = []
        for i, m in enumerate(RIR_LEN):
            path = f"{tmp}/RIRS_NOISES/simulated_rirs/a/b/r{i}.wav"
            os.makedirs(os.path.dirname(path), exist_ok=True)
            h = (rng.standard_normal(m) * np.exp(-np.arange(m) / 60.0)).astype(np.float32)
            wavfile.write(path, SR, h)
            row_of[path] = i
            rirs.append(h)
        raw = [(rng.standard_normal(m) * 5000).astype(np.int16).astype(np.float64) for m in INPUT_LEN]

        ds = dataset.Dataset(sampling_rate=SR, data_folder_path=tmp)
        rec = _Recorder(SEED_DRAWS)
        dataset.random = rec
        inputs, outputs, case_kind, draws = [], [], [], []
        for k, kind in enumerate(KINDS):
            for x in raw:
                case = len(inputs)
                rec.calls.clear()
                y = ds.augment_data(x.copy(), kind)
                calls = list(rec.calls)
                if len(x) < 3 * SR:
                    cropped = np.pad(x, (0, 3 * SR - len(x)))
                else:                                  # the first draw is the crop of the input itself
                    name, a, b, start = calls.pop(0)
                    assert name == "randint" and (a, b) == (0, len(x) - 3 * SR)
                    cropped = x[start:start + 3 * SR]
                for name, a, b, got in calls:
                    draws.append((case, 0, a, b, row_of[got]) if name == "choice" else (case, 1, a, b, got))
                assert y.shape == (N,) and y.dtype == np.float64
                inputs.append(cropped)
                outputs.append(y)
                case_kind.append(k)

    m_max = max(len(c) for c in clips)
    pool = np.zeros((len(clips), m_max), dtype=np.int16)
    for r, c in enumerate(clips):
        pool[r, :len(c)] = c
    l_max = max(len(h) for h in rirs)
    rir_mat = np.zeros((len(rirs), l_max), dtype=np.float32)
    for r, h in enumerate(rirs):
        rir_mat[r, :len(h)] = h
    mg.save("g9_augment.npz", samplerate=np.int64(SR), n=np.int64(N), kinds=np.array(KINDS), seed_data=SEED_DATA,
            seed_draws=SEED_DRAWS, pool=pool, pool_len=np.array([len(c) for c in clips], dtype=np.int64),
            music_rows=np.array(groups["music"]), speech_rows=np.array(groups["speech"]), noise_rows=np.array(groups["noise"]),
            rirs=rir_mat, rir_len=np.array([len(h) for h in rirs], dtype=np.int64), inputs=np.array(inputs),
            case_kind=np.array(case_kind, dtype=np.int64), draws=np.array(draws, dtype=np.int64), outputs=np.array(outputs))


if __name__ == "__main__":
    main_()
