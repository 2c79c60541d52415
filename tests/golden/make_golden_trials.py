#!/usr/bin/env python3
"""Generate g8_trials.npz by running the REFERENCE's own trial collection (plda_score_stat.py:13-90).

Runs only where the reference checkout is present (as make_golden.py, whose stand-in technique for the third-party
packages that are not installed is reused here).  It imports the reference's `plda_score_stat`, gives `plda_classifier` a
plain stand-in for speechbrain's StatObject_SB and a `plda_scores` that returns this repo's oracle scores
(oracle/plda_oracle.py) for a seeded PLDA model, builds a small synthetic DataFrame in the layout the reference reads
(main.py:317-318) and a trial file, and runs the reference's `__init__` and `test_plda` unmodified.  Nothing of the
reference is copied: the fixture holds the inputs and what the reference's object held afterwards.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_trials.py

g8_trials.npz
  vectors [60, 16] float64, ids [60] (one id occurs twice), labels [60], the model (mean, F, Sigma), seeds
  trial_text       the trial file's text; labels spelt `1` / `0` and `1.0` / `0.0`, both of which the parser accepts
  positive_scores, negative_scores, positive_scores_mask, negative_scores_mask, checked_label, checked_xvec
                   the reference's attributes after test_plda
"""
import importlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

N_VEC, DIM, RANK, N_SPK, N_TRIALS = 60, 16, 6, 12, 300
SEED_MODEL, SEED_DATA = 8, 80


class _Stat:
    """The fields of StatObject_SB the path reads (plda_classifier.py:71-79)."""

    def __init__(self, modelset, segset, start, stop, stat0, stat1):
        self.modelset, self.segset, self.start, self.stop, self.stat0, self.stat1 = modelset, segset, start, stop, stat0, stat1


class _Scores:
    def __init__(self, modelset, segset, scoremat):
        self.modelset, self.segset, self.scoremat = modelset, segset, scoremat
        self.scoremask = np.ones(scoremat.shape, dtype=bool)


class _Plda:
    pass


def main_():
    assert os.path.isdir(mg.REF), "reference not present: fixtures can only be generated next to a reference checkout"
    mg.install_stubs()
    sys.path.insert(0, mg.REF)
    sys.path.insert(0, os.path.join(mg.REPO, "oracle"))
    import pandas as pd
    import plda_oracle as po
    pss = importlib.import_module("plda_score_stat")
    pc = importlib.import_module("plda_classifier")
    pc.StatObject_SB = _Stat

    def oracle_scores(plda, en_stat, te_stat):
        return _Scores(en_stat.modelset, te_stat.modelset,
                       po.fast_plda_scoring(en_stat.stat1, te_stat.stat1, plda.mean, plda.F, plda.Sigma))
    pc.plda_scores = oracle_scores

    plda = _Plda()
    plda.mean, plda.F, plda.Sigma = po.make_plda(DIM, RANK, seed=SEED_MODEL)
    rng = np.random.default_rng(SEED_DATA)
    spk = np.arange(N_VEC) % N_SPK
    centres = rng.normal(0, 1, (N_SPK, RANK)) @ plda.F.T
    # float32 values widened, printed by numpy and read back by the reference: what x_vector_test.csv holds
    vecs = (plda.mean + centres[spk] + 0.6 * rng.normal(0, 1, (N_VEC, DIM))).astype(np.float32).astype(np.float64)
    ids = [f"id{10270 + s}/{'abcdefghij'[i % 10]}x{i // 10}Q/{i:05d}.wav" for i, s in enumerate(spk)]
    ids[41] = ids[7]                      # one id occurs twice: the reference resolves it to its first position
    frame = pd.DataFrame({"index": np.arange(N_VEC), "id": ids, "label": spk, "xvector": [str(v) for v in vecs]})
    frame.columns = ["index", "id", "label", "xvector"]

    # trials between ids that occur once (the reference's .item() lookup refuses an id that occurs twice)
    usable = [i for i in range(N_VEC) if i not in (7, 41)]
    lines = []
    for t in range(N_TRIALS):
        a, b = rng.choice(usable, 2, replace=False)
        if t % 3 == 0:                    # a third of the trials same-speaker
            same = [j for j in usable if spk[j] == spk[a] and j != a]
            b = same[int(rng.integers(len(same)))]
        match = int(spk[a] == spk[b])
        label = (str(match), f"{match}.0")[t % 2]
        lines.append(f"{label} {ids[a]} {ids[b]}\n")
    trial_text = "".join(lines)

    obj = pss.plda_score_stat_object(frame)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "veri_test.txt")
        with open(path, "w") as f:
            f.write(trial_text)
        obj.test_plda(plda, path)
    assert len(obj.positive_scores) + len(obj.negative_scores) == N_TRIALS and len(obj.positive_scores) >= 50
    mg.save("g8_trials.npz", seed_model=SEED_MODEL, seed_data=SEED_DATA, vectors=vecs, read_vectors=np.asarray(obj.x_vec_test),
            ids=np.array(ids), labels=spk.astype(np.int64), mean=plda.mean, F=plda.F, Sigma=plda.Sigma,
            trial_text=np.array(trial_text), positive_scores=np.asarray(obj.positive_scores, dtype=np.float64),
            negative_scores=np.asarray(obj.negative_scores, dtype=np.float64),
            positive_scores_mask=np.asarray(obj.positive_scores_mask), negative_scores_mask=np.asarray(obj.negative_scores_mask),
            checked_label=np.asarray(obj.checked_label, dtype=np.int64), checked_xvec=np.asarray(obj.checked_xvec))


if __name__ == "__main__":
    main_()
