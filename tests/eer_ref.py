"""CPU oracles for the trial evaluation (xvector_amd.evaluate).  TEST INFRASTRUCTURE ONLY; a plain module like plda_em_ref.py.

PARITY UNPINNED against the package: the reference calls speechbrain.utils.metric_stats.EER / minDCF (speechbrain==0.5.12,
plda_score_stat.py:8, 96-97) on float32 tensors; the package is not installed here.  `naive` restates its published threshold
walk literally, in float32: candidate thresholds = the sorted unique scores plus the midpoints of neighbours,
FRR = (pos <= t).sum() / P and FAR = (neg > t).sum() / N as float32 quotients, the first strict minimum of |FAR - FRR| wins
(EER = (FAR + FRR) / 2), minDCF = min of c_miss FRR p_target + c_fa FAR (1 - p_target), first minimum.  `by_sort` is the
formulation the kernels use (sorted distinct scores, cumulative counts, exact rates) in numpy float64 / int64, for sizes the
walk cannot do; tests/test_evaluate.py ties the two together and `by_sort` to sklearn's roc_curve.
"""
from collections import namedtuple

import numpy as np
import torch

Result = namedtuple("Result", "eer eer_th far frr min_dcf min_dcf_th eer_gap")


def _f32(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64)).to(torch.float32)


def _thresholds(pos, neg):
    th, _ = torch.sort(torch.cat([pos, neg]))
    th = torch.unique(th)
    mid = (th[0:-1] + th[1:]) / 2
    th, _ = torch.sort(torch.cat([th, mid]))
    return th


def _rates(pos, neg, th, chunk=2048):
    """float32 FRR, FAR of every threshold (the package's quotients), thresholds in chunks to bound memory."""
    frr = torch.empty(th.numel(), dtype=torch.float32)
    far = torch.empty(th.numel(), dtype=torch.float32)
    for a in range(0, th.numel(), chunk):
        t = th[a:a + chunk]
        frr[a:a + chunk] = (pos[:, None] <= t[None, :]).sum(0).float() / pos.shape[0]
        far[a:a + chunk] = (neg[:, None] > t[None, :]).sum(0).float() / neg.shape[0]
    return frr, far


def naive(pos, neg, c_miss=1.0, c_fa=1.0, p_target=0.5):
    pos, neg = _f32(pos), _f32(neg)
    th = _thresholds(pos, neg)
    frr, far = _rates(pos, neg, th)
    min_index, final_frr, final_far = 0, 0, 0
    gap = (far - frr).abs().tolist()
    frr_l, far_l = frr.tolist(), far.tolist()
    for i in range(th.numel()):
        if gap[i] < abs(final_far - final_frr) or i == 0:
            min_index, final_frr, final_far = i, frr_l[i], far_l[i]
    c_det = (c_miss * frr * p_target + c_fa * far * (1 - p_target)).numpy()
    k = int(np.argmin(c_det))           # the first minimum
    return Result((final_far + final_frr) / 2, float(th[min_index]), final_far, final_frr, float(c_det[k]), float(th[k]),
                  abs(final_far - final_frr))


def naive_objectives_at(pos, neg, th, c_miss=1.0, c_fa=1.0, p_target=0.5):
    """(|FAR - FRR|, detection cost) of the walk at the threshold `th`, in its float32 arithmetic."""
    pos, neg = _f32(pos), _f32(neg)
    frr, far = _rates(pos, neg, torch.tensor([th], dtype=torch.float32))
    return float((far - frr).abs()[0]), float((c_miss * frr * p_target + c_fa * far * (1 - p_target))[0])


def curves(pos, neg):
    """(u, tp, fa): the distinct float32 scores in ascending order, targets <= u_k, non-targets > u_k (int64)."""
    with np.errstate(over="ignore"):
        pos = np.asarray(pos, dtype=np.float64).astype(np.float32) + np.float32(0.0)
        neg = np.asarray(neg, dtype=np.float64).astype(np.float32) + np.float32(0.0)
    s = np.concatenate([pos, neg])
    is_t = np.concatenate([np.ones(pos.size, dtype=np.int64), np.zeros(neg.size, dtype=np.int64)])
    order = np.argsort(s, kind="stable")
    s, is_t = s[order], is_t[order]
    last = np.r_[s[1:] != s[:-1], True]
    tp = np.cumsum(is_t)[last]
    nn = np.cumsum(1 - is_t)[last]
    return s[last], tp, neg.size - nn


def by_sort(pos, neg, c_miss=1.0, c_fa=1.0, p_target=0.5):
    u, tp, fa = curves(pos, neg)
    P, N = int(np.size(pos)), int(np.size(neg))
    k = int(np.argmin(np.abs(fa * P - tp * N)))          # exact integers, the first minimum
    frr, far = tp / P, fa / N
    c_det = c_miss * frr * p_target + c_fa * far * (1 - p_target)
    j = int(np.argmin(c_det))
    return Result((far[k] + frr[k]) / 2, float(u[k]), float(far[k]), float(frr[k]), float(c_det[j]), float(u[j]),
                  abs(float(far[k]) - float(frr[k])))


def by_sort_objectives_at(pos, neg, th, c_miss=1.0, c_fa=1.0, p_target=0.5):
    u, tp, fa = curves(pos, neg)
    k = int(np.searchsorted(u, np.float32(th)))
    assert k < u.size and u[k] == np.float32(th), "the threshold is not one of the scores"
    frr, far = tp[k] / np.size(pos), fa[k] / np.size(neg)
    return abs(far - frr), c_miss * frr * p_target + c_fa * far * (1 - p_target)


def draw(rng, n_pos, n_neg, levels=None):
    """Target scores around +1, non-target scores around -1.5 (sigma 1.5), optionally quantised to `levels` values."""
    pos = rng.normal(1.0, 1.5, n_pos)
    neg = rng.normal(-1.5, 1.5, n_neg)
    if levels:          # steps of 0.5 clipped to exactly `levels` values
        pos = np.clip(np.round(pos * 2.0), -(levels // 2), levels // 2 - 1) * 0.5
        neg = np.clip(np.round(neg * 2.0), -(levels // 2), levels // 2 - 1) * 0.5
    return pos.astype(np.float32).astype(np.float64), neg.astype(np.float32).astype(np.float64)
