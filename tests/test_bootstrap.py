"""CPU-only checks of the bootstrap (include/xvec_boot.h, xvector_amd.bootstrap): the numpy restatement tests/boot_ref.py
against tests/eer_ref.py on the literally expanded list; the Poisson table against exact rationals; the host-only plan
(csrc/boot_plan.h) through its dump program -- constants, the two maps, the batching rule on either side of a batch, the
workspace regions, every refusal's text, the overflow rule; the host count and weight entry points against the restatement;
the percentile rule against a case worked by hand, compare's refusals; the exports and what the entry points answer to a null
and a short workspace (each returns before the library touches a device)."""
import ctypes as C
import os
import re
from fractions import Fraction
from math import factorial

import numpy as np
import pytest

import boot_ref as br
import eer_ref
from conftest import ROOT
from hipcc_support import header_constants, host_program, needs_host_cxx

P = 0x1000      # a pointer that is never followed


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return host_program("boot_plan_dump", tmp_path_factory.mktemp("boot_plan"))


# ---------------------------------------------------------------- the restatement

def test_poisson_table_is_the_exact_cumulative_distribution():
    """T_i = floor(2^32 P[Poisson(1) <= i]) bracketed between two rational bounds of 1 / e that give the same floor."""
    lo = sum(Fraction((-1) ** k, factorial(k)) for k in range(30))      # even number of terms: below 1 / e
    hi = lo + Fraction(1, factorial(30))                                # one more term: above
    assert lo < hi
    table = br.poisson_table()
    assert len(table) == 13 and table[-1] == 2 ** 32 - 1 and table[-2] < 2 ** 32 - 1
    for i, t in enumerate(table):
        cdf = sum(Fraction(1, factorial(k)) for k in range(i + 1))
        assert int(lo * cdf * 2 ** 32) == int(hi * cdf * 2 ** 32) == t, i
    # the weight is the number of thresholds at or below the word: its distribution is Poisson(1) to within 2^-32 per class
    for w, word in ((0, 0), (0, table[0] - 1), (1, table[0]), (1, table[1] - 1), (2, table[1]), (12, table[11]), (13, 2 ** 32 - 1)):
        assert int((np.uint64(word) >= br.POISSON_T).sum()) == w


def _case(seed, n_rows=9, n_cols=11, n=70, levels=6, g_rows=4, g_cols=5):
    rng = np.random.default_rng(seed)
    scores = np.round(rng.normal(0, 1.5, (n_rows, n_cols)) * levels / 3) * 3 / levels      # few levels: runs of equal scores
    rows, cols = rng.integers(0, n_rows, n), rng.integers(0, n_cols, n)
    rg, cg = rng.integers(0, g_rows, n_rows), rng.integers(0, g_cols, n_cols)
    tgt = (rng.random(n) < 0.4).astype(np.uint8)
    scores[rows, cols] += tgt * 0.5
    return scores, rows, cols, tgt, rg, cg


@pytest.mark.parametrize("mode", ["rows", "cols", "independent", "joint", "poisson"])
def test_restatement_equals_the_evaluation_of_the_expanded_list(mode):
    """Every trial repeated w_b(t) times and handed to eer_ref: `by_sort` (the kernels' formulation) must agree field for field,
    `naive` (the package's float32 walk) in both objectives to its float32 rounding."""
    scores, rows, cols, tgt, rg, cg = _case(3)
    joint = mode == "joint"
    srt = br.Sorted.trials(scores, rows, cols, tgt, rg if mode in ("rows", "independent", "joint") else None,
                           cg if mode in ("cols", "independent", "joint") else None,
                           5 if joint else 4 if mode in ("rows", "independent") else 0,
                           5 if mode in ("cols", "independent", "joint") else 0)
    evaluated = 0
    for b in range(0, 40):
        w = srt.weights(11, b, joint)
        rec = br.replicate(srt, w, p_target=0.25, c_fa=2.0)
        pos, neg = br.expanded(srt, w)
        assert rec["n_target"] == pos.size and rec["n_nontarget"] == neg.size
        if pos.size == 0 or neg.size == 0:
            assert rec["state"] == 1 and np.isnan(rec["eer"])
            continue
        evaluated += 1
        ref = eer_ref.by_sort(pos, neg, c_fa=2.0, p_target=0.25)
        assert (rec["eer"], rec["eer_threshold"], rec["far"], rec["frr"], rec["min_dcf"], rec["min_dcf_threshold"]) == \
            (ref.eer, ref.eer_th, ref.far, ref.frr, ref.min_dcf, ref.min_dcf_th), b
        walk = eer_ref.naive(pos, neg, c_fa=2.0, p_target=0.25)
        # (the walk breaks ties of |FAR - FRR| by its float32 rounding: the objectives agree, not always the arg-min)
        assert abs(abs(rec["far"] - rec["frr"]) - walk.eer_gap) < 1e-6 and abs(rec["min_dcf"] - walk.min_dcf) < 1e-6, b
    assert evaluated >= 30
    if mode != "poisson":
        assert all(br.group_counts(11, b, s, g).sum() == g for b in (1, 2, 77) for s in (0, 1) for g in (1, 2, 5, 63, 64, 65, 1000))


def test_restatement_counts_what_it_leaves_out_and_knows_the_states():
    scores, rows, cols, tgt, rg, cg = _case(5)
    scores[rows[3], cols[3]] = np.nan
    hit = (rows == rows[3]) & (cols == cols[3])
    rows[7], cols[8] = -1, 11
    hit[7] = hit[8] = False
    rg = rg.copy()
    rg[rows[10]] = 4                    # outside [0, 4)
    in_bad_group = (rg[np.clip(rows, 0, 8)] == 4) & (rows >= 0) & (cols < 11)
    srt = br.Sorted.trials(scores, rows, cols, tgt, rg, cg, 4, 5)
    assert srt.n_bad_index == 2 and srt.n_bad_group == int(in_bad_group.sum()) >= 1
    assert srt.n_nan == int((hit & ~in_bad_group).sum())
    assert srt.t.size == 70 - srt.n_bad_index - srt.n_bad_group - srt.n_nan
    assert br.state(0, 5) == 1 and br.state(5, 5) == 1 and br.state(3, 5) == 0
    assert br.state(1, 2 ** 31 - 1) == 0 and br.state(1, 2 ** 31) == 2 and br.state(0, 2 ** 31) == 2


# ---------------------------------------------------------------- the plan header

@needs_host_cxx
def test_plan_constants_and_maps(plan):
    consts = header_constants("xvec_boot.h", "XVEC_BOOT_")
    consts.pop("MAGIC")                  # (hexadecimal: read below)
    assert consts == {"MAX_GROUPS": 16384, "MAX_BOOT": 100000, "POISSON_TERMS": 13}
    text = open(os.path.join(ROOT, "include", "xvec_boot.h")).read()
    assert "#define XVEC_BOOT_MAGIC 0x626f6f74" in text and br.MAGIC == 0x626f6f74 == int.from_bytes(b"boot", "big")
    got = plan(["const", "poisson"])
    assert got[0] == f"const 256 16 4096 16384 100000 {br.MAGIC} 8 256 {1 << 20} 8 72 13"
    assert [int(x) for x in got[1].split()[1:]] == br.poisson_table()
    words = [0, 1, 0x5e2d58d7, 0x5e2d58d8, 0x7fffffff, 0x80000000, 0xfffffffb, 0xfffffffc, 0xfffffffe, 0xffffffff]
    got = plan([f"pweight {w}" for w in words])
    assert [int(x.split()[1]) for x in got] == [int((np.uint64(w) >= br.POISSON_T).sum()) for w in words]
    picks = [(w, g) for w in words for g in (1, 2, 63, 16384)]
    got = plan([f"pick {w} {g}" for w, g in picks])
    assert [int(x.split()[1]) for x in got] == [(w * g) >> 32 for w, g in picks]
    assert all(0 <= (w * g) >> 32 < g for w, g in picks)
    assert plan(["pack 16383 5 1", "pack 0 16383 2", "packi 2147483646 1", "packi 7 0"]) == \
        [f"pack {16383 | 5 << 14 | 1 << 28} 16383 5 1", f"pack {16383 << 14 | 2 << 28} 0 16383 2",
         f"packi {2147483646 | 1 << 31} 2147483646 1", "packi 7 7 0"]


@needs_host_cxx
def test_plan_draws_equal_the_restatement(plan):
    seeds = (0, 1, 0x123456789abcdef0, 2 ** 64 - 1)
    asks = [(s, b, side, g) for s in seeds for b in (1, 2, 100000) for side in (0, 1) for g in (1, 2, 63, 64, 65, 1000)]
    got = plan([f"counts {s} {b} {side} {g}" for s, b, side, g in asks])
    for (s, b, side, g), line in zip(asks, got):
        c = [int(x) for x in line.split()[1:]]
        assert c == br.group_counts(s, b, side, g).tolist() and sum(c) == g, (s, b, side, g)
    ts = [0, 1, 2, 3, 4, 5, 4095, 4096, 123456, 2 ** 31 - 2]
    got = plan([f"tweight {s} {b} {t}" for s in seeds for b in (1, 9) for t in ts])
    want = [int(br.poisson_weights(s, b, np.array([t]))[0]) for s in seeds for b in (1, 9) for t in ts]
    assert [int(x.split()[1]) for x in got] == want
    # the weights are Poisson(1): mean and variance 1 over many trials
    w = br.poisson_weights(7, 3, np.arange(200000))
    assert abs(w.mean() - 1.0) < 0.01 and abs(w.var() - 1.0) < 0.02 and w.max() <= 13


def _batch_rule(n, n_boot):
    tiles = (n + 4095) // 4096
    b = min(256, max(8, (1 << 20) // tiles // 8 * 8))
    b = min(b, (n_boot + 1 + 7) // 8 * 8)
    return b, -(-(n_boot + 1) // b)


@needs_host_cxx
def test_batching_rule_and_workspace_layout(plan):
    """The batch is a function of (n, n_boot): a multiple of the chunk, bounded by the partials; replicate counts on either
    side of a batch boundary give the number of launches the rule says."""
    from xvector_amd import hip
    cases = [(1, 1), (1, 6), (1, 7), (1, 8), (37720, 254), (37720, 255), (37720, 256), (37720, 1000), (4874 * 4874, 100),
             (4874 * 4874, 175), (4874 * 4874, 176), (2 ** 31 - 1, 100000), (4096 * 4096, 255), (4096 * 4097, 255)]
    got = plan([f"batch {n} {nb}" for n, nb in cases])
    for (n, nb), line in zip(cases, got):
        size, count = _batch_rule(n, nb)
        assert line == f"batch {size} {count}", (n, nb)
        assert size % 8 == 0 and size * ((n + 4095) // 4096) <= max(1 << 20, 8 * ((n + 4095) // 4096))
        assert hip.lib.xvec_boot_batch(n, nb) == size and hip.lib.xvec_boot_batches(n, nb) == count
    assert plan(["batch 37720 255"]) == ["batch 256 1"] and plan(["batch 37720 256"]) == ["batch 256 2"]
    assert plan(["batch 0 10", "batch 10 0", "batch 10 100001", f"batch {2 ** 31} 10"]) == ["batch 0 0"] * 4
    for n, nb, g0, g1 in ((1, 1, 0, 0), (4097, 20, 3, 0), (37720, 1000, 40, 40), (37720, 1000, 0, 16384), (4874 * 4874, 100, 1251, 1251)):
        v = [int(x) for x in plan([f"layout {n} {nb} {g0} {g1}"])[0].split()[1:]]
        offs, total, batch, tiles = v[:13], v[13], v[14], v[15]
        assert batch == _batch_rule(n, nb)[0] and tiles == (n + 4095) // 4096
        sizes = [4 * n] * 4 + [tiles * 256 * 4, -(-tiles * 256 // 4096) * 4, 64, batch * (g0 + g1) * 2, batch * tiles * 16, batch * 16,
                 batch * tiles * 24, batch * tiles * 24, batch * tiles * 8]
        assert offs[0] == 0 and all(o % 256 == 0 for o in offs) and total % 256 == 0
        for o, size, nxt in zip(offs, sizes, offs[1:] + [total]):
            assert o + size <= nxt < o + size + 256, (n, nb, offs, sizes)      # disjoint, in order, no slack beyond alignment
        assert hip.lib.xvec_boot_workspace_bytes(n, nb, g0, g1) == total
    # the partials of a batch stay bounded at all pairs: about 75 MB whatever n_boot is
    v = [int(x) for x in plan([f"layout {4874 * 4874} 100000 1251 1251"])[0].split()[1:]]
    assert v[13] - v[8] < 80e6
    for bad in ((0, 1, 0, 0), (1, 0, 0, 0), (1, 100001, 0, 0), (1, 1, 16385, 0), (1, 1, 0, 16385), (1, 1, -1, 0), (2 ** 31, 1, 0, 0)):
        assert plan(["layout %d %d %d %d" % bad]) == ["layout" + " 0" * 16]
        assert hip.lib.xvec_boot_workspace_bytes(*bad) == 0


REFUSALS = [
    ("noparams", "refused null pointer: params"),
    ("params 0 0 0 0 0 0 1 1 0.5", "refused n_boot = 0 must lie in 1 .. 100000"),
    ("params 100001 0 0 0 0 0 1 1 0.5", "refused n_boot = 100001 must lie in 1 .. 100000"),
    ("params 100000 0 0 0 0 0 1 1 0.5", "ok"),
    ("params 10 1 16385 0 0 0 1 1 0.5", "refused 16385 row and 0 column groups: at most 16384 on a side"),
    ("params 10 1 4 1 16385 0 1 1 0.5", "refused 4 row and 16385 column groups: at most 16384 on a side"),
    ("params 10 1 16384 1 16384 1 1 1 0.5", "ok"),
    ("params 10 1 0 0 0 0 1 1 0.5", "refused n_row_groups = 0: at least one group with row_group, 0 without"),
    ("params 10 0 3 0 0 0 1 1 0.5", "refused n_row_groups = 3: at least one group with row_group, 0 without"),
    ("params 10 0 -1 0 0 0 1 1 0.5", "refused n_row_groups = -1: at least one group with row_group, 0 without"),
    ("params 10 0 0 1 0 0 1 1 0.5", "refused n_col_groups = 0: at least one group with col_group, 0 without"),
    ("params 10 0 0 0 2 0 1 1 0.5", "refused n_col_groups = 2: at least one group with col_group, 0 without"),
    ("params 10 1 3 0 0 1 1 1 0.5", "refused joint needs row_group and col_group"),
    ("params 10 0 0 0 0 1 1 1 0.5", "refused joint needs row_group and col_group"),
    ("params 10 1 3 1 4 1 1 1 0.5", "refused joint needs n_row_groups == n_col_groups (got 3 and 4)"),
    ("params 10 1 3 1 4 0 1 1 0.5", "ok"),
    ("params 10 0 0 0 0 0 -1 1 0.5", "refused c_miss = -1 and c_fa = 1 must be finite and >= 0, p_target = 0.5 in [0, 1]"),
    ("params 10 0 0 0 0 0 1 inf 0.5", "refused c_miss = 1 and c_fa = inf must be finite and >= 0, p_target = 0.5 in [0, 1]"),
    ("params 10 0 0 0 0 0 1 1 1.5", "refused c_miss = 1 and c_fa = 1 must be finite and >= 0, p_target = 1.5 in [0, 1]"),
    ("params 10 0 0 0 0 0 1 1 nan", "refused c_miss = 1 and c_fa = 1 must be finite and >= 0, p_target = nan in [0, 1]"),
    ("vector 0 1 0", "refused the plain vector form has no groups: its trials are resampled one by one"),
    ("vector 0 0 1", "refused the plain vector form has no groups: its trials are resampled one by one"),
    ("vector 0 0 0", "ok"),
    ("vector 1 1 1", "ok"),
    ("outputs 0 1", "refused null pointer: summary / records"),
    ("outputs 1 0", "refused null pointer: summary / records"),
    ("outputs 1 1", "ok"),
    ("hcounts 0 0 4 1", "refused b = 0 must lie in 1 .. 100000"),
    ("hcounts 100001 0 4 1", "refused b = 100001 must lie in 1 .. 100000"),
    ("hcounts 1 2 4 1", "refused side = 2 must be 0 (rows) or 1 (columns)"),
    ("hcounts 1 0 0 1", "refused n_groups = 0 must lie in 1 .. 16384"),
    ("hcounts 1 1 16385 1", "refused n_groups = 16385 must lie in 1 .. 16384"),
    ("hcounts 1 1 16384 0", "refused null pointer: counts_out"),
    ("hcounts 1 1 16384 1", "ok"),
    ("hpoisson 0 0 1", "refused b = 0 must lie in 1 .. 100000"),
    ("hpoisson 1 -1 1", "refused t = -1 must lie in 0 .. 2^31 - 2"),
    ("hpoisson 1 2147483647 1", "refused t = 2147483647 must lie in 0 .. 2^31 - 2"),
    ("hpoisson 1 2147483646 0", "refused null pointer: weight_out"),
    ("hpoisson 1 2147483646 1", "ok"),
]


@needs_host_cxx
def test_every_refusal_has_its_text(plan):
    assert plan([q for q, _ in REFUSALS]) == [a for _, a in REFUSALS]


@needs_host_cxx
def test_overflow_and_degenerate_rule(plan):
    """A replicate of 2^31 or more weighted trials would overflow the cross products: the rule the kernels ask, on its edges."""
    asks = [(0, 5), (5, 5), (3, 5), (1, 2 ** 31 - 1), (2 ** 31 - 2, 2 ** 31 - 1), (1, 2 ** 31), (0, 2 ** 31), (2 ** 31, 2 ** 31), (5, 2 ** 40),
            (0, 0)]
    got = plan([f"state {p} {a}" for p, a in asks])
    assert [int(x.split()[1]) for x in got] == [br.state(p, a) for p, a in asks] == [1, 1, 0, 0, 0, 2, 2, 2, 2, 1]
    # below the bound the cross products fit: |fa P - tp N| <= P N < 2^62
    assert (2 ** 31 - 1) ** 2 < 2 ** 62


# ---------------------------------------------------------------- the module and the C ABI without a device

EXPORTS = {"xvec_boot_last_error", "xvec_boot_workspace_bytes", "xvec_boot_batch", "xvec_boot_batches", "xvec_boot_trials",
           "xvec_boot_all_pairs", "xvec_boot_counts_host", "xvec_boot_poisson_host"}


def test_exports_and_module_surface():
    import torch
    import xvector_amd
    from xvector_amd import bootstrap, evaluate, hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xvec_boot.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(xvec_boot_[a-z_0-9]+)\s*\(", src)) == EXPORTS <= set(hip.EXPORTS)
    assert {"xvec_eval_sorted_order", "xvec_eval_sorted_order_all_pairs", "xvec_eval_sorted_order_workspace_bytes"} <= set(hip.EXPORTS)
    assert all(hasattr(hip.lib, n) for n in EXPORTS)
    assert C.sizeof(hip._wsb_boot) == C.sizeof(C.c_size_t) and issubclass(hip._wsb_boot, hip._wsb_fuse) and hip._wsb_boot is not hip._wsb_fuse
    assert C.sizeof(hip.BootParams) == 64 and hip.BootParams.seed.offset == 32 and hip.BootParams.c_miss.offset == 40
    for name in ("BootstrapResult", "BootstrapComparison", "bootstrap_trials", "bootstrap_all_pairs"):
        assert getattr(xvector_amd, name) is getattr(bootstrap, name) and name in xvector_amd.__all__
    assert xvector_amd.bootstrap is bootstrap and "bootstrap" in xvector_amd.__all__
    assert bootstrap.MAX_GROUPS == 16384 and bootstrap.MAX_BOOT == 100000
    assert callable(evaluate.plda_score_stat_object.confidence) and callable(evaluate.sorted_order)
    cpu = torch.zeros(3, 3, dtype=torch.float64)
    for call in (lambda: bootstrap.bootstrap_trials(cpu, xvector_amd.TrialList([0, 1], [1, 2], [1, 0])),
                 lambda: bootstrap.bootstrap_all_pairs(cpu, [0, 0, 1]), lambda: evaluate.sorted_order(cpu[0], [1, 0, 1])):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()


def test_host_entry_points_equal_the_restatement():
    from xvector_amd import bootstrap, hip
    for seed in (0, 5, 2 ** 64 - 1):
        for b in (1, 3, 100000):
            for side in (0, 1):
                for g in (1, 2, 63, 64, 65, 16384):
                    c = bootstrap.group_counts(seed, b, side, g)
                    assert c.dtype == np.uint16 and c.tolist() == br.group_counts(seed, b, side, g).tolist() and int(c.sum()) == g
            ts = [0, 1, 2, 3, 4, 4097, 2 ** 31 - 2]
            assert [bootstrap.poisson_weight(seed, b, t) for t in ts] == br.poisson_weights(seed, b, np.array(ts)).tolist()
    # the two sides and two replicates draw differently; the same arguments draw the same
    a = bootstrap.group_counts(1, 1, 0, 1000)
    assert (a != bootstrap.group_counts(1, 1, 1, 1000)).any() and (a != bootstrap.group_counts(1, 2, 0, 1000)).any()
    assert (a != bootstrap.group_counts(2, 1, 0, 1000)).any() and (a == bootstrap.group_counts(1, 1, 0, 1000)).all()
    err = lambda: hip.lib.xvec_boot_last_error().decode()
    out = np.zeros(4, dtype=np.uint16).ctypes.data_as(C.POINTER(C.c_uint16))
    assert hip.lib.xvec_boot_counts_host(0, 0, 0, 4, out) == hip.ERR_ARG and err() == "b = 0 must lie in 1 .. 100000"
    assert hip.lib.xvec_boot_counts_host(0, 1, 2, 4, out) == hip.ERR_ARG and err() == "side = 2 must be 0 (rows) or 1 (columns)"
    assert hip.lib.xvec_boot_counts_host(0, 1, 0, 16385, out) == hip.ERR_ARG and err() == "n_groups = 16385 must lie in 1 .. 16384"
    assert hip.lib.xvec_boot_counts_host(0, 1, 0, 4, None) == hip.ERR_ARG and err() == "null pointer: counts_out"
    assert hip.lib.xvec_boot_poisson_host(0, 1, -1, C.byref(C.c_int32())) == hip.ERR_ARG and err() == "t = -1 must lie in 0 .. 2^31 - 2"
    assert hip.lib.xvec_boot_poisson_host(0, 1, 0, None) == hip.ERR_ARG and err() == "null pointer: weight_out"


def _params(hip, **kw):
    p = dict(row_group=None, col_group=None, n_row_groups=0, n_col_groups=0, joint=0, n_boot=10, seed=0, c_miss=1.0, c_fa=1.0, p_target=0.5)
    p.update(kw)
    return hip.BootParams(**p)


def test_c_abi_argument_errors_return_before_any_device_call():
    from xvector_amd import hip
    lib, err = hip.lib, lambda: hip.lib.xvec_boot_last_error().decode()
    need = lib.xvec_boot_workspace_bytes(4, 10, 2, 0)
    assert need > 0 and need % 256 == 0

    def trials(params, scores=P, ld=4, rows=3, cols=4, ri=P, ci=P, tgt=P, n=4, summary=P, records=P, ws=P, size=need):
        return lib.xvec_boot_trials(scores, ld, rows, cols, ri, ci, tgt, n, None if params is None else C.byref(params), summary,
                                    records, ws, size, None)

    def pairs(params, scores=P, ld=4, rows=3, cols=4, rc=P, cc=P, summary=P, records=P, ws=P, size=need):
        return lib.xvec_boot_all_pairs(scores, ld, rows, cols, rc, cc, 1, None if params is None else C.byref(params), summary,
                                       records, ws, size, None)
    ok = _params(hip, row_group=P, n_row_groups=2)
    for call in (trials, pairs):
        assert call(None) == hip.ERR_ARG and err() == "null pointer: params"
        assert call(_params(hip, n_boot=0)) == hip.ERR_ARG and err() == "n_boot = 0 must lie in 1 .. 100000"
        assert call(_params(hip, n_boot=100001)) == hip.ERR_ARG and err() == "n_boot = 100001 must lie in 1 .. 100000"
        assert call(_params(hip, row_group=P, n_row_groups=16385)) == hip.ERR_ARG and \
            err() == "16385 row and 0 column groups: at most 16384 on a side"
        assert call(_params(hip, row_group=P, n_row_groups=0)) == hip.ERR_ARG and "at least one group with row_group" in err()
        assert call(_params(hip, col_group=P, n_col_groups=0)) == hip.ERR_ARG and "at least one group with col_group" in err()
        assert call(_params(hip, row_group=P, n_row_groups=2, joint=1)) == hip.ERR_ARG and err() == "joint needs row_group and col_group"
        assert call(_params(hip, row_group=P, n_row_groups=2, col_group=P, n_col_groups=3, joint=1)) == hip.ERR_ARG and \
            err() == "joint needs n_row_groups == n_col_groups (got 2 and 3)"
        assert call(_params(hip, p_target=2.0)) == hip.ERR_ARG and "p_target = 2 in [0, 1]" in err()
        assert call(ok, summary=None) == hip.ERR_ARG and err() == "null pointer: summary / records"
        assert call(ok, records=None) == hip.ERR_ARG and err() == "null pointer: summary / records"
        assert call(ok, scores=None) == hip.ERR_ARG and err() == "null pointer: scores"
        assert call(ok, ld=3) == hip.ERR_ARG and err() == "ld = 3 is smaller than n_cols = 4"
        # the workspace: null, and one byte short
        assert call(ok, ws=None) == hip.ERR_ARG and err() == "null pointer: workspace"
    assert trials(ok, size=need - 1) == hip.ERR_WORKSPACE and err() == f"workspace too small: {need - 1} < {need} bytes"
    need12 = lib.xvec_boot_workspace_bytes(12, 10, 2, 0)
    assert pairs(ok, size=need12 - 1) == hip.ERR_WORKSPACE and err() == f"workspace too small: {need12 - 1} < {need12} bytes"
    assert trials(ok, n=0) == hip.ERR_ARG and err() == "n_trials = 0: need at least one trial"
    assert trials(ok, n=2 ** 31) == hip.ERR_TOO_LARGE and err() == "n_trials = 2147483648 exceeds 2^31 - 1"
    assert trials(ok, tgt=None) == hip.ERR_ARG and err() == "null pointer: is_target"
    assert trials(ok, ri=None) == hip.ERR_ARG and "both be given or both be null" in err()
    assert trials(ok, ri=None, ci=None, rows=1) == hip.ERR_ARG and \
        err() == "the plain vector form has no groups: its trials are resampled one by one"
    assert pairs(ok, rc=None) == hip.ERR_ARG and err() == "null pointer: row_class / col_class"
    assert pairs(ok, rows=65536, cols=65536, ld=65536) == hip.ERR_TOO_LARGE and "exceed 2^31 - 1 trials" in err()
    # every (void*, _wsb_boot) pair of the binding is held here or below
    takes = {n for n, (_, a) in hip._SIGS.items() if any(x is hip._wsb_boot and a[i - 1] is C.c_void_p for i, x in enumerate(a))}
    assert takes == {"xvec_boot_trials", "xvec_boot_all_pairs", "xvec_eval_sorted_order", "xvec_eval_sorted_order_all_pairs"}


def test_sorted_order_argument_errors_return_before_any_device_call():
    from xvector_amd import hip
    lib, err = hip.lib, lambda: hip.lib.xvec_eval_last_error().decode()
    need = lib.xvec_eval_sorted_order_workspace_bytes(5)
    assert need > 0 and need % 256 == 0 and lib.xvec_eval_sorted_order_workspace_bytes(0) == 0
    assert lib.xvec_eval_sorted_order_workspace_bytes(2 ** 31) == 0
    order = lambda scores=P, n=5, tgt=P, keys=P, out=P, ws=P, size=need: lib.xvec_eval_sorted_order(
        scores, 5, 1, 5, None, None, tgt, n, keys, out, ws, size, None)
    assert order(scores=None) == hip.ERR_ARG and err() == "null pointer: scores"
    assert order(n=0) == hip.ERR_ARG and err() == "n_trials = 0: need at least one trial"
    assert order(n=6) == hip.ERR_ARG and "without index arrays the scores are a vector" in err()
    assert order(tgt=None) == hip.ERR_ARG and err() == "null pointer"
    assert order(ws=None) == hip.ERR_ARG and err() == "null pointer"
    assert order(size=need - 1) == hip.ERR_WORKSPACE and err() == f"workspace too small: {need - 1} < {need} bytes"
    assert order(keys=None) == hip.ERR_ARG and err() == "null pointer: keys_out / order_out"
    assert order(out=None) == hip.ERR_ARG and err() == "null pointer: keys_out / order_out"
    need20 = lib.xvec_eval_sorted_order_workspace_bytes(20)
    pairs = lambda rc=P, keys=P, ws=P, size=need20, rows=4, cols=5, ld=5: lib.xvec_eval_sorted_order_all_pairs(
        P, ld, rows, cols, rc, P, 1, keys, P, ws, size, None)
    assert pairs(rc=None) == hip.ERR_ARG and err() == "null pointer"
    assert pairs(ws=None) == hip.ERR_ARG and err() == "null pointer"
    assert pairs(size=need20 - 1) == hip.ERR_WORKSPACE and err() == f"workspace too small: {need20 - 1} < {need20} bytes"
    assert pairs(keys=None) == hip.ERR_ARG and err() == "null pointer: keys_out / order_out"
    assert pairs(rows=65536, cols=65536, ld=65536) == hip.ERR_TOO_LARGE and "exceed 2^31 - 1 trials" in err()


# ---------------------------------------------------------------- percentiles and the paired comparison

def _result(values, seed=1, n_boot=None, mode="joint", groups=(5, 5), point=0.1):
    import torch
    from xvector_amd import TrialResult
    from xvector_amd.bootstrap import BootstrapResult
    v = torch.tensor(values, dtype=torch.float64)
    z = torch.zeros_like(v)
    n = torch.ones(v.numel(), dtype=torch.int64)
    return BootstrapResult(TrialResult(point, 0.0, point, point, point, 0.0, 1, 1), v, v * 2, z, z, z, z, n, n, 0, 0, 0,
                           int(torch.isnan(v).sum()), 0, v.numel() if n_boot is None else n_boot, seed, mode, groups[0], groups[1])


def test_percentile_rule_on_a_hand_computed_case():
    """k_lo = max(1, floor((m + 1)(1 - level) / 2)), k_hi = m + 1 - k_lo, over the replicates that are not NaN."""
    from xvector_amd.bootstrap import percentile_ranks
    assert percentile_ranks(1000, 0.95) == (25, 976) and percentile_ranks(999, 0.95) == (25, 975)
    assert percentile_ranks(39, 0.95) == (1, 39) and percentile_ranks(79, 0.95) == (2, 78) and percentile_ranks(1, 0.95) == (1, 1)
    assert percentile_ranks(100, 0.9) == (5, 96) and percentile_ranks(19, 0.9) == (1, 19) and percentile_ranks(199, 0.99) == (1, 199)
    for m in (1, 2, 39, 40, 79, 80, 199, 200, 999, 1000, 1001, 100000):
        for level in (0.5, 0.8, 0.9, 0.95, 0.99):
            assert percentile_ranks(m, level) == br.percentile_ranks(m, level), (m, level)
    with pytest.raises(ValueError, match="no replicate"):
        percentile_ranks(0, 0.95)
    with pytest.raises(ValueError, match="inside"):
        percentile_ranks(10, 1.0)
    # 79 values 0.79, 0.78, ..., 0.01 and one NaN, shuffled: m = 79, ranks 2 and 78 -> 0.02 and 0.78; at 50 %: ranks 20 and 60
    vals = [k / 100 for k in range(79, 0, -1)] + [float("nan")]
    vals = [vals[(7 * i) % 80] for i in range(80)]
    r = _result(vals)
    assert r.interval("eer", 0.95) == (0.02, 0.78) and r.interval("eer", 0.5) == (0.2, 0.6)
    assert r.interval("min_dcf", 0.95) == (0.04, 1.56)
    m, mean = 79, 0.4
    want = (sum((k / 100 - mean) ** 2 for k in range(1, 80)) / (m - 1)) ** 0.5
    assert abs(r.stderr("eer") - want) < 1e-15 and abs(r.stderr("min_dcf") - 2 * want) < 1e-15
    with pytest.raises(ValueError, match="metric 'cllr'"):
        r.interval("cllr")
    with pytest.raises(ValueError, match="stderr needs two"):
        _result([0.5, float("nan")]).stderr()


def test_compare_pairs_replicates_and_refuses_unpaired_results():
    from xvector_amd.bootstrap import compare
    a = _result([0.10, 0.20, 0.30, float("nan"), 0.50], point=0.25)
    b = _result([0.15, 0.15, 0.35, 0.40, float("nan")], point=0.30)
    c = compare(a, b, "eer", level=0.5)
    # differences -0.05, 0.05, -0.05, NaN, NaN: three valid; m = 3 at 50 %: ranks 1 and 3
    assert c.n_valid == 3 and abs(c.difference + 0.05) < 1e-15 and abs(c.lo + 0.05) < 1e-15 and abs(c.hi - 0.05) < 1e-15
    assert abs(c.share_a_lower - 2 / 3) < 1e-15 and c.metric == "eer"
    assert compare(a, b, "min_dcf", level=0.5).lo == 2 * c.lo
    for other, text in ((_result([0.1] * 5, seed=2), "differ in seed"), (_result([0.1] * 4), "differ in n_boot"),
                        (_result([0.1] * 5, mode="independent"), "differ in mode"),
                        (_result([0.1] * 5, groups=(5, 6)), "differ in group counts")):
        with pytest.raises(ValueError, match=text):
            compare(a, other)
