"""CPU-only checks of score analysis (include/xvec_analyze.h, xvector_amd.analyze): the numpy oracle tests/analyze_ref.py
against numpy's own reductions, np.histogram, scipy's gaussian_kde and a literal transcription of the reference's
max-and-zero loop; the host-only plan (csrc/analyze_plan.h) through its dump program -- constants, every refusal's text, the
workspace regions on either side of each size threshold, the copies rule around its thresholds, the digit and candidate plan,
the bin map against numpy on ties, edges, infinities and values no integer holds; the exports against the header and what the
entry points answer to bad arguments and to a null or short workspace (each returns before the library touches a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import analyze_ref as ar
from conftest import ROOT
from hipcc_support import header_constants, host_program, needs_host_cxx

P = 0x1000      # a pointer that is never followed


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return host_program("analyze_plan_dump", tmp_path_factory.mktemp("analyze_plan"))


# ---------------------------------------------------------------- the oracle

def _case(seed, n_rows=13, n_cols=17, n=150):
    rng = np.random.default_rng(seed)
    scores = rng.normal(0.0, 9.0, (n_rows, n_cols))
    rows, cols = rng.integers(-1, n_rows + 1, n), rng.integers(0, n_cols, n)
    tgt = (rng.random(n) < 0.35).astype(np.uint8)
    scores[2, 3] = np.nan
    rows[5], cols[5] = 2, 3
    return scores, rows, cols, tgt


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_moments_equal_numpys(seed):
    scores, rows, cols, tgt = _case(seed)
    u = ar.usable_trials(scores, rows, cols, tgt)
    bad = (rows < 0) | (rows >= scores.shape[0])
    assert u.n_bad == int(bad.sum()) and u.n_nan == int(np.isnan(scores[rows[~bad], cols[~bad]]).sum()) >= 1
    for c, m in enumerate(ar.summary(u)):
        s, t = u.of(c)[:2]
        assert m["n"] == len(s) and m["min"] == np.min(s) and m["max"] == np.max(s)
        assert s[list(u.of(c)[1]).index(m["t_min"])] == m["min"] and (s[t < m["t_min"]] != m["min"]).all()
        assert s[list(u.of(c)[1]).index(m["t_max"])] == m["max"] and (s[t < m["t_max"]] != m["max"]).all()
        np.testing.assert_allclose(float(m["mean"]), np.mean(s), rtol=1e-13)
        np.testing.assert_allclose(float(m["var"]), np.var(s), rtol=1e-12)
    empty = ar.moments(np.zeros(0), np.zeros(0, np.int64))
    assert empty["n"] == 0 and empty["t_min"] == -1 and np.isnan(empty["mean"])
    # all pairs: the diagonal and the lower triangle leave when asked to
    cls = np.arange(13) % 4
    sq = scores[:, :13]
    full, off, up = (ar.usable_all_pairs(sq, cls, cls, d, o) for d, o in ((False, False), (True, False), (True, True)))
    assert len(full.s) + full.n_nan == 169 and len(off.s) + off.n_nan == 156 and len(up.s) + up.n_nan == 78 and (up.row < up.col).all()


def test_oracle_bins_equal_np_histogram_away_from_ties():
    rng = np.random.default_rng(3)
    s = rng.normal(0.0, 20.0, 4000)
    s = s[np.abs(s - np.floor(s) - 0.5) > 1e-6]                      # no value within rounding of a tie of rint
    u = ar.Usable(s, np.zeros(len(s), bool), np.arange(len(s)), np.zeros(len(s), np.int64), np.arange(len(s)), 0, 0)
    for width, first, n_bins in ((1.0, -30, 61), (0.25, -100, 200), (3.0, -5, 12)):
        got = ar.histogram(u, width, first, n_bins, ar.RINT)[0]
        edges = (np.arange(first, first + n_bins + 1) - 0.5) * width
        want = np.histogram(s, bins=edges)[0]
        assert (got[1:-1] == want).all() and got[0] == (s < edges[0]).sum() and got[-1] == (s >= edges[-1]).sum() and got.sum() == len(s)
        got = ar.histogram(u, width, first, n_bins, ar.FLOOR)[0]
        edges = np.arange(first, first + n_bins + 1) * width
        assert (got[1:-1] == np.histogram(s, bins=edges)[0]).all() and got.sum() == len(s)


def test_oracle_density_equals_scipys_gaussian_kde_on_the_repeated_values():
    from scipy.stats import gaussian_kde
    rng = np.random.default_rng(4)
    values = np.arange(-20, 31, dtype=np.float64)
    counts = rng.integers(0, 40, len(values))
    grid, dens = ar.density(values, counts, gridsize=64)
    data = np.repeat(values, counts)
    np.testing.assert_allclose(dens, gaussian_kde(data)(grid), rtol=1e-9)
    h = len(data) ** (-0.2) * data.std(ddof=1)
    assert grid[0] == data.min() - 3 * h and len(grid) == 64
    grid, dens = ar.density(values, counts, bw=1.5, cut=2)
    np.testing.assert_allclose(dens, gaussian_kde(data, bw_method=1.5 / data.std(ddof=1))(grid), rtol=1e-9)
    # and the module's own density is the oracle's
    from xvector_amd import analyze
    hist = analyze.ScoreHistogram(counts, counts[::-1].copy(), values, (0, 0), (0, 0), analyze.Bins(-20, len(values)))
    for which, c in (("nontarget", counts), ("target", counts[::-1]), ("all", counts + counts[::-1])):
        g, d = hist.density(which, gridsize=50)
        rg, rd = ar.density(values, c, gridsize=50)
        assert np.array_equal(g, rg) and np.array_equal(d, rd)


def test_oracle_hardest_equals_the_references_loop_where_the_definitions_coincide():
    """A small positive matrix without repeated scores: the reference's loop finds one cell per hit, in the oracle's order."""
    rng = np.random.default_rng(5)
    n = 12
    scores = rng.permutation(n * n).reshape(n, n).astype(np.float64) + 1.0
    names = [f"id{10000 + i // 3}/a/{i}.wav" for i in range(n)]
    spk = np.array([x.split("/")[0] for x in names])
    pos = spk[:, None] == spk[None, :]
    u = ar.usable_all_pairs(scores, spk, spk, skip_diagonal=False)
    fp, fn = ar.hardest(u, 20)
    hits = ar.reference_false_positives(scores * ~pos, 20)
    assert [(h[0], int(h[1][0]), int(h[2][0])) for h in hits] == [(r["score"], r["row"], r["col"]) for r in fp]
    assert all(len(h[1]) == 1 for h in hits)
    # the misses: the lowest positive scores (the reference's second loop searches the minimum of pos_scores)
    order = np.sort(scores[pos])[:20]
    assert fn["score"].tolist() == order.tolist() and (fn["t"] == fn["row"] * n + fn["col"]).all()
    # ties go to the lower t, the two zeros are equal, the order is that of the double and not of its float32 rounding
    s = np.array([1.0, 1.0 + 2.0 ** -40, -0.0, 0.0, 1.0, -np.inf, np.inf])
    u = ar.Usable(s, np.zeros(7, bool), np.arange(7), np.zeros(7, np.int64), np.arange(7), 0, 0)
    assert ar.hardest(u, 7)[0]["t"].tolist() == [6, 1, 0, 4, 2, 3, 5]
    pairs, num, perf = ar.confusable_pairs(fp, names, names)
    assert len(num) == len(perf) == 20 and max(num) == len(pairs) and num[0] == 1 and all(a <= b for a, b in pairs)


# ---------------------------------------------------------------- the plan

@needs_host_cxx
def test_plan_constants_and_grid(plan):
    k = header_constants("xvec_analyze.h", "XVEC_ANALYZE_")
    const = [int(x) for x in plan(["const"])[0].split()[1:]]
    assert const == [256, 8, k["TILE"], k["MAX_BLOCKS"], k["MAX_BINS"], k["MAX_K"], k["MAX_CAND"], 16384, 8256, 32, 256, 8, 112, 16,
                     256, 24, k["MAX_BLOCKS"] * k["TILE"] + 1]
    assert (k["TILE"], k["MAX_BLOCKS"], k["MAX_BINS"], k["MAX_K"], k["FLOOR"], k["RINT"]) == (2048, 1024, 4094, 2048, 0, 1)
    tile, G = k["TILE"], k["MAX_BLOCKS"]
    grid = lambda n: [int(x) for x in plan([f"grid {n}"])[0].split()[1:]]
    assert grid(1) == [1, 1, 1, 8 + 9 + 1 + 9] and grid(tile) == [1, 1, 1, 27] and grid(tile + 1) == [2, 2, 1, 27]
    assert grid(G * tile) == [G, G, 1, 8 + 9 + 4 + 9] and grid(G * tile + 1) == [G + 1, G, 2, 16 + 9 + 4 + 9]
    assert grid(4874 * 4874) == [11600, G, 12, 96 + 9 + 4 + 9]
    # the blocks' ranges cut the tiles without a gap, in rising order, one or two tiles each just past the grid
    ends = [plan([f"range {b} {G + 1} {G}"])[0].split()[1:] for b in (0, 1, G - 2, G - 1)]
    assert ends == [["0", "1"], ["1", "2"], [str(G - 2), str(G - 1)], [str(G - 1), str(G + 1)]]
    cover = [tuple(int(x) for x in a.split()[1:]) for a in plan([f"range {b} 11600 {G}" for b in range(G)])]
    assert cover[0][0] == 0 and cover[-1][1] == 11600 and all(a[1] == b[0] for a, b in zip(cover, cover[1:]))
    assert max(e - s for s, e in cover) == 12


@needs_host_cxx
def test_plan_bin_map_equals_numpys(plan):
    below_half = np.nextafter(0.5, 0.0)
    cases = []
    ties = [-2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 3.5, below_half, -below_half, np.nextafter(0.5, 1.0), -0.0, 0.0]
    edges = [-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, np.nextafter(1.0, 0.0), np.nextafter(-1.0, -2.0), -0.0]
    wild = [np.inf, -np.inf, 1e300, -1e300, 1e19, -1e19, 2.0 ** 63, -2.0 ** 63, 4.9e-324]
    for width in (1.0, 0.25, 3.0):
        for first, n_bins in ((-2, 5), (0, 1), (-7, 2), (1, 64), (-(2 ** 52), 3), (2 ** 52 - 3, 3)):
            for rounding in (ar.FLOOR, ar.RINT):
                for s in ties + edges + wild + [x * width for x in ties + edges]:
                    cases.append((float(s), width, first, n_bins, rounding))
    got = [int(a.split()[1]) for a in plan([f"slot {s.hex()} {w.hex()} {f} {n} {r}" for s, w, f, n, r in cases])]
    want = [int(ar.slots(np.array([s]), w, f, n, r)[0]) for s, w, f, n, r in cases]
    assert got == want
    one = lambda s, rounding, first=-2, n_bins=5, width=1.0: int(plan([f"slot {float(s).hex()} {float(width).hex()} {first} {n_bins} {rounding}"])[0].split()[1])
    # rint goes to even on exact ties; the largest double below one half goes down
    assert [one(s, ar.RINT) for s in (-2.5, -1.5, -0.5, 0.5, 1.5, 2.5)] == [1, 1, 3, 3, 5, 5]
    assert one(below_half, ar.RINT) == 3 and one(0.5, ar.RINT) == 3 and one(np.nextafter(0.5, 1.0), ar.RINT) == 4
    # floor: a value on an edge opens its bin
    assert [one(s, ar.FLOOR) for s in (-2.0, np.nextafter(-2.0, -3.0), 2.0, np.nextafter(3.0, 2.0), 3.0)] == [1, 0, 5, 5, 6]
    # what no integer holds goes to the ends without being converted
    assert [one(s, ar.RINT) for s in (np.inf, 1e300, 2.0 ** 63)] == [6, 6, 6] and [one(s, ar.FLOOR) for s in (-np.inf, -1e300)] == [0, 0]
    assert one(-0.0, ar.RINT) == 3 and one(-0.0, ar.FLOOR) == 3 and one(-0.0, ar.FLOOR, first=0, n_bins=1) == 1


@needs_host_cxx
def test_plan_copies_rule_and_select_plan(plan):
    copies = lambda n_bins, asked=0: [int(x) for x in plan([f"copies {n_bins} {asked}"])[0].split()[1:]]
    assert copies(1) == [32, 32, 6, 7] and copies(2) == [32, 32, 8, 9] and copies(64) == [32, 32, 132, 133]
    # 256 bins: 516 slots, 8256 // 517 = 15 copies fit -> 8
    assert copies(256) == [8, 8, 516, 517] and copies(256, 2) == [8, 2, 516, 517]
    # the thresholds: c copies while c strides fit the 8256 words
    for c in (32, 16, 8, 4, 2):
        last = (8256 // c - 1) // 2 - 2                   # the most bins with 2 (n_bins + 2) + 1 <= 8256 / c
        assert copies(last)[0] == c and copies(last + 1)[0] == c // 2, c
    assert copies(2061)[0] == 2 and copies(2062)[0] == 1 and copies(4094) == [1, 1, 8192, 8193]
    assert copies(0)[0] == 0 and copies(4095)[0] == 0
    assert [a.split()[1] for a in plan(["cap 200 0", "cap 2048 0", "cap 64 64", "cap 1 4096"])] == ["16384", "16384", "64", "4096"]
    assert [a.split()[1] for a in plan(["shift 1", "shift 2", "shift 7", "shift 8"])] == ["56", "48", "8", "0"]


@needs_host_cxx
def test_plan_workspace_regions(plan):
    k = header_constants("xvec_analyze.h", "XVEC_ANALYZE_")
    tile, G = k["TILE"], k["MAX_BLOCKS"]
    up = lambda v: (v + 255) // 256 * 256
    summary = lambda n, b=0: [int(x) for x in plan([f"summary {n} {b}"])[0].split()[1:]]
    for n in (1, tile, tile + 1, 2 * tile + 1, G * tile, G * tile + 1, 2 ** 31 - 1):
        blocks = min(G, -(-n // tile))
        assert summary(n) == [0, up(112 * blocks), up(112 * blocks) + up(16 * blocks), -(-n // tile), blocks] == summary(n, 4094)
    assert summary(0)[2] == 0 and summary(2 ** 31)[2] == 0 and summary(5, -1)[2] == 0 and summary(5, 4095)[2] == 0
    hardest = lambda n, kk, cap=0: [int(x) for x in plan([f"hardest {n} {kk} {cap}"])[0].split()[1:]]
    for n in (1, G * tile + 1, 2 ** 31 - 1):              # the workspace does not grow with the trials
        for kk, cap, used in ((1, 0, 16384), (2048, 0, 16384), (64, 64, 64), (200, 65536, 65536)):
            blocks = min(G, -(-n // tile))
            cand = up(24 * used)
            assert hardest(n, kk, cap) == [0, 16384, 16640, 16640 + 16 * G, 16640 + 32 * G, 16640 + 32 * G + cand,
                                           16640 + 32 * G + 2 * cand, -(-n // tile), blocks, used]
    for bad in ((0, 1, 0), (5, 0, 0), (5, 2049, 0), (5, 64, 63), (5, 64, 65537), (2 ** 31, 1, 0)):
        assert hardest(*bad)[6] == 0, bad


@needs_host_cxx
def test_plan_refusals(plan):
    ask = lambda line: plan([line])[0]
    ok_bins = "bins 1 64 1.0 -32 1 0 0 1"
    assert ask(ok_bins) == "ok" and ask("bins 0 0 0 0 9 9 9 0") == "ok"                    # no bins: nothing is looked at
    assert ask("bins 1 0 1.0 0 1 0 0 1") == "refused n_bins = 0 must lie in 1 .. 4094"
    assert ask("bins 1 4095 1.0 0 1 0 0 1") == "refused n_bins = 4095 must lie in 1 .. 4094"
    assert ask("bins 1 64 0 0 1 0 0 1") == "refused width = 0 must be positive and finite"
    assert ask("bins 1 64 -1 0 1 0 0 1") == "refused width = -1 must be positive and finite"
    assert ask("bins 1 64 inf 0 1 0 0 1") == "refused width = inf must be positive and finite"
    assert ask("bins 1 64 nan 0 1 0 0 1") == "refused width = nan must be positive and finite"
    assert ask(f"bins 1 64 1 {2 ** 52 + 1} 1 0 0 1") == f"refused first = {2 ** 52 + 1} must lie in -2^52 .. 2^52"
    assert ask(f"bins 1 64 1 {-2 ** 52 - 1} 1 0 0 1") == f"refused first = {-2 ** 52 - 1} must lie in -2^52 .. 2^52"
    assert ask(f"bins 1 64 1 {2 ** 52} 1 0 0 1") == "ok"
    assert ask("bins 1 64 1 0 2 0 0 1") == "refused rounding = 2 must be 0 (floor) or 1 (rint)"
    assert ask("bins 1 64 1 0 1 3 0 1") == "refused hist_copies = 3 must be 0 or a power of two up to 32 for 64 bins"
    assert ask("bins 1 4094 1 0 1 2 0 1") == "refused hist_copies = 2 must be 0 or a power of two up to 1 for 4094 bins"
    assert ask("bins 1 64 1 0 1 -1 0 1") == "refused hist_copies = -1 must be 0 or a power of two up to 32 for 64 bins"
    assert ask("bins 1 64 1 0 1 32 0 1") == "ok"
    assert ask("bins 1 64 1 0 1 0 5 1") == "refused reserved = 5 must be 0"
    assert ask("bins 1 64 1 0 1 0 0 0") == "refused null pointer: counts"
    assert ask("stats 0") == "refused null pointer: out" and ask("stats 1") == "ok"
    assert ask("select 0 1 0") == "refused null pointer: select"
    assert ask("select 1 0 0") == "refused k = 0 must lie in 1 .. 2048" and ask("select 1 2049 0") == "refused k = 2049 must lie in 1 .. 2048"
    assert ask("select 1 64 63") == "refused cand_cap = 63 must be 0 or lie in k = 64 .. 65536"
    assert ask("select 1 64 65537") == "refused cand_cap = 65537 must be 0 or lie in k = 64 .. 65536"
    assert ask("select 1 64 64") == "ok" and ask("select 1 2048 0") == "ok"
    assert ask("lists 0 1 1") == ask("lists 1 0 1") == "refused null pointer: nontarget_out / target_out"
    assert ask("lists 1 1 0") == "refused null pointer: counts" and ask("lists 1 1 1") == "ok"
    assert ask("query 0 0 1") == "refused n_trials = 0 must lie in 1 .. 2^31 - 1"
    assert ask("query 5 4095 1") == "refused n_bins = 4095 must lie in 0 .. 4094"
    assert ask("query 5 0 0") == "refused null pointer: out" and ask("query 5 0 1") == "ok"


# ---------------------------------------------------------------- the module and the C ABI without a device

EXPORTS = {"xvec_analyze_last_error", "xvec_analyze_plan_host", "xvec_analyze_summary_workspace_bytes",
           "xvec_analyze_hardest_workspace_bytes", "xvec_analyze_summary", "xvec_analyze_summary_all_pairs", "xvec_analyze_hardest",
           "xvec_analyze_hardest_all_pairs"}


def test_exports_and_module_surface():
    import torch
    import xvector_amd
    from xvector_amd import analyze, evaluate, hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xvec_analyze.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(xvec_analyze_[a-z_0-9]+)\s*\(", src)) == EXPORTS <= set(hip.EXPORTS)
    assert all(hasattr(hip.lib, n) for n in EXPORTS)
    assert C.sizeof(hip._wsb_analyze) == C.sizeof(C.c_size_t) and issubclass(hip._wsb_analyze, hip._wsb_boot) and \
        hip._wsb_analyze is not hip._wsb_boot
    assert C.sizeof(hip.AnalyzeBins) == 32 and hip.AnalyzeBins.n_bins.offset == 16 and C.sizeof(hip.AnalyzeSelect) == 8
    assert analyze.RECORD.itemsize == 24 and analyze.RECORD == ar.RECORD and analyze._STATS_WORDS * 8 == 208
    k = header_constants("xvec_analyze.h", "XVEC_ANALYZE_")
    assert (analyze.MAX_BINS, analyze.MAX_K, analyze.FLOOR, analyze.RINT) == (k["MAX_BINS"], k["MAX_K"], k["FLOOR"], k["RINT"])
    for name in ("ScoreSummary", "ScoreHistogram", "HardestTrials", "score_summary", "score_summary_all_pairs", "hardest_trials",
                 "hardest_all_pairs", "confusable_pairs", "compare_speaker_results"):
        assert getattr(xvector_amd, name) is getattr(analyze, name) and name in xvector_amd.__all__
    assert xvector_amd.analyze is analyze and "analyze" in xvector_amd.__all__
    assert callable(evaluate.plda_score_stat_object.analyze)
    cpu = torch.zeros(3, 3, dtype=torch.float64)
    trials = xvector_amd.TrialList([0, 1], [1, 2], [1, 0])
    for call in (lambda: analyze.score_summary(cpu, trials), lambda: analyze.score_summary_all_pairs(cpu, [0, 0, 1]),
                 lambda: analyze.hardest_trials(cpu, trials), lambda: analyze.hardest_all_pairs(cpu, [0, 0, 1]),
                 lambda: analyze.compare_speaker_results(cpu, ["id1/a", "id1/b", "id2/a"], ["id1/a", "id1/b", "id2/a"])):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()
    # the host half: the reference's pair lists
    rec = np.array([(9.0, 0, 2, 2), (8.0, 1, 2, 5), (7.5, 2, 0, 6), (7.0, 0, 1, 1)], dtype=analyze.RECORD)
    names = ["id10001/x/1.wav", "id10003/x/1.wav", "id10002/y/2.wav"]
    assert analyze.confusable_pairs(rec, names, names) == ([(10001, 10002), (10002, 10003), (10001, 10003)], [1, 2, 1, 3], [9.0, 8.0, 7.5, 7.0])
    assert analyze.confusable_pairs(rec, names, names) == ar.confusable_pairs(rec, names, names)
    assert analyze.confusable_pairs(rec[:2], [5, 7, 6], [5, 7, 6])[0] == [(5, 6), (6, 7)]


@needs_host_cxx
def test_plan_host_equals_the_dump(plan):
    from xvector_amd import analyze, hip
    for n in (1, 2048, 2049, 1024 * 2048, 1024 * 2048 + 1, 4874 * 4874):
        p = analyze.plan(n, 256)
        t, b, m, d = (int(x) for x in plan([f"grid {n}"])[0].split()[1:])
        assert (p["tiles"], p["blocks"], p["most_tiles"], p["sum_depth"]) == (t, b, m, d)
        assert p["hist_copies"] == 8 and p["cand_cap"] == 16384 and p["second_tile_from"] == 1024 * 2048 + 1
    assert analyze.plan(5)["hist_copies"] == 0
    err = lambda: hip.lib.xvec_analyze_last_error().decode()
    assert hip.lib.xvec_analyze_plan_host(0, 0, (C.c_int64 * 8)()) == hip.ERR_ARG and err() == "n_trials = 0 must lie in 1 .. 2^31 - 1"
    assert hip.lib.xvec_analyze_plan_host(5, 0, None) == hip.ERR_ARG and err() == "null pointer: out"


def test_c_abi_argument_errors_return_before_any_device_call():
    from xvector_amd import hip
    lib, err = hip.lib, lambda: hip.lib.xvec_analyze_last_error().decode()
    need_s, need_h = lib.xvec_analyze_summary_workspace_bytes(4, 64), lib.xvec_analyze_hardest_workspace_bytes(4, 3, 0)
    need_s12, need_h12 = lib.xvec_analyze_summary_workspace_bytes(12, 64), lib.xvec_analyze_hardest_workspace_bytes(12, 3, 0)
    assert need_s == 512 and need_h > 2 * 24 * 16384 and need_s % 256 == 0 and need_h % 256 == 0
    assert lib.xvec_analyze_summary_workspace_bytes(0, 0) == 0 == lib.xvec_analyze_summary_workspace_bytes(4, 4095)
    assert lib.xvec_analyze_summary_workspace_bytes(2 ** 31, 0) == 0 == lib.xvec_analyze_hardest_workspace_bytes(2 ** 31, 1, 0)
    assert lib.xvec_analyze_hardest_workspace_bytes(4, 0, 0) == 0 == lib.xvec_analyze_hardest_workspace_bytes(4, 3, 2)
    bins = lambda **kw: hip.AnalyzeBins(**{**dict(width=1.0, first=-32, n_bins=64, rounding=1, hist_copies=0, reserved=0), **kw})
    sel = lambda **kw: hip.AnalyzeSelect(**{**dict(k=3, cand_cap=0), **kw})
    ref = lambda x: None if x is None else C.byref(x)

    def summary(b, scores=P, ld=4, rows=3, cols=4, ri=P, ci=P, tgt=P, n=4, out=P, counts=P, ws=P, size=need_s):
        return lib.xvec_analyze_summary(scores, ld, rows, cols, ri, ci, tgt, n, ref(b), out, counts, ws, size, None)

    def summary_pairs(b, scores=P, ld=4, rows=3, cols=4, rc=P, cc=P, out=P, counts=P, ws=P, size=need_s12):
        return lib.xvec_analyze_summary_all_pairs(scores, ld, rows, cols, rc, cc, 1, 0, ref(b), out, counts, ws, size, None)

    def hardest(s, scores=P, ld=4, rows=3, cols=4, ri=P, ci=P, tgt=P, n=4, out0=P, out1=P, counts=P, ws=P, size=need_h):
        return lib.xvec_analyze_hardest(scores, ld, rows, cols, ri, ci, tgt, n, ref(s), out0, out1, counts, ws, size, None)

    def hardest_pairs(s, scores=P, ld=4, rows=3, cols=4, rc=P, cc=P, out0=P, out1=P, counts=P, ws=P, size=need_h12):
        return lib.xvec_analyze_hardest_all_pairs(scores, ld, rows, cols, rc, cc, 1, 1, ref(s), out0, out1, counts, ws, size, None)
    for call in (summary, summary_pairs):
        assert call(bins(n_bins=0)) == hip.ERR_ARG and err() == "n_bins = 0 must lie in 1 .. 4094"
        assert call(bins(n_bins=4095)) == hip.ERR_ARG and err() == "n_bins = 4095 must lie in 1 .. 4094"
        assert call(bins(width=0.0)) == hip.ERR_ARG and err() == "width = 0 must be positive and finite"
        assert call(bins(width=float("inf"))) == hip.ERR_ARG and err() == "width = inf must be positive and finite"
        assert call(bins(first=2 ** 52 + 1)) == hip.ERR_ARG and err() == f"first = {2 ** 52 + 1} must lie in -2^52 .. 2^52"
        assert call(bins(rounding=2)) == hip.ERR_ARG and err() == "rounding = 2 must be 0 (floor) or 1 (rint)"
        assert call(bins(hist_copies=64)) == hip.ERR_ARG and err() == "hist_copies = 64 must be 0 or a power of two up to 32 for 64 bins"
        assert call(bins(reserved=1)) == hip.ERR_ARG and err() == "reserved = 1 must be 0"
        assert call(bins(), counts=None) == hip.ERR_ARG and err() == "null pointer: counts"
        assert call(None, out=None) == hip.ERR_ARG and err() == "null pointer: out"
        assert call(None, scores=None) == hip.ERR_ARG and err() == "null pointer: scores"
        assert call(None, ld=3) == hip.ERR_ARG and err() == "ld = 3 is smaller than n_cols = 4"
        assert call(None, counts=None, ws=None) == hip.ERR_ARG and err() == "null pointer: workspace"
        assert call(bins(), ws=None) == hip.ERR_ARG and err() == "null pointer: workspace"
    for call in (hardest, hardest_pairs):
        assert call(None) == hip.ERR_ARG and err() == "null pointer: select"
        assert call(sel(k=0)) == hip.ERR_ARG and err() == "k = 0 must lie in 1 .. 2048"
        assert call(sel(k=2049)) == hip.ERR_ARG and err() == "k = 2049 must lie in 1 .. 2048"
        assert call(sel(cand_cap=2)) == hip.ERR_ARG and err() == "cand_cap = 2 must be 0 or lie in k = 3 .. 65536"
        assert call(sel(cand_cap=65537)) == hip.ERR_ARG and err() == "cand_cap = 65537 must be 0 or lie in k = 3 .. 65536"
        assert call(sel(), out0=None) == hip.ERR_ARG and err() == "null pointer: nontarget_out / target_out"
        assert call(sel(), out1=None) == hip.ERR_ARG and err() == "null pointer: nontarget_out / target_out"
        assert call(sel(), counts=None) == hip.ERR_ARG and err() == "null pointer: counts"
        assert call(sel(), scores=None) == hip.ERR_ARG and err() == "null pointer: scores"
        assert call(sel(), ws=None) == hip.ERR_ARG and err() == "null pointer: workspace"
    for call, arg, need in ((summary, bins(), need_s), (summary_pairs, None, need_s12), (hardest, sel(), need_h),
                            (hardest_pairs, sel(), need_h12)):
        assert call(arg, size=need - 1) == hip.ERR_WORKSPACE and err() == f"workspace too small: {need - 1} < {need} bytes"
    for call, arg in ((summary, None), (hardest, sel())):
        assert call(arg, n=0) == hip.ERR_ARG and err() == "n_trials = 0: need at least one trial"
        assert call(arg, n=2 ** 31) == hip.ERR_TOO_LARGE and err() == "n_trials = 2147483648 exceeds 2^31 - 1"
        assert call(arg, tgt=None) == hip.ERR_ARG and err() == "null pointer: is_target"
        assert call(arg, ri=None) == hip.ERR_ARG and "both be given or both be null" in err()
        assert call(arg, ri=None, ci=None, rows=3) == hip.ERR_ARG and "without index arrays the scores are a vector" in err()
    for call, arg in ((summary_pairs, None), (hardest_pairs, sel())):
        assert call(arg, rc=None) == hip.ERR_ARG and err() == "null pointer: row_class / col_class"
        assert call(arg, rows=65536, cols=65536, ld=65536) == hip.ERR_TOO_LARGE and "exceed 2^31 - 1 trials" in err()
    # every (void*, _wsb_analyze) pair of the binding is held here
    takes = {n for n, (_, a) in hip._SIGS.items() if any(x is hip._wsb_analyze and a[i - 1] is C.c_void_p for i, x in enumerate(a))}
    assert takes == {"xvec_analyze_summary", "xvec_analyze_summary_all_pairs", "xvec_analyze_hardest", "xvec_analyze_hardest_all_pairs"}
