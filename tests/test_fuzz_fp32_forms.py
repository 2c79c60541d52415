"""The host restatement of the fp32 kernel forms' geometry (tests/fp32_forms_ref.py) against closed forms, and the reach of the
seeded case list that tests/test_fuzz_fp32_forms_gpu.py walks: at 256 CUs and hidden width 512 every class K1..K10 is met by
at least two of the default cases, every case meets a class, and each Winograd handle (W, S4, S8) meets a tile that starts in
a hole (K3), a tile with three utterance starts (K4a) and a u_tile advance of two or more between a block's tiles (K5b).

Pinned to the mid family alone the list loses K5a, K5b and K6b (test_mid_family_alone_is_not_enough): under the row cap no
range gets a third group, so no block runs a second tile.  K3 does NOT go missing there, other than the plan for this file
expected: a ragged hole is one to three pairs wide, and some of the ~100 tile starts of a layer meet one of the 20..48 holes in
most mid cases (K4a stays too: the 15- and 16-frame utterances of a ragged case are one or two pairs long each)."""
import numpy as np
import pytest

import fp32_forms_ref as ref

NUM_CU, HIDDEN = 256, 512
SMALL_BATCHES = [([15], False), ([16, 15, 40, 133], False), ([21] * 3, True), ([22] * 3, True), ([77] * 5, True),
                 ([15, 16, 17, 18, 19, 20, 21, 22, 23] * 7, False), ([300] * 40, True), (list(range(15, 90)), False)]


@pytest.mark.parametrize("d", (2, 3))
def test_pair_count_is_the_number_of_pairs(d):
    for T in range(1, 41):
        firsts = [t for t in range(T) if t % (2 * d) < d]            # y(t) leads a pair; y(t + d), where it exists, is its second
        assert ref.wino_pair_count(T, d) == len(firsts), (T, d)
        rows = [ref.pair_first_row(j, d) for j in range(len(firsts))]
        assert rows == firsts, (T, d)
        covered = sorted(rows + [i + d for i in rows if i + d < T])
        assert covered == list(range(T)), f"T'={T} d={d}: every output row belongs to exactly one pair"


def test_pair_bases_leave_room_for_every_utterance():
    rng = np.random.default_rng(5)
    for _ in range(200):
        lengths = rng.integers(15, 60, int(rng.integers(1, 40))).tolist()
        for layer, d in ref.DILATION.items():
            pb = ref.pair_bases(lengths, ref.CUM[layer], d)
            ro = ref.row_offsets(lengths, ref.CUM[layer])
            cnt = [ref.wino_pair_count(int(t), d) for t in np.diff(ro)]
            assert all(pb[u] + cnt[u] <= pb[u + 1] for u in range(len(lengths))), (lengths, d)
            assert pb[-1] == (int(ro[-1]) >> 1) + len(lengths) * d
    for T in (15, 16, 21, 22, 300):
        for layer, d in ref.DILATION.items():
            pb = ref.pair_bases([T] * 7, ref.CUM[layer], d, fixed=True)
            assert list(np.diff(pb)) == [ref.wino_pair_count(T - ref.CUM[layer], d)] * 7


@pytest.mark.parametrize("num_cu,per_cu,n_tiles", [(256, 2, 4), (256, 1, 2), (256, 3, 4), (256, 2, 12), (256, 3, 12), (304, 2, 4),
                                                   (8, 2, 4), (64, 2, 1), (64, 2, 2)])
def test_group_ranges_tile_the_groups(num_cu, per_cu, n_tiles):
    periods = set()
    for G in list(range(1, 700)) + [1000, 1023, 4097]:
        P, period = ref.persistent_grid(num_cu, per_cu, n_tiles, G)
        assert 1 <= P <= G and P * n_tiles <= max(n_tiles, num_cu * per_cu)
        periods.add(period > 0)
        ranges = [ref.group_range(G, P, period, p) for p in range(P)]
        assert ranges[0][0] == 0 and ranges[-1][1] == G
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), (G, P, period)
        sizes = [e - b for b, e in ranges]
        assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1, (G, P, period, sizes)
        if period:      # the extra groups go to first-slot ranges first: blocks p and p + P / 2 of a CU sum to the same work
            assert per_cu == 2 and P * n_tiles == 2 * num_cu
    if (num_cu, per_cu, n_tiles) in ((256, 2, 4), (64, 2, 1), (64, 2, 2)):
        assert periods == {False, True}, "both branches of group_range are walked"


def test_cut_tiles():
    assert ref.cut_tiles(3, 4, 2) == [(3, 1)] and ref.cut_tiles(3, 5, 2) == [(3, 2)] and ref.cut_tiles(3, 8, 2) == [(3, 2), (5, 2), (7, 1)]
    assert ref.cut_tiles(0, 3, 4) == [(0, 3)] and ref.cut_tiles(2, 12, 4) == [(2, 4), (6, 4), (10, 2)] and ref.cut_tiles(0, 8, 4) == [(0, 4), (4, 4)]


@pytest.mark.parametrize("form", ref.FORMS)
@pytest.mark.parametrize("num_cu", (256, 8))
def test_every_valid_pair_and_row_is_in_exactly_one_tile(form, num_cu):
    for lengths, fixed in SMALL_BATCHES:
        for layer in range(5):
            grid = ref.layer_grid(form, layer, lengths, num_cu, HIDDEN, fixed)
            owner = np.zeros(32 * grid.groups_total, dtype=np.int64)
            for tiles in ref.block_tiles(grid):
                assert tiles and all(1 <= G <= grid.unit for _, G in tiles) and all(G == grid.unit for _, G in tiles[:-1])
                for g, G in tiles:
                    owner[32 * g: 32 * (g + G)] += 1
            assert (owner == 1).all(), (form, layer, lengths)
            if grid.kind == "winograd_f23":
                d = ref.DILATION[layer]
                pb = ref.pair_bases(lengths, ref.CUM[layer], d, fixed)
                assert 32 * (grid.groups_total - 1) < pb[-1] <= len(owner)
            else:
                rows = sum(lengths) - len(lengths) * ref.CUM[layer]
                assert 32 * (grid.groups_total - 1) < rows <= len(owner)
            assert grid.blocks == grid.per_col * grid.n_tiles


def test_records_and_grids_of_the_forms():
    lengths = [300] * 64
    for form in ref.FORMS:
        forms, ops, thr = ref.expected_record(form)
        for layer in range(5):
            g = ref.layer_grid(form, layer, lengths, NUM_CU, HIDDEN, True)
            assert (g.kind, g.operands, g.threads) == (forms[layer], ops[layer], thr[layer]), (form, layer)
    # one block per CU over two 256-channel columns; two per CU over four; three per CU over 4 and 12 (tests/test_split3_blocks_gpu.py)
    assert ref.layer_grid("S8", 1, lengths, NUM_CU, HIDDEN, True).blocks == 256
    assert ref.layer_grid("S4", 1, lengths, NUM_CU, HIDDEN, True).blocks == 512
    assert ref.layer_grid("S8", 3, lengths, NUM_CU, HIDDEN, True).per_col == 192
    assert ref.layer_grid("S8", 4, lengths, NUM_CU, HIDDEN, True).per_col == 64
    assert ref.layer_grid("S4", 4, lengths, NUM_CU, HIDDEN, True).per_col == 42


def _coverage(case_list):
    per_case = [{f: ref.classes_met(c.lengths, NUM_CU, f, HIDDEN, c.fixed) for f in ref.FORMS} for c in case_list]
    cases_of = {k: sum(1 for m in per_case if any(k in s for s in m.values())) for k in ref.CLASSES}
    by_form = {f: set().union(*[m[f] for m in per_case]) for f in ref.FORMS}
    return per_case, cases_of, by_form


def _missing(case_list):
    per_case, cases_of, by_form = _coverage(case_list)
    miss = {k for k, v in cases_of.items() if v < 2}
    miss |= {f"{f}:{k}" for f in ("W", "S4", "S8") for k in ("K3", "K4a", "K5b") if k not in by_form[f]}
    miss |= {f"case {i}" for i, m in enumerate(per_case) if not any(m.values())}
    return miss, cases_of


def test_case_list_shape():
    cs = ref.cases(ref.DEFAULT_N, ref.DEFAULT_SEED)
    assert cs == ref.cases(ref.DEFAULT_N, ref.DEFAULT_SEED), "the list is a function of its seed"
    assert len(cs) == 12 and {c.family for c in cs} == set(ref.FAMILIES)
    assert sum(not c.fixed for c in cs) == 8
    for c in cs:
        B, rows = len(c.lengths), sum(c.lengths) - 4 * len(c.lengths)
        assert min(c.lengths) >= 15
        if c.family == "tiny":
            assert 1 <= B <= 6 and max(c.lengths) <= 80
        elif c.family == "many_short":
            assert 300 <= B <= 900 and max(c.lengths) <= 40
        else:
            assert 20 <= B <= 48 and max(c.lengths) <= 400 and min(c.lengths) >= 15
        assert rows <= (ref.DEEP_ROW_CAP if c.family == "many_short" and B >= 720 else ref.ROW_CAP), (c.family, rows)
        if not c.fixed:
            assert 15 in c.lengths and 16 in c.lengths and B >= 3


def test_default_cases_reach_every_class():
    miss, cases_of = _missing(ref.cases(ref.DEFAULT_N, ref.DEFAULT_SEED))
    print("cases per class:", cases_of)
    assert not miss, f"not reached by the default case list: {sorted(miss)}"


def test_mid_family_alone_is_not_enough():
    miss, _ = _missing(ref.cases(ref.DEFAULT_N, ref.DEFAULT_SEED, families=("mid",)))
    assert {"K5a", "K5b", "K6b", "W:K5b", "S4:K5b", "S8:K5b"} <= miss, sorted(miss)


def test_tiny_family_alone_is_not_enough():
    miss, _ = _missing(ref.cases(ref.DEFAULT_N, ref.DEFAULT_SEED, families=("tiny",)))
    assert {"K5a", "K5b", "K10", "W:K5b", "S4:K5b", "S8:K5b"} <= miss, sorted(miss)
