"""The geometry of the fp32 frame-level kernel forms restated on the host, in plain Python: no GPU, no import from the product.

What is restated, and from where (csrc/):
  wino_pair_count, pair bases     tdnn_common.h; tdnn_wino_rows.h (set_rows_impl: pb, first_utterance)
  persistent_grid                 xvec_api.hip (and plan_layer: groups_total, n_tiles, the blocks per CU of each form)
  group_range, both branches      tdnn_common.h
  the cut of a range into tiles   tdnn_wino.hip / tdnn_wino_s3.hip / tdnn_wino_s3w.hip: two 32-pair groups per tile and an odd
                                  one-group tail; tdnn_layer_impl.h (tdnn_body): four 32-row groups and ONE tail tile of G < 4
From it: the tile list of every block of every layer for (lengths, num_cu, form), and the classes K1..K10 a case meets
(classify).  tests/test_fuzz_fp32_forms.py checks the restatement against closed forms and the default case list's coverage;
tests/test_fuzz_fp32_forms_gpu.py ties it to what ran (the block counts of the launch record) and walks the cases.

Layers are indexed 0..4 as in time_context_layers; "layers 2-3" of the prose are indices 1 and 2 (dilation 2 and 3), "layers
4-5" indices 3 and 4.  A batch is a list of utterance lengths in input frames; a fixed-length batch is the same list with
fixed=True (the kernels then take the row and pair bases from a product, not from the offsets array).

A Winograd tile of G groups is taken as its 32 G pairs -- the pairs whose products it forms and whose rows it stores.  (set_rows
tables 64 pairs for every tile, the tail tile included; the second half of a tail tile's table is never read.)

The classes (classify), counted per tile, range or utterance of the Winograd layers of a form:
  K1_d2, K1_d3  an utterance with a one-output pair (i + d >= T'), at d = 2 / d = 3
  K2            hole pairs of a ragged batch lie inside a tile
  K3            a tile's first pair lies in a hole behind its utterance's last pair (set_rows_impl clamps j0)
  K4a / K4b     three or more utterance starts behind a tile's first pair / none (the block-uniform walk of set_rows_impl)
  K5a / K5b     a block runs two tiles or more / u_tile advances by two utterances or more between two of them
  K6a / K6b     a block's range is one group / 3, 5, .. groups: two-group tiles, then the odd tail tile
  K7            pairs past the end of the pair axis lie in the last tile
  K8a / K8b     an utterance other than the first starts on an even / odd compact row of a ragged batch (pb takes row >> 1)
and of layers 4-5 under every form:
  K9            a 32-row group holds rows of three utterances or more (the row masks of the pooling epilogue)
  K10           a block runs two tiles or more and ends in a tail tile of G < 4

The forms (the handles of the GPU test):
  D    every layer direct (128x128 kernel, two blocks per CU)
  W    layers 2-3 fp32 Winograd F(2,3), 128-channel tiles, two blocks per CU; the rest direct
  S4   layers 2-3 Winograd on bf16_split3 operands, four waves (128-channel tiles, two blocks per CU); layers 4-5 bf16_split3
       at two blocks per CU
  S8   layers 2-3 the same on eight waves (256-channel tiles, one block per CU); layers 4-5 bf16_split3 at three blocks per CU"""
from collections import namedtuple

import numpy as np

CUM = (4, 8, 14, 14, 14)              # frames of context consumed after layers 1..5 (xvec_api.hip, plan_stack)
DILATION = {1: 2, 2: 3}               # the Winograd layers: three taps d frames apart
FORMS = ("D", "W", "S4", "S8")
POOL_CHANNELS = 1500
WINO_CLASSES = ("K1_d2", "K1_d3", "K2", "K3", "K4a", "K4b", "K5a", "K5b", "K6a", "K6b", "K7", "K8a", "K8b")
TAIL_CLASSES = ("K9", "K10")
CLASSES = WINO_CLASSES + TAIL_CLASSES

LayerGrid = namedtuple("LayerGrid", "kind operands threads unit groups_total n_tiles per_col pair_period blocks")


def round_up(v, m):
    return -(-v // m) * m


# ------------------------------------------------------------------------------------------------ pair space
def wino_pair_count(T, d):
    """Pairs (t, t + d) of an utterance with T output frames (tdnn_common.h)."""
    r = T % (2 * d)
    return d * (T // (2 * d)) + min(r, d)


def pair_first_row(j, d):
    """Output row i of pair j's first output y(i); its second is y(i + d) (set_rows_impl: i = jl + d * (jl / d))."""
    return j + d * (j // d)


def row_offsets(lengths, cum):
    """First compact output row of every utterance (and the end of the last) behind `cum` frames of context."""
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64) - cum)])


def pair_bases(lengths, cum, d, fixed=False):
    """First pair of every utterance, and pb[B] = the length of the pair axis (plan_layer sizes groups_total from it).
    Ragged: (row_off >> 1) + u d, which leaves holes; fixed: u * p_fixed, which leaves none."""
    ro = row_offsets(lengths, cum)
    u = np.arange(len(lengths) + 1, dtype=np.int64)
    if fixed:
        assert len(set(lengths)) == 1
        return u * wino_pair_count(int(lengths[0]) - cum, d)
    return (ro >> 1) + u * d


# ------------------------------------------------------------------------------------------------ grid and ranges
def persistent_grid(num_cu, per_cu, n_tiles, groups_total):
    """(blocks per column, pair_period) of a persistent kernel of the 128x128 family (xvec_api.hip)."""
    per_col = max(1, min(num_cu * per_cu // n_tiles, groups_total))
    nwg = per_col * n_tiles
    ok = per_cu == 2 and nwg == 2 * num_cu and nwg % 16 == 0 and (nwg // 8) % (2 * n_tiles) == 0
    return per_col, ((nwg // 8) // n_tiles if ok else 0)


def group_range(groups_total, P, pair_period, p):
    """[begin, end) of the groups of range p of P (tdnn_common.h): both branches."""
    if pair_period > 0:
        PQ, hq = pair_period, pair_period >> 1
        base, rem = groups_total // P, groups_total % P
        rem1 = min(rem, P >> 1)
        rem2 = rem - rem1
        xq, w = p // PQ, p % PQ
        nf = xq * hq + min(w, hq)
        ns = xq * hq + (w - hq if w > hq else 0)
        begin = base * p + min(nf, rem1) + min(ns, rem2)
        extra = (nf < rem1) if w < hq else (ns < rem2)
        return begin, begin + base + (1 if extra else 0)
    return groups_total * p // P, groups_total * (p + 1) // P


def cut_tiles(begin, end, unit):
    """[(first group, G)] of a block's range.  unit 2 (Winograd): `for (; g + 2 <= g_end; g += 2) tile<2>; if (g < g_end) tile<1>`;
    unit 4 (tdnn_body): tiles of four, then one tile of the 1..3 groups left."""
    out, g = [], begin
    while g + unit <= end:
        out.append((g, unit))
        g += unit
    if g < end:
        out.append((g, end - g))
    return out


def layer_grid(form, layer, lengths, num_cu, hidden=512, fixed=False, split3_blocks_cu=3):
    """What plan_layer chooses for `layer` of the fp32 path under the knobs of handle `form` (module docstring)."""
    B, total = len(lengths), int(np.sum(lengths))
    rows_out = total - B * CUM[layer]
    n_pad = round_up(POOL_CHANNELS if layer == 4 else hidden, 128)
    kind, operands, threads, unit, per_cu, n_tiles = "direct", "fp32", 256, 4, 2, n_pad // 128
    groups_total = -(-rows_out // 32)
    if layer in (3, 4) and form in ("S4", "S8"):
        kind, operands, per_cu = "bf16_split3", "bf16_split3", min(2, split3_blocks_cu) if form == "S4" else split3_blocks_cu
    elif layer in DILATION and form != "D":
        kind, unit = "winograd_f23", 2
        groups_total = -(-int(pair_bases(lengths, CUM[layer], DILATION[layer], fixed)[-1]) // 32)
        if form != "W":
            operands = "bf16_split3"
            if form == "S8" and n_pad % 256 == 0:
                threads, per_cu, n_tiles = 512, 1, n_pad // 256
    per_col, pair_period = persistent_grid(num_cu, per_cu, n_tiles, groups_total)
    return LayerGrid(kind, operands, threads, unit, groups_total, n_tiles, per_col, pair_period, per_col * n_tiles)


def block_tiles(grid):
    """The tile list [(first group, G)] of every range of a layer's grid (each is run by n_tiles blocks, one per channel column)."""
    return [cut_tiles(*group_range(grid.groups_total, grid.per_col, grid.pair_period, p), grid.unit) for p in range(grid.per_col)]


def expected_record(form):
    """(forms, operands, threads) of the five layers as the library reports them for handle `form` at width 512."""
    forms, ops, thr = ["direct"] * 5, ["fp32"] * 5, [256] * 5
    if form != "D":
        forms[1:3] = ["winograd_f23"] * 2
    if form in ("S4", "S8"):
        ops[1:5] = ["bf16_split3"] * 4
        forms[3:5] = ["bf16_split3"] * 2
    if form == "S8":
        thr[1:3] = [512] * 2
    return forms, ops, thr


# ------------------------------------------------------------------------------------------------ classes
def classify(lengths, num_cu, form, hidden=512, fixed=False):
    """{class: count} for one case under one form, and the utterances whose pair-space start lies in a tile marked K3 or K4a:
    (counts, marked).  The classes of layers 2-3 are counted over the form's Winograd layers (none under D), those of layers
    4-5 over both layers under every form."""
    n = {k: 0 for k in CLASSES}
    marked = set()
    B = len(lengths)
    for layer, d in DILATION.items():
        grid = layer_grid(form, layer, lengths, num_cu, hidden, fixed)
        if grid.kind != "winograd_f23":
            continue
        ro = row_offsets(lengths, CUM[layer])
        pb = pair_bases(lengths, CUM[layer], d, fixed)
        to = np.diff(ro)
        cnt = np.array([wino_pair_count(int(t), d) for t in to], dtype=np.int64)
        last = pb[:-1] + cnt                      # one past the last valid pair of every utterance
        n[f"K1_d{d}"] += int(sum(1 for t in to if t % (2 * d)))       # T' = 2dk + r, r > 0: the last min(r, d) pairs have i + d >= T'
        if not fixed:
            n["K8a"] += int(np.sum(ro[1:B] % 2 == 0))
            n["K8b"] += int(np.sum(ro[1:B] % 2 == 1))
        for tiles in block_tiles(grid):
            size = sum(G for _, G in tiles)
            n["K5a"] += len(tiles) >= 2
            n["K6a"] += size == 1
            n["K6b"] += size >= 3 and size % 2 == 1
            prev_u = None
            for g, G in tiles:
                q0, q1 = 32 * g, 32 * (g + G)
                ut = min(int(np.searchsorted(pb[:B], q0, side="right")) - 1, B - 1)      # largest u with pb[u] <= q0
                u_end = max(ut + 1, int(np.searchsorted(pb[:B], q1, side="left")))        # first u with pb[u] >= q1
                inside = list(range(ut + 1, u_end))                                        # the starts set_rows walks
                holes = 0 if fixed else sum(max(0, min(q1, int(pb[u + 1])) - max(q0, int(last[u]))) for u in range(ut, u_end))
                # (fixed: the pair axis ends at pb[B] with no hole behind the last utterance; ragged: pb[B] counts one)
                n["K2"] += holes > 0
                k3 = q0 >= last[ut]
                n["K3"] += bool(k3)
                n["K4a"] += len(inside) >= 3
                n["K4b"] += len(inside) == 0
                if k3 or len(inside) >= 3:
                    marked.update([ut] + inside)
                if prev_u is not None:
                    n["K5b"] += ut - prev_u >= 2
                prev_u = ut
                n["K7"] += q1 > pb[B]
    ro = row_offsets(lengths, CUM[3])
    for g in range(-(-int(ro[-1]) // 32)):
        lo, hi = 32 * g, min(32 * g + 32, int(ro[-1]))
        n["K9"] += int(np.searchsorted(ro, hi, side="left")) - (int(np.searchsorted(ro, lo, side="right")) - 1) >= 3
    for layer in (3, 4):
        for tiles in block_tiles(layer_grid(form, layer, lengths, num_cu, hidden, fixed)):
            n["K10"] += len(tiles) >= 2 and tiles[-1][1] < 4
    return n, sorted(marked)


def classes_met(lengths, num_cu, form, hidden=512, fixed=False):
    return {k for k, v in classify(lengths, num_cu, form, hidden, fixed)[0].items() if v}


# ------------------------------------------------------------------------------------------------ the case list
FAMILIES = ("tiny", "many_short", "mid")
ROW_CAP = 12000                       # layer-1 output rows of a case (a case stays within a few seconds including its oracle)
# The many-short family at 256 CUs and width 512: every Winograd form has 128 ranges per column (2 * 256 / 4 four-wave
# columns, 256 / 2 eight-wave ones), a range runs a second tile from its third group on, and layer 2's pair axis is
# (layer-1 rows) / 2 pairs long (sum/2 - 4B + 2B) -- 187 groups at 12 000 rows: one tile per block.  Every second case of the
# family is therefore a DEEP one: B in 720..900 under a cap at which 128 ranges of layer 2 get three groups (> 2 * 128 * 32
# pairs = 16 384 rows) whatever the lengths drawn.
DEEP_ROW_CAP = 21000
Case = namedtuple("Case", "family lengths fixed seed")


def _fit(lengths, lo, cap, rng, keep=()):
    """Shorten randomly chosen utterances (never below `lo`, and none of `keep`) until the layer-1 rows fit `cap`."""
    over = int(np.sum(lengths - 4)) - cap
    while over > 0:
        i = int(rng.integers(len(lengths)))
        if i in keep:
            continue
        cut = min(over, int(lengths[i]) - lo, max(1, int(lengths[i]) // 3))
        lengths[i] -= cut
        over -= cut
    return lengths


def make_case(family, ragged, rng, deep=False):
    """One case: tiny (B in 1..6 -- 3..6 when ragged --, lengths 15..80), many short (B in 300..900, lengths 15..40; deep: B in
    720..900, lengths 28..40) or mid (B in 20..48, padded length up to 400, lengths from a quarter of it upwards).  A ragged
    case holds one utterance of 15 frames (a single pooled frame) and one of 16; its padded length is its longest utterance."""
    seed = int(rng.integers(1 << 30))
    if family == "tiny":
        B, lo, T = int(rng.integers(3 if ragged else 1, 7)), 15, int(rng.integers(15 if not ragged else 17, 81))
    elif family == "many_short":
        B, lo, T = (int(rng.integers(720, 901)) if deep else int(rng.integers(300, 901))), (28 if deep else 15), int(rng.integers(34, 41))
    else:
        B, T = int(rng.integers(20, 49)), int(rng.integers(60, 401))
        lo = max(15, T // 4)
    cap = DEEP_ROW_CAP if deep else ROW_CAP
    if not ragged:
        T = max(15, min(T, cap // B + 4))
        return Case(family, [T] * B, True, seed)
    lengths = rng.integers(lo, T + 1, B).astype(np.int64)
    others = [int(i) for i in rng.permutation(B) if i != int(np.argmax(lengths))][:2]
    for s, v in zip(others, (15, 16)):
        lengths[s] = v
    lengths = _fit(lengths, 15, cap, rng, keep=others)
    return Case(family, [int(v) for v in lengths], False, seed)


def cases(n, seed, families=FAMILIES):
    """The seeded case list: the families in turn, two of three cases ragged; every second many-short case a deep one."""
    rng = np.random.default_rng(seed)
    out, shorts = [], 0
    for i in range(n):
        family = families[i % len(families)]
        deep = family == "many_short" and shorts % 2 == 0
        shorts += family == "many_short"
        out.append(make_case(family, (i // len(families) + i) % 3 != 0, rng, deep))
    return out


DEFAULT_N, DEFAULT_SEED = 12, 2025
