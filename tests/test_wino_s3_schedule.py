"""The K loop of the Winograd split3 kernel (csrc/tdnn_wino_s3.hip) as hipcc compiles it for gfx950, on the CPU: the operand
look-ahead the source asks for must be in the machine code.  hipcc once sank all twelve U-plane loads of the next chunk behind
the chunk's last MFMAs and copied the fragments into place on the loop's back edge, so that every chunk waited for a whole
vector-memory round trip; these checks pin the order against a compiler that does it again.

The K loop's MFMA block is the basic block that holds the loop's s_barrier (one for the two-group tile, one for the odd
tail tile); it starts with the chunk's four input-row loads and ends with the loop's branch.  In it:
  * no run of more than four buffer_load instructions without an MFMA between them (the head's four input rows; the three U
    fragments of a product behind its last MFMA);
  * every product's U loads are there: 4 + 4 x 3 loads, in five runs;
  * no 64-bit (or wider) register move between the barrier and the end of the block, and none anywhere in the loop -- from the
    targets of its back edges to the last of them, which takes in the chunk's head (V stores, the step of the load stream) and
    the epilogue -- that copies a loaded fragment: a vector-register source that a buffer_load_dwordx4 or ds_read_b128 wrote
    and no instruction has overwritten since.  (The head's 64-bit row arithmetic moves scalar pairs and its own values; those are not fragments.)
    A fragment is loaded into the registers its MFMAs read;
  * the waits for vector memory inside the block are counted, never vmcnt(0)."""
import re

import pytest

from hipcc_support import kernel_asm, needs_hipcc

WIDE_MOV = re.compile(r"v_mov_b64|v_pk_mov_b32|v_mov_b128|v_accvgpr_mov")


def _blocks():
    """[(label, [instructions])] of the compiled file, in layout order."""
    blocks, cur = [], None
    for line in kernel_asm("tdnn_wino_s3.hip").splitlines():
        s = line.split(";")[0].strip()
        m = re.match(r"^([.\w$]+):$", s)
        if m:
            cur = (m.group(1), [])
            blocks.append(cur)
        elif s and not s.startswith(".") and cur is not None:
            cur[1].append(s)
    return blocks


@pytest.fixture(scope="module")
def compiled():
    return _blocks()


@pytest.fixture(scope="module")
def loops(compiled):
    """The instruction lists of the kernel's basic blocks that hold an s_barrier and at least 24 MFMAs."""
    out = [b for _, b in compiled if any(i.startswith("s_barrier") for i in b) and sum(i.startswith("v_mfma") for i in b) >= 24]
    assert len(out) == 2, f"expected the K loops of s3_tile<2> and s3_tile<1>, found {len(out)} blocks"
    return out


@pytest.fixture(scope="module")
def loop_regions(compiled):
    """Per K loop: (its MFMA block, every instruction of the loops around it in layout order, the MFMA block first): from the
    earliest target to the last of the branches behind the block that jump to it or in front of it.  Only loops that
    enclose the block have such branches: the K loop (its chunk head reaches the block on two paths, with and without new
    row tables) and the tile loop with the epilogue."""
    index = {label: k for k, (label, _) in enumerate(compiled)}
    out = []
    for at, (label, b) in enumerate(compiled):
        if not (any(i.startswith("s_barrier") for i in b) and sum(i.startswith("v_mfma") for i in b) >= 24):
            continue
        edges = []
        for j in range(at, len(compiled)):
            for i in compiled[j][1]:
                m = re.match(r"s_c?branch\S*\s+(\S+)$", i)
                if m and index.get(m.group(1), len(compiled)) <= at:
                    edges.append((index[m.group(1)], j))
        assert edges, f"no loop around {label}"
        t, j = min(e[0] for e in edges), max(e[1] for e in edges)
        rest = [i for _, blk in compiled[at + 1:j + 1] + compiled[t:at] for i in blk]
        out.append((b, b + rest))
    assert len(out) == 2
    return out


def _regs(operand):
    """Vector registers an operand such as v[4:7] or v12 names."""
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", operand)
    return {int(m.group(1))} if m else set()


def _load_runs(block):
    runs, n = [], 0
    for ins in block:
        if ins.startswith("buffer_load"):
            n += 1
        elif ins.startswith("v_mfma") and n:
            runs.append(n)
            n = 0
    if n:
        runs.append(n)
    return runs


@needs_hipcc
def test_u_loads_stay_behind_their_product(loops):
    for b in loops:
        n_mfma = sum(i.startswith("v_mfma") for i in b)
        assert n_mfma in (24, 48), n_mfma
        runs = _load_runs(b)
        print("MFMAs", n_mfma, "buffer_load runs", runs)
        assert max(runs) <= 4, f"a cluster of {max(runs)} buffer loads with no MFMA between them: {runs}"
        assert runs == [4, 3, 3, 3, 3], runs
        assert b[-1].startswith(("s_cbranch", "s_branch")), b[-1]


@needs_hipcc
def test_no_fragment_copies_behind_the_barrier(loops):
    for b in loops:
        at = max(i for i, ins in enumerate(b) if ins.startswith("s_barrier"))
        tail = b[at:]
        assert any(i.startswith(("s_cbranch", "s_branch")) for i in tail)
        moves = [i for i in tail if WIDE_MOV.match(i)]
        assert not moves, moves


@needs_hipcc
def test_vector_memory_waits_are_counted(loops):
    for b in loops:
        waits = [int(m.group(1)) for i in b for m in [re.search(r"vmcnt\((\d+)\)", i)] if i.startswith("s_waitcnt") and m]
        print("vmcnt waits", waits)
        assert waits and min(waits) >= 13, waits       # tdnn_wino_s3.hip, s3_tile: 13 younger entries stay in flight, never a drain


@needs_hipcc
def test_no_fragment_copies_anywhere_in_the_loop(loop_regions):
    for block, region in loop_regions:
        assert len(region) > len(block)                          # the chunk's head is in the region
        # registers that hold a loaded value: written by a 16-byte load and by nothing since (a walk in layout order, once
        # round the loop, starting behind the MFMA block, where every fragment register has been loaded)
        is_load = lambda i: i.startswith(("buffer_load_dwordx4", "ds_read_b128"))
        holds = set()
        for i in block:
            if is_load(i):
                holds |= _regs(i.split()[1].rstrip(","))
        assert len(holds) >= 12 * 4 + 2 * 3 * 4, len(holds)      # twelve U fragments and the two fragment sets
        copies, n_wide = [], 0
        for i in region[len(block):] + block:
            ops = [o.strip() for o in i.split(None, 1)[1].split(",")] if " " in i else []
            if WIDE_MOV.match(i):
                n_wide += 1
                if any(_regs(o) & holds for o in ops[1:]):
                    copies.append(i)
            if is_load(i):
                holds |= _regs(ops[0])
            elif ops and not i.startswith(("ds_write", "buffer_store", "global_store", "s_")):
                holds -= _regs(ops[0])
        print("wide moves in the loop", n_wide, "of loaded values", copies)
        assert not copies, copies
