"""The LDS image of the Winograd split3 kernel's V planes (csrc/wino_s3_lds_map.h) on the CPU: tests/abi/wino_s3_lds_map_dump.cpp,
compiled with the host compiler, prints the store offset of every thread and the read offset of every lane; the test lays
them over both buffers and all twelve (product, plane) blocks as the kernel does (csrc/tdnn_wino_s3.hip: s3_vstore, WS3_RD)
and checks that the image is a bijection that hands every lane its MFMA operand, and that no store and no read instruction
has two lanes of one service group on one bank (MI355X: ds_write_b64 is served in 4 groups of 16 consecutive lanes with 32
banks of 4 bytes, ds_read_b128 in the 4 groups below with 64 banks).  No GPU, no HIP library."""
import pytest

from hipcc_support import host_program, needs_host_cxx

pytestmark = needs_host_cxx

# lanes served together by ds_read_b128
READ_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
               [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
READ_GROUPS += [[l + 32 for l in g] for g in READ_GROUPS]
WRITE_GROUPS = [list(range(16 * j, 16 * j + 16)) for j in range(16)]       # per wave: 4 groups of 16 consecutive lanes


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    m = {"st": {}, "rd": {}}
    for line in host_program("wino_s3_lds_map_dump", tmp_path_factory.mktemp("wino_s3_lds_map")).output().splitlines():
        f = line.split()
        if f[0] == "const":
            m["k"], m["pairs"], m["plane"], m["stage"] = map(int, f[1:])
        elif f[0] == "st":
            m["st"][int(f[1])] = int(f[2])
        else:
            m["rd"][(int(f[1]), int(f[2]))] = int(f[3])
    assert len(m["st"]) == 256 and len(m["rd"]) == 128
    return m


def _blocks(m):
    """Byte address of every (buffer, product, plane) block, as the kernel places them."""
    return [buf * m["stage"] + (3 * k + pl) * m["plane"] for buf in range(2) for k in range(4) for pl in range(3)]


def test_constants(maps):
    assert (maps["k"], maps["pairs"], maps["plane"], maps["stage"]) == (16, 64, 64 * 32, 12 * 64 * 32)
    assert 2 * maps["stage"] == 2 * (4 * 3 * 64 * 16 * 2)          # what tests/test_wino_split3_resources.py plans per block


def test_every_byte_written_once_and_read_as_the_mfma_operand(maps):
    """Thread tid stages k 4 (tid & 3) .. + 3 (8 bytes) of pair (tid >> 3) + 32 ((tid >> 2) & 1); lane (r, h) of pair group g
    must read k 8 h .. 8 h + 7 of pair 32 g + r, in order."""
    for base in _blocks(maps):
        owner = {}                                  # byte address -> (pair, k-byte)
        for tid in range(256):
            pair = (tid >> 3) + 32 * ((tid >> 2) & 1)
            a = base + maps["st"][tid]
            assert a % 8 == 0
            for b in range(8):
                assert a + b not in owner, f"byte {a + b} written twice"
                owner[a + b] = (pair, (tid & 3) * 8 + b)
        assert sorted(owner) == list(range(base, base + maps["plane"])), "the block is not covered exactly"
        for g in range(2):
            for lane in range(64):
                r, h = lane & 31, lane >> 5
                a = base + maps["rd"][(g, lane)]
                assert a % 16 == 0
                assert [owner[a + b] for b in range(16)] == [(32 * g + r, 16 * h + b) for b in range(16)], (g, lane)


def _conflicts(addrs, width, n_banks):
    """Pairs of lanes whose accesses of `width` bytes touch one bank at different addresses."""
    seen, bad = {}, []
    for lane, a in addrs:
        for d in range(0, width, 4):
            bank = ((a + d) // 4) % n_banks
            if bank in seen and seen[bank][1] != a + d:
                bad.append((seen[bank][0], lane, bank))
            seen[bank] = (lane, a + d)
    return bad


def test_stores_are_conflict_free(maps):
    for base in _blocks(maps):
        for grp in WRITE_GROUPS:
            bad = _conflicts([(t, base + maps["st"][t]) for t in grp], 8, 32)
            assert not bad, f"ds_write_b64 lanes {grp[0]}..{grp[-1]} at block {base}: {bad[:4]}"


def test_fragment_reads_are_conflict_free(maps):
    for base in _blocks(maps):
        for g in range(2):
            for grp in READ_GROUPS:
                bad = _conflicts([(l, base + maps["rd"][(g, l)]) for l in grp], 16, 64)
                assert not bad, f"ds_read_b128 pair group {g}, lanes {grp}: {bad[:4]}"


def test_the_checks_see_the_plain_image(maps):
    """The row-major image the kernel had (row p at 32 p, no swap) is two-way conflicted on both sides: the two checks above
    are not vacuous."""
    plain_st = {t: ((t >> 3) + 32 * ((t >> 2) & 1)) * 32 + (t & 3) * 8 for t in range(256)}
    plain_rd = {l: (l & 31) * 32 + (l >> 5) * 16 for l in range(64)}
    assert _conflicts([(t, plain_st[t]) for t in WRITE_GROUPS[0]], 8, 32)
    assert _conflicts([(l, plain_rd[l]) for l in READ_GROUPS[0]], 16, 64)
