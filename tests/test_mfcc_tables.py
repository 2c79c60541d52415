"""The host-built tables of the MFCC front end (csrc/mfcc_tables.h) on the CPU: tests/abi/mfcc_tables_dump.cpp, compiled once
per session with the host compiler, writes the blob and its offsets for a configuration; every table is checked against the
oracle's formulas or against the layout rule the kernel reads it by (csrc/mfcc.hip).  No GPU, no HIP library."""
import functools
import os

import numpy as np
import pytest

import mfcc_oracle as mo
from conftest import ROOT
from hipcc_support import host_program, needs_host_cxx

pytestmark = needs_host_cxx

DEFAULTS = dict(samplerate=16000, winlen=0.025, winstep=0.01, numcep=24, nfilt=26, nfft=512, lowfreq=0.0, highfreq=0.0,
                preemph=0.97, ceplifter=22, append_energy=1)
# (configuration, allow_banded, kernel form: 0 general, 1 nfft-512 with the dense filterbank, 2 with the banded one -- what
#  tests/test_mfcc.py::test_kernel_form_of_a_plan expects; None: decided by _expected_form alone)
CASES = {
    "reference": (dict(), True, 2),
    "reference-dense": (dict(), False, 1),
    "telephone-band": (dict(nfilt=20, numcep=13, lowfreq=300.0, highfreq=3400.0), True, None),
    "32x32": (dict(nfilt=32, numcep=32), True, None),              # 16 bin groups: more than the banded form holds -> dense
    "40-filters": (dict(nfilt=40, numcep=20), True, 0),
    "nfft256": (dict(nfft=256, winlen=0.016), True, 0),
    "nfft1024": (dict(nfft=1024), True, 0),
    "nfft2048": (dict(nfft=2048, winlen=0.05, nfilt=40, numcep=13), True, 0),   # odd log2: the extra W_N pass
    "no-lifter": (dict(ceplifter=0), True, 2),
    # found by searching the builder (see test_fall_back_branches_are_reached)
    "wide-triangles": (dict(nfilt=4, numcep=4), True, 1),         # a filter in more than 8 groups -> dense
    "unusually-dense": (dict(samplerate=1000000, nfilt=17, numcep=13), True, 0),   # 21 (tile, bin group) products -> general
}
FAST = [k for k, (kw, _, _) in CASES.items() if {**DEFAULTS, **kw}["nfft"] == 512 and {**DEFAULTS, **kw}["nfilt"] <= 32]


@pytest.fixture(scope="session")
def dump_exe(tmp_path_factory):
    return host_program("mfcc_tables_dump", tmp_path_factory.mktemp("mfcc_tables"), include=[os.path.join(ROOT, "include")]).output


class Tables:
    def __init__(self, exe, kw, allow_banded):
        self.cfg = {**DEFAULTS, **kw}
        head, _, raw = exe(*[str(v) for v in self.cfg.values()], str(int(allow_banded)), text=False).partition(b"\n")
        self.rc = int(head.split()[0].split(b"=")[1])
        self.msg = head.decode().partition("msg=")[2]
        if self.rc:
            return
        fields = {k: int(v) for k, v in (item.split("=") for item in head.decode().split())}
        self.blob = np.frombuffer(raw, dtype="<f4")
        assert self.blob.size == fields.pop("blob")
        self.__dict__.update(fields)                   # the offsets, the scalar fields and the layout constants (kEx, ...)

    def f(self, off, n):
        return self.blob[off:off + n]

    def i(self, off, n):
        return self.blob[off:off + n].view("<i4")

    @property
    def nfft512(self):                                 # the nfft-512 kernel's tables were built (it may still not be chosen)
        return self.cfg["nfft"] == 512 and self.cfg["nfilt"] <= 32 and self.cfg["numcep"] <= 32

    @property
    def form(self):
        return 0 if not self.fast else 1 if self.f_band < 0 else 2


@pytest.fixture(scope="session")
def tables(dump_exe):
    @functools.lru_cache(maxsize=None)
    def get(name):
        kw, allow, _ = CASES[name]
        return Tables(dump_exe, kw, allow)
    return get


def _ulps(a, b):
    """distance in float32 representable values (0 for +0 against -0)"""
    def key(x):
        v = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(v < 0, -(v & 0x7FFFFFFF), v)
    return np.abs(key(a) - key(b))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _oracle_bins(c):
    high = c["highfreq"] or c["samplerate"] / 2
    mel = np.linspace(mo.hz2mel(c["lowfreq"]), mo.hz2mel(high), c["nfilt"] + 2)
    return np.floor((c["nfft"] + 1) * mo.mel2hz(mel) / c["samplerate"])


def _oracle_fb(c):
    return mo.get_filterbanks(c["nfilt"], c["nfft"], c["samplerate"], c["lowfreq"], c["highfreq"] or None)


def _oracle_dctl(c):
    rows = mo.dct2_ortho(np.eye(c["nfilt"]), c["numcep"]).T                      # basis x scale, [numcep, nfilt]
    return rows * mo.lifter_coeffs(c["numcep"], c["ceplifter"])[:, None] if c["ceplifter"] > 0 else rows


def _sparse_expanded(t):
    c = t.cfg
    w, lo, off = t.f(t.fbw_off, t.fblo_off - t.fbw_off), t.i(t.fblo_off, c["nfilt"]), t.i(t.fboff_off, c["nfilt"] + 1)
    full = np.zeros((c["nfilt"], t.nbins), np.float32)
    for j in range(c["nfilt"]):
        full[j, lo[j]:lo[j] + off[j + 1] - off[j]] = w[off[j]:off[j + 1]]
    return full, lo, off


def _dense2(t):
    """[32][256]: the filterbank the nfft-512 kernel multiplies with -- zero padded, bin 256 dropped, x 2 (its power rows are halves)"""
    full, _, _ = _sparse_expanded(t)
    d = np.zeros((32, 256), np.float32)
    d[:t.cfg["nfilt"]] = 2.0 * full[:, :256]
    return d


def _greedy_groups(d, cap, max_groups):
    """The banded form's rule restated: consecutive bins, at most `cap` per group, the filters of a group inside a window of four
    starting at its first weighted bin's lowest filter (at most 28).  [(first bin, bins, first filter)] or None: does not fit."""
    live = [np.flatnonzero(d[:, k]) for k in range(256)]
    groups, k = [], 0
    while k < 256:
        if len(groups) == max_groups:
            return None
        k0, a = k, None
        while k < 256 and k - k0 < cap:
            if live[k].size:
                if a is None:
                    a = min(int(live[k][0]), 28)
                if live[k][-1] > a + 3:
                    break
            k += 1
        if k == k0:
            return None
        groups.append((k0, k - k0, a or 0))
    return groups


def _expected_form(t, allow_banded):
    c = t.cfg
    if c["nfft"] != 512 or c["nfilt"] > 32 or c["numcep"] > 32:
        return 0
    d = _dense2(t)
    tiles = [np.flatnonzero(d[16 * s:16 * s + 16].reshape(16, 16, 16).any(axis=(0, 2))) for s in range(2)]
    if sum(int(g[-1] - g[0] + 1) for g in tiles if g.size) > 4 * t.kMaxItems:
        return 0
    groups = _greedy_groups(d, t.kBandCap, t.kBandGroups)
    if not allow_banded or groups is None:
        return 1
    per_filter = [sum(1 for k0, n, a in groups if a <= f <= a + 3 and d[f, k0:k0 + n].any()) for f in range(32)]
    return 2 if max(per_filter) <= t.kBandGat else 1


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_form(tables, name):
    t = tables(name)
    _, allow, form = CASES[name]
    assert t.rc == 0 and t.form == _expected_form(t, allow)
    if form is not None:
        assert t.form == form
    c = t.cfg
    assert (t.frame_len, t.frame_step) == (mo._round_half_up(np.float32(c["winlen"]).item() * c["samplerate"]),
                                           mo._round_half_up(np.float32(c["winstep"]).item() * c["samplerate"]))
    assert 1 << t.log2n == c["nfft"] and t.nbins == c["nfft"] // 2 + 1 and t.table_floats % 2 == 0
    if t.nfft512:
        assert t.f_tw1 % 4 == 0 and t.f_tw1 >= t.table_floats and (t.f_band < 0 or t.f_band % 4 == 0)


def test_fall_back_branches_are_reached(tables):
    """Both automatic fall-backs exist within nfilt <= 32.  A search of the builder over samplerate x nfilt x lowfreq x highfreq
    found the dense filterbank for two reasons: more than 15 bin groups (nfilt = 32, also nfilt >= 29 at the defaults) and a filter
    in more than 8 groups (nfilt <= 5: f_gat_n stops at 8).  The general kernel for more than 20 (tile, bin group) products it
    found only at sample rates far above audio (1 MHz, nfilt = 17: 21 products; at most 20 up to 192 kHz)."""
    assert tables("32x32").form == 1 and tables("32x32").f_gat_n == 0
    assert _greedy_groups(_dense2(tables("32x32")), 19, 15) is None
    assert tables("wide-triangles").form == 1 and tables("wide-triangles").f_gat_n == 8
    t = tables("unusually-dense")
    assert t.form == 0 and t.nfft512 and t.f_n0 + t.f_n1 == 21


@pytest.mark.parametrize("name", list(CASES))
def test_sparse_filterbank_is_the_packages(tables, name):
    """Bit equality with the oracle rounded to float32 (numpy.linspace and the header's expression gave the same bin edges and
    weights in every configuration here; no ulp bar was needed)."""
    t = tables(name)
    c = t.cfg
    full, lo, off = _sparse_expanded(t)
    ref, bins = _oracle_fb(c), _oracle_bins(c)
    assert off[0] == 0 and off[-1] == t.fblo_off - t.fbw_off
    assert np.array_equal(lo, bins[:-2].astype(int)) and np.array_equal(np.diff(off), (bins[2:] - bins[:-2]).astype(int))
    assert np.array_equal(full != 0, ref != 0)
    assert np.array_equal(_bits(full), _bits(ref.astype(np.float32)))


@pytest.mark.parametrize("name", list(CASES))
def test_dct_lifter_rows(tables, name):
    t = tables(name)
    c = t.cfg
    ld = c["nfilt"] | 1
    assert t.fbw_off - t.dctl_off == c["numcep"] * ld
    rows = t.f(t.dctl_off, c["numcep"] * ld).reshape(c["numcep"], ld)
    assert np.array_equal(_bits(rows[:, :c["nfilt"]]), _bits(_oracle_dctl(c).astype(np.float32)))
    assert not _bits(rows[:, c["nfilt"]:]).any()


def _w(j, m):
    j = np.asarray(j, dtype=np.float64)
    return np.stack([np.cos(2 * np.pi * j / m), -np.sin(2 * np.pi * j / m)], axis=-1).astype(np.float32)


@pytest.mark.parametrize("name", list(CASES))
def test_general_twiddles(tables, name):
    """Per pass h = 1, 4, 16, ...: h records {W_2h^j, W_4h^j, W_4h^(j+h)}; W_N^j, j < N/2, behind them exactly when log2(nfft)
    is odd.  cos / -sin in float64 rounded to float32: one ulp (two libms)."""
    t = tables(name)
    n = t.cfg["nfft"]
    ref = []
    for st in range(0, t.log2n - 1, 2):
        h = 1 << st
        j = np.arange(h)
        ref.append(np.stack([_w(j, 2 * h), _w(j, 4 * h), _w(j + h, 4 * h)], axis=1).reshape(-1))
    if t.log2n % 2:
        ref.append(_w(np.arange(n // 2), n).reshape(-1))
    ref = np.concatenate(ref)
    assert t.tw_off == 0 and t.dctl_off == ref.size
    assert ref.size == 2 * (sum(3 << st for st in range(0, t.log2n - 1, 2)) + (n // 2 if t.log2n % 2 else 0))
    assert _ulps(t.f(0, ref.size), ref).max() <= 1


@pytest.mark.parametrize("name", FAST)
def test_fft512_twiddles(tables, name):
    t = tables(name)
    k, l, c = np.arange(1, 8)[:, None], np.arange(64)[None, :], np.arange(8)[None, :]
    assert t.f_tw2 - t.f_tw1 == 7 * 64 * 2 and t.f_fb - t.f_tw2 == 7 * 8 * 2
    assert _ulps(t.f(t.f_tw1, 7 * 64 * 2), _w(l * k, 512).reshape(-1)).max() <= 1
    tw2 = t.f(t.f_tw2, 7 * 8 * 2)
    assert _ulps(tw2 * np.float32(64), _w(c * k, 64).reshape(-1)).max() <= 1      # (x 64: a power of two, exact)
    assert np.array_equal(_bits(tw2.reshape(7, 8, 2)[:, 0, 0]), _bits(np.full(7, 2.0 ** -6)))   # W^0 = 1 carries 2^-6 alone


def _fragment_index(tiles, groups):
    """lane l of product (tile t, group g), element j -> (row 16 t + (l & 15), column 16 g + 4 (l >> 4) + j)"""
    t, g, l, j = np.meshgrid(np.arange(tiles), np.arange(groups), np.arange(64), np.arange(4), indexing="ij")
    return 16 * t + (l & 15), 16 * g + 4 * (l >> 4) + j


@pytest.mark.parametrize("name", FAST)
def test_mfma_fragments_are_exact_permutations(tables, name):
    t = tables(name)
    c = t.cfg
    d = _dense2(t)
    assert t.f_dct - t.f_fb == 2 * 16 * 64 * 4
    r, col = _fragment_index(2, 16)
    assert np.array_equal(_bits(t.f(t.f_fb, r.size).reshape(r.shape)), _bits(d[r, col]))
    dct = np.zeros((32, 32), np.float32)
    dct[:c["numcep"], :c["nfilt"]] = t.f(t.dctl_off, c["numcep"] * (c["nfilt"] | 1)).reshape(c["numcep"], -1)[:, :c["nfilt"]]
    r, col = _fragment_index(2, 2)
    assert np.array_equal(_bits(t.f(t.f_dct, r.size).reshape(r.shape)), _bits(dct[r, col]))
    for s, (lo, n) in enumerate(((t.f_lo0, t.f_n0), (t.f_lo1, t.f_n1))):
        live = np.flatnonzero(d[16 * s:16 * s + 16].reshape(16, 16, 16).any(axis=(0, 2)))
        assert (lo, n) == ((int(live[0]), int(live[-1] - live[0] + 1)) if live.size else (0, 0))


class Band:
    """The banded tables of a plan decoded by the kernel's lane rule: wave w, lane l = 16 fq + 4 slot + t belongs to group
    4 w + slot and filter column t; its weight of instruction n = 4 q5 + c sits at [w][q5][l][c], its byte offset at [w][l]
    behind all the weights."""
    def __init__(self, t):
        self.w = np.zeros((16, 4, t.kBandN), np.float32)
        self.k_rd = np.zeros(16, int)
        wts = t.f(t.f_band, 4 * 5 * 64 * 4).reshape(4, 5, 64, 4)
        offs = t.i(t.f_band + 4 * 5 * 64 * 4, 4 * 64).reshape(4, 64)
        assert t.f_gat == t.f_band + 4 * 5 * 64 * 4 + 4 * 64
        for w in range(4):
            for l in range(64):
                fq, g, col = l >> 4, 4 * w + ((l >> 2) & 3), l & 3
                lane = wts[w, :, l, :].reshape(-1)
                if fq == 0:
                    self.w[g, col] = lane
                assert np.array_equal(_bits(lane), _bits(self.w[g, col]))        # the four frame quads read the same weights
                rowf = (fq * (2 * t.kEx + t.kExRow) + t.kExRow0 + (col & 1) * t.kPS if col >> 1
                        else 4 * t.kEx * 2 + (2 * fq + (col & 1)) * t.kPS)
                assert offs[w, l] % 4 == 0
                k = offs[w, l] // 4 - rowf
                if fq == 0 and col == 0:
                    self.k_rd[g] = k
                assert k == self.k_rd[g]
        # a group's first filter: the one window of four whose rows hold the group's weights
        d = _dense2(t)
        self.a = {}
        for g in range(16):
            if self.w[g].any():
                fits = [a for a in range(29) if all(
                    not self.w[g, col, n] or _bits(self.w[g, col, n]) == _bits(d[a + col, self.k_rd[g] + n])
                    for col in range(4) for n in range(t.kBandN))]
                assert len(fits) == 1, (g, fits)
                self.a[g] = fits[0]


@pytest.fixture(scope="session")
def band(tables):
    @functools.lru_cache(maxsize=None)
    def get(name):
        return Band(tables(name))
    return get


BANDED = ["reference", "telephone-band", "no-lifter"]


@pytest.mark.parametrize("name", BANDED)
def test_banded_filterbank_holds_every_weight_once(tables, band, name):
    t, b = tables(name), band(name)
    assert t.form == 2
    d = _dense2(t)
    count, recon = np.zeros((32, 256), int), np.zeros((32, 256), np.float32)
    spans = []
    for g in range(16):
        gi, ni = np.nonzero(b.w[g])
        assert not np.signbit(b.w[g][b.w[g] == 0]).any()                     # every other band weight is +0.0
        lo_k, hi_k = 0, 256 - t.kBandN
        if gi.size:
            k = b.k_rd[g] + ni
            np.add.at(count, (b.a[g] + gi, k), 1)
            recon[b.a[g] + gi, k] = b.w[g][gi, ni]
            assert 0 <= b.a[g] <= 28 and k.max() - k.min() + 1 <= t.kBandCap
            spans.append((int(k.min()), int(k.max())))
            lo_k, hi_k = max(0, int(k.max()) + 1 - t.kBandN), min(int(k.min()), hi_k)
        assert lo_k <= b.k_rd[g] <= hi_k                                    # the read covers the group and stays inside the row
    assert not b.w[15].any() and 15 not in b.a
    assert all(spans[i][1] < spans[i + 1][0] for i in range(len(spans) - 1))   # groups are consecutive runs of bins, in bin order
    assert np.array_equal(count, (d != 0).astype(int))
    assert np.array_equal(_bits(recon), _bits(d))
    if name == "reference":
        for w in range(4):                                                      # 64 lanes of a read on 64 different banks
            assert sorted(b.k_rd[4 * w:4 * w + 4] % 4) == [0, 1, 2, 3]


@pytest.mark.parametrize("name", BANDED)
def test_gather_table_names_the_partial_sums_of_each_filter(tables, band, name):
    t, b = tables(name), band(name)

    def part_byte(g, j):
        return ((g >> 2) * 2 * t.kEx + t.kExPart) * 4 + ((g & 3) * 4 + j) * 16

    gat = t.i(t.f_gat, t.kBandGat * 32).reshape(t.kBandGat, 32)
    assert t.f_gat + t.kBandGat * 32 == t.blob.size
    longest = 0
    for f in range(32):
        want = [part_byte(g, f - a) for g, a in sorted(b.a.items()) if 0 <= f - a <= 3 and b.w[g, f - a].any()]
        want += [part_byte(15, 0)] * (t.kBandGat - len(want))
        assert list(gat[:, f]) == want, f
        longest = max(longest, t.kBandGat - want.count(part_byte(15, 0)))
    assert t.f_gat_n == longest


def test_argument_errors(dump_exe):
    """tests/abi/arg_paths.c's cases for xvec_mfcc_create that reach the builder (the null pointers stop in front of it), and
    the other refusals of its checks: XVEC_ERR_ARG = 1, argument errors before any table."""
    for kw in (dict(nfft=500), dict(numcep=40), dict(nfft=32), dict(nfft=8192), dict(samplerate=0), dict(nfilt=0, numcep=0),
               dict(nfilt=300, numcep=13, nfft=1024), dict(nfft=64, nfilt=40), dict(numcep=0), dict(winlen=0.0), dict(winstep=0.00001)):
        t = Tables(dump_exe, kw, True)
        assert t.rc == 1 and t.msg, kw
    assert "power of two" in Tables(dump_exe, dict(nfft=500), True).msg
    assert "numcep <= nfilt" in Tables(dump_exe, dict(numcep=40), True).msg
