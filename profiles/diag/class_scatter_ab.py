"""A/B of the shared class-statistics / scatter kernels (csrc/class_scatter.h) against a tree from before them.

    python profiles/diag/class_scatter_ab.py kernels OTHER_TREE     # no GPU: both trees built with `make`
    python profiles/diag/class_scatter_ab.py dump OUT.npz           # on a GPU, once in each tree, each its own process
    python profiles/diag/class_scatter_ab.py compare A.npz B.npz    # no GPU

kernels  per kernel of plda_train.hip and lda.hip: what hipcc reports for it in each tree (VGPRs, AGPRs, LDS, scratch, waves
         per SIMD) and whether its gfx950 instructions are the other tree's (ab_host_only.device_disassembly of the two .o,
         cut at the kernel symbols, addresses and encodings dropped; the kernels paired by RENAMED).  Where they are not:
         how many instructions stand on one side only once register numbers and branch distances are wiped out.  Exit status
         0 iff LDS, scratch and occupancy agree everywhere.
dump     every output of xvec_plda_stats (mean, counts, class_sums, class_sums_t, sigma_obs) and of xvec_lda_stats (mean,
         class_means, s_within, s_between) at the shapes of tests/test_plda_edges_gpu.py and tests/test_lda_gpu.py, seeded as
         there, into one .npz.
compare  np.array_equal on every array of two dumps.  Exit status 0 iff the names and all bits agree."""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PKG = "speaker-recognition-x-vectors_amd"
UNITS = ("plda_train", "lda")
# kernel of the tree with class_scatter.h -> its name in a tree from before (template arguments: the first two)
RENAMED = {("plda_train", "stats_mean_kernel"): "plda_mean_kernel", ("lda", "stats_mean_kernel"): "lda_mean_kernel",
           ("plda_train", "class_scatter_kernel"): "plda_scatter_kernel", ("lda", "class_scatter_kernel"): "lda_scatter_kernel",
           ("plda_train", "class_scatter_reduce_kernel"): "plda_scatter_reduce_kernel",
           ("lda", "class_scatter_reduce_kernel"): "lda_scatter_reduce_kernel"}


# ---------------------------------------------------------------- kernels

def _makefile_flags(tree):
    text = open(os.path.join(tree, PKG, "csrc", "Makefile")).read()
    flags = re.search(r"^CXXFLAGS = (.*?) \$\(if", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    return [f for f in flags if f != "-fPIC"] + ["--cuda-device-only"]


def _short(mangled):
    """'plda_class_sum_kernel<float>' from the mangled name of a kernel in xvec's anonymous namespace (template arguments of
    these files: float, double, bool)."""
    m = re.match(r"_ZN4xvec12_GLOBAL__N_1(\d+)", mangled)
    start = m.end()
    name, rest = mangled[start:start + int(m.group(1))], mangled[start + int(m.group(1)):]
    if not rest.startswith("I"):
        return name
    toks = re.match(r"I((?:f|d|Lb[01]E)+)E", rest).group(1)
    words = {"f": "float", "d": "double", "Lb0E": "false", "Lb1E": "true"}
    return name + "<" + ", ".join(words[t] for t in re.findall(r"f|d|Lb[01]E", toks)) + ">"


def _resources(tree, unit):
    out = subprocess.run(["/opt/rocm/bin/hipcc", *_makefile_flags(tree), "-Rpass-analysis=kernel-resource-usage", "-c",
                          unit + ".hip", "-o", os.devnull], cwd=os.path.join(tree, PKG, "csrc"), capture_output=True, text=True,
                         check=True).stderr
    pats = (("vgprs", r" VGPRs: (\d+)"), ("agprs", r" AGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
            ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"))
    res, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = _short(m.group(1))
            res[name] = {}
        for key, pat in pats:
            m = re.search(pat, line)
            if m and name:
                res[name][key] = int(m.group(1))
    return res


def _instructions(tree, unit, tmp):
    """{kernel: [instruction text, ...]} of <tree>'s built <unit>.o"""
    from ab_host_only import device_disassembly
    text = device_disassembly(os.path.join(tree, PKG, "csrc", unit + ".o"), tmp)
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = kernels.setdefault(_short(m.group(1)), []) if m.group(1).startswith("_ZN4xvec12_GLOBAL__N_1") else None
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    return kernels


def _edit_distance(ia, ib):
    """'-a +b': instructions only in the first / only in the second list once register numbers and branch distances are
    wiped out (difflib's longest matching blocks: an upper bound of the true edit distance)."""
    import difflib

    def wipe(line):
        line = re.sub(r"\b([vsa])\[\d+:\d+\]", r"\1[#]", line)
        line = re.sub(r"\b([vsa])\d+\b", r"\1#", line)
        return re.sub(r"^(s_c?branch\S*) \d+$", r"\1 #", line)
    a, b = [wipe(x) for x in ia], [wipe(x) for x in ib]
    same = sum(m.size for m in difflib.SequenceMatcher(None, a, b, autojunk=False).get_matching_blocks())
    return f"-{len(a) - same} +{len(b) - same}"


def _parent_name(unit, name):
    base, _, targs = name.partition("<")
    old = RENAMED.get((unit, base))
    if old is None:
        return name
    if not targs:
        return old
    return old + "<" + ", ".join(targs.rstrip(">").split(", ")[:2]) + ">"


def kernels(other):
    bad = 0
    print(f"{'kernel (new tree)':58s} {'VGPR':>9s} {'AGPR':>7s} {'LDS':>13s} {'scratch':>7s} {'waves/SIMD':>10s}  instructions (parent -> new)")
    with tempfile.TemporaryDirectory() as tmp:
        for unit in UNITS:
            new_r, old_r = _resources(HERE, unit), _resources(other, unit)
            new_i, old_i = _instructions(HERE, unit, tmp), _instructions(other, unit, tmp)
            print(f"-- {unit}.hip: {len(old_r)} kernels in the parent, {len(new_r)} in the new tree")
            for name in sorted(new_r):
                old = _parent_name(unit, name)
                a, b = old_r[old], new_r[name]
                bad += any(a[k] != b[k] for k in ("lds", "scratch", "occupancy"))
                ia, ib = old_i[old], new_i[name]
                if ia == ib:
                    verdict = f"identical ({len(ib)})"
                else:
                    verdict = f"DIFFER: {len(ia)} -> {len(ib)} instructions; registers renamed: {_edit_distance(ia, ib)}"
                pair = lambda k: f"{a[k]}/{b[k]}"
                print(f"{name + ('' if old == name else '  [' + old + ']'):58s} {pair('vgprs'):>9s} {pair('agprs'):>7s} {pair('lds'):>13s} "
                      f"{pair('scratch'):>7s} {pair('occupancy'):>10s}  {verdict}")
    print("LDS, scratch and occupancy: " + ("unchanged everywhere" if not bad else f"{bad} kernels differ"))
    return 1 if bad else 0


# ---------------------------------------------------------------- dump / compare

def dump(path):
    import numpy as np
    import torch
    from xvector_amd import hip, lda, plda
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import lda_ref
    dev = "cuda:0"
    out = {}

    def on_device(x, dtype, misaligned=False):
        t = torch.from_numpy(x.astype(np.float32) if dtype == "f32" else x).to(dev)
        if misaligned:                          # one element into a buffer: dim % 4 == 0 stages element by element
            buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=dev)
            u = buf[1:1 + t.numel()].view(*t.shape)
            u.copy_(t)
            assert u.data_ptr() % 16 != 0
            return u
        return t

    def plda_data(n, dim, n_classes, seed):     # tests/test_plda_edges_gpu.py::_data
        rng = np.random.default_rng(seed)
        labels = np.concatenate([np.arange(n_classes), rng.integers(0, n_classes, n - n_classes)])
        rng.shuffle(labels)
        return 3.0 + rng.normal(0, 1, (n_classes, dim))[labels] + rng.normal(0, 1, (n, dim)), labels

    cases = [(2, 1, 1, 4, "f64", 1.0, False), (2, 1, 2, 5, "f64", 1.0, False)]
    cases += [(300, d, 20, d, t, 0.5 if d == 65 else 1.0, False) for d in (63, 64, 65, 129) for t in ("f32", "f64")]
    cases += [(n, 65, 9, n, "f64", 1.0, False) for n in (257, 513)]
    cases += [(7169, 512, 40, 7, "f32", 1.0, False), (500, 64, 30, 11, "f32", 1.0, True), (500, 64, 30, 11, "f64", 1.0, True)]
    for n, dim, C, seed, dtype, sf, mis in cases:
        x, labels = plda_data(n, dim, C, seed)
        st = plda.PldaStats(on_device(x, dtype, mis), labels, scaling_factor=sf)
        key = f"plda_n{n}_d{dim}_c{C}_{dtype}" + ("_misaligned" if mis else "")
        for name, a in (("mean", st.mean), ("counts", st.counts), ("class_sums", st.class_sums()),
                        ("class_sums_t", st._cls_t.cpu().numpy()), ("sigma_obs", st.sigma_obs)):
            out[f"{key}/{name}"] = a

    def lda_labels(n, n_classes, rng):          # tests/test_lda_gpu.py::_labels_unequal
        lab = np.arange(n_classes)
        if n > n_classes:
            rest = n - n_classes
            big = (rest * 3) // 5 if n_classes > 1 else rest
            others = rng.integers(min(1, n_classes - 1), n_classes, rest - big)
            lab = np.concatenate([lab, np.full(big, min(1, n_classes - 1)), others])
        rng.shuffle(lab)
        return lab

    def lda_case(key, x, labels, dtype, mis=False):
        st = lda.LdaStats(on_device(x, dtype, mis), labels)
        for name in ("mean", "class_means", "s_within", "s_between"):
            out[f"{key}/{name}"] = getattr(st, name)

    for n, dim, C, dtype in [(2, 1, 1, "f64"), (15, 3, 4, "f32"), (16, 63, 5, "f64"), (17, 64, 5, "f32"), (65, 65, 6, "f64"),
                             (65, 130, 3, "f32"), (200, 64, 7, "f64"), (200, 130, 9, "f32")]:       # STATS_SHAPES
        rng = np.random.default_rng(n * 1000 + dim)
        labels = lda_labels(n, C, rng)
        x = 3.0 + rng.normal(0, 1, (C, dim))[labels] + rng.normal(0, 0.5, (n, dim))
        lda_case(f"lda_n{n}_d{dim}_c{C}_{dtype}", x, labels, dtype)
    rng = np.random.default_rng(7)              # test_stats_row_slices_without_rows
    labels = lda_labels(897, 40, rng)
    lda_case("lda_n897_d512_c40_f32", rng.normal(0, 1, (40, 512))[labels] + rng.normal(0, 0.5, (897, 512)), labels, "f32")
    for dtype in ("f32", "f64"):                # test_stats_from_a_misaligned_base
        rng = np.random.default_rng(11)
        labels = lda_labels(200, 7, rng)
        x = rng.normal(0, 1, (7, 64))[labels] + rng.normal(0, 0.5, (200, 64))
        lda_case(f"lda_n200_d64_c7_{dtype}_misaligned", x, labels, dtype, True)
    x, labels = lda_ref.make_case(200, 24, 7, offset=1e6)
    lda_case("lda_n200_d24_c7_f64_offset1e6", x, labels, "f64")
    np.savez(path, **out)
    print(f"build {hip.version().split()[-1]}: {len(out)} arrays, {sum(a.size for a in out.values())} elements -> {path}")
    return 0


def compare(a_path, b_path):
    import numpy as np
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for name in sorted(set(a.files) & set(b.files)):
        if not (a[name].shape == b[name].shape and a[name].dtype == b[name].dtype and
                np.array_equal(a[name].view(np.uint64), b[name].view(np.uint64))):       # the bits: -0.0 and NaN count
            bad.append(name)
    print(f"{len(a.files)} arrays against {len(b.files)}: " + ("every bit equal" if not bad else "DIFFER: " + ", ".join(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    mode, args = sys.argv[1], sys.argv[2:]
    sys.exit({"kernels": kernels, "dump": dump, "compare": compare}[mode](*(os.path.abspath(p) for p in args)))
