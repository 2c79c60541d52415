"""A/B of the trial family's shared headers (csrc/trial_plan.h, csrc/trial_device.h: eval.hip, calib.hip, report.hip; snorm.hip for
its block sum) against a tree from before them.

    python profiles/diag/trial_units_ab.py lines OTHER_TREE        # no GPU
    python profiles/diag/trial_units_ab.py kernels OTHER_TREE      # no GPU: both trees built with `make`
    python profiles/diag/trial_units_ab.py dump OUT.npz            # on a GPU, once in each tree, each its own process
    python profiles/diag/trial_units_ab.py compare A.npz B.npz     # no GPU

lines    the line counts of the touched files in both trees, and in which files of this tree's csrc/ each shared name is
         defined (a using-declaration is not a definition).  Exit status 0 iff the total went down and every name has one home.
kernels  per kernel of the four units: what hipcc reports for it in each tree (VGPRs, LDS, scratch, waves per SIMD) and whether
         its gfx950 instructions are the other tree's (as class_scatter_ab.py compares them).  Exit status 0 iff LDS, scratch and
         occupancy agree everywhere.
dump     every output of the four units at the shapes of profiles/trial_units_ab.txt, seeded, into one .npz.
compare  the names, shapes, types and bytes of every array of two dumps.  Exit status 0 iff all agree."""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from class_scatter_ab import PKG, _edit_distance, _makefile_flags       # noqa: E402

UNITS = ("eval", "calib", "report", "snorm")
FILES = ("eval.hip", "calib.hip", "report.hip", "snorm.hip", "calib_plan.h", "report_plan.h", "trial_plan.h", "trial_device.h")
NAMES = ("block_excl_scan", "block_count", "block_extreme", "key_score", "score_key", "read_trial", "kBitVoid", "count_ok",
         "check_trials", "check_all_pairs")


# ---------------------------------------------------------------- lines

def _line_count(tree, name):
    path = os.path.join(tree, PKG, "csrc", name)
    if not os.path.exists(path):
        return 0
    with open(path) as f:
        return sum(1 for _ in f)


def lines(other):
    count = _line_count
    print(f"  {'':20s} {'parent':>7s} {'new':>6s}")
    totals = [0, 0]
    for f in FILES:
        a, b = count(other, f), count(HERE, f)
        totals[0] += a
        totals[1] += b
        print(f"  {f:20s} {a or '-':>7} {b or '-':>6}")
    print(f"  {'together':20s} {totals[0]:>7} {totals[1]:>6}     ({totals[1] - totals[0]:+d})")
    bad = totals[1] >= totals[0]
    csrc = os.path.join(HERE, PKG, "csrc")
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    for name in NAMES + ("block_sum",):
        # a definition: the name after a type, in front of its parameters or its value, on a line that is no comment
        pat = re.compile(rf"^(?!\s*//)[^\n;]*\b(?:inline|__device__|constexpr)\b[^\n;(]*[\w>&*] {name}\s*(?:\(|=)", re.M)
        homes = [f for f, text in sources.items() if pat.search(text)]
        print(f"  {name:16s} defined in {', '.join(homes)}")
        bad |= homes != (["trial_device.h", "tsne.hip"] if name == "block_sum" else homes[:1]) or not homes
    return 1 if bad else 0


# ---------------------------------------------------------------- kernels

def _short(mangled):
    text = subprocess.run(["c++filt", mangled], capture_output=True, text=True, check=True).stdout
    m = re.match(r"(?:void )?xvec::\(anonymous namespace\)::(.*?)\((?:[^()]|\([^()]*\))*\)\s*$", text.strip())
    return m.group(1) if m else None


def _resources(tree, unit):
    out = subprocess.run(["/opt/rocm/bin/hipcc", *_makefile_flags(tree), "-Rpass-analysis=kernel-resource-usage", "-c",
                          unit + ".hip", "-o", os.devnull], cwd=os.path.join(tree, PKG, "csrc"), capture_output=True, text=True,
                         check=True).stderr
    pats = (("vgprs", r" VGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
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
    from ab_host_only import device_disassembly
    text = device_disassembly(os.path.join(tree, PKG, "csrc", unit + ".o"), tmp)
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = _short(m.group(1)) if m.group(1).startswith("_ZN4xvec12_GLOBAL__N_1") else None
            cur = kernels.setdefault(name, []) if name else None
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    return kernels


def kernels(other):
    bad = 0
    print(f"{'kernel':44s} {'VGPR':>9s} {'LDS':>13s} {'scratch':>7s} {'waves/SIMD':>10s}  instructions (parent -> new)")
    with tempfile.TemporaryDirectory() as tmp:
        for unit in UNITS:
            new_r, old_r = _resources(HERE, unit), _resources(other, unit)
            new_i, old_i = _instructions(HERE, unit, tmp), _instructions(other, unit, tmp)
            print(f"-- {unit}.hip: {len(old_r)} kernels in the parent, {len(new_r)} in the new tree")
            bad += sorted(old_r) != sorted(new_r)
            for name in sorted(new_r):
                a, b = old_r[name], new_r[name]
                bad += any(a[k] != b[k] for k in ("lds", "scratch", "occupancy"))
                ia, ib = old_i[name], new_i[name]
                if ia == ib:
                    verdict = f"identical ({len(ib)})"
                else:
                    verdict = f"DIFFER: {len(ia)} -> {len(ib)} instructions; registers renamed: {_edit_distance(ia, ib)}"
                pair = lambda k: f"{a[k]}/{b[k]}"
                print(f"{name:44s} {pair('vgprs'):>9s} {pair('lds'):>13s} {pair('scratch'):>7s} {pair('occupancy'):>10s}  {verdict}")
    print("kernel names, LDS, scratch and occupancy: " + ("unchanged everywhere" if not bad else f"{bad} differ"))
    return 1 if bad else 0


# ---------------------------------------------------------------- dump

def planted_matrix(n_rows, n_cols, seed, finite=False):
    """tests/test_trial_units_gpu.py's: three NaN, +inf, -inf, -0.0 / +0.0, six equal scores (finite: 9.5 and -9.5 for the two
    infinities, so that a fit converges)."""
    import numpy as np
    s = np.random.default_rng(seed).normal(0.0, 3.0, (n_rows, n_cols))
    cells = {(3, 3): np.nan, (13, n_cols - 1): np.nan, (n_rows - 1, 7): np.nan, (5, 6): 9.5 if finite else np.inf,
             (40, 33): -9.5 if finite else -np.inf, (1, 2): -0.0, (2, 1): 0.0}
    cells.update({(10, j): 0.25 for j in range(6)})
    for (i, j), v in cells.items():
        s[i, j] = v
    return s, list(cells)


def dump(path):
    import dataclasses
    import numpy as np
    import torch
    from xvector_amd import calibrate as cal, evaluate as ev, hip, report as rp, snorm
    dev = "cuda:0"
    out = {}
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    def record(key, r):                        # a result dataclass / named tuple / DetCurve: every field an array
        fields = r._asdict() if hasattr(r, "_asdict") else {f.name: getattr(r, f.name) for f in dataclasses.fields(r)}
        for name, v in fields.items():
            out[f"{key}/{name}"] = host(v)

    def eval_bytes(key, call, n, *args):
        ws = torch.empty(int(hip.lib.xvec_eval_workspace_bytes(n)), dtype=torch.uint8, device=dev)
        rec = torch.zeros(len(ev._Result._fields_), dtype=torch.float64, device=dev)
        assert call(*args, 1.0, 1.0, 0.01, rec.data_ptr(), ws.data_ptr(), ws.numel(), stream()) == 0, hip.lib.xvec_eval_last_error()
        out[f"{key}/eval_result"] = host(rec)

    def trial_list(n, n_rows, n_cols, cells, seed):
        rng = np.random.default_rng(seed)
        rows, cols = rng.integers(0, n_rows, n), rng.integers(0, n_cols, n)
        if n > 200:                            # (shorter lists: seeded cells alone)
            for k, (i, j) in enumerate(cells):
                rows[3 * k], cols[3 * k] = i, j
            rows[100], cols[200] = -1, n_cols
        return ev.TrialList(rows, cols, rng.integers(0, 2, n))

    def list_case(key, s, s_fit, trials):
        n = len(trials)
        s_d, f_d = torch.from_numpy(s).to(dev), torch.from_numpy(s_fit).to(dev)
        r_d, c_d, t_d = trials.on(dev)
        shape = (s_d.data_ptr(), s_d.stride(0), s.shape[0], s.shape[1], r_d.data_ptr(), c_d.data_ptr(), t_d.data_ptr(), n)
        eval_bytes(key, hip.lib.xvec_eval_trials, n, *shape)
        keys = torch.zeros(n, dtype=torch.int32, device=dev)
        bits = torch.zeros(n, dtype=torch.uint8, device=dev)
        ws = torch.empty(int(hip.lib.xvec_eval_workspace_bytes(n)), dtype=torch.uint8, device=dev)
        assert hip.lib.xvec_eval_sorted_keys(*shape, keys.data_ptr(), bits.data_ptr(), ws.data_ptr(), ws.numel(), stream()) == 0
        out[f"{key}/sorted_keys"], out[f"{key}/sorted_bits"] = host(keys), host(bits)
        out[f"{key}/fit_inf"] = host(cal.fit_calibration(s_d, trials).record)
        c = cal.fit_calibration(f_d, trials)
        out[f"{key}/fit"] = host(c.record)
        out[f"{key}/apply"] = host(c.apply(f_d))
        record(f"{key}/cllr", cal.cllr(s_d, trials, c_miss=1.0, c_fa=2.0, p_target=0.3))
        record(f"{key}/cllr_finite", cal.cllr(f_d, trials, c_miss=1.0, c_fa=2.0, p_target=0.3))
        record(f"{key}/pav", cal.pav_segments(s_d, trials))
        for grid in (0, 50):
            record(f"{key}/det_grid{grid}", rp.det_curve(s_d, trials, grid=grid))

    def pairs_case(key, s, s_fit, rl, cl, skip):
        n_rows, n_cols = s.shape
        s_d, f_d = torch.from_numpy(s).to(dev), torch.from_numpy(s_fit).to(dev)
        r_d, c_d = torch.from_numpy(rl).to(dev), torch.from_numpy(cl).to(dev)
        eval_bytes(key, hip.lib.xvec_eval_all_pairs, n_rows * n_cols, s_d.data_ptr(), s_d.stride(0), n_rows, n_cols, r_d.data_ptr(),
                   c_d.data_ptr(), int(skip))
        out[f"{key}/fit_inf"] = host(cal.fit_calibration_all_pairs(s_d, rl, cl, skip_diagonal=skip).record)
        out[f"{key}/fit"] = host(cal.fit_calibration_all_pairs(f_d, rl, cl, skip_diagonal=skip).record)
        record(f"{key}/cllr", cal.cllr_all_pairs(s_d, rl, cl, skip_diagonal=skip, c_miss=1.0, c_fa=2.0, p_target=0.3))
        record(f"{key}/cllr_finite", cal.cllr_all_pairs(f_d, rl, cl, skip_diagonal=skip, c_miss=1.0, c_fa=2.0, p_target=0.3))
        for grid in (0, 50):
            record(f"{key}/det_grid{grid}", rp.det_curve_all_pairs(s_d, rl, cl, skip_diagonal=skip, grid=grid))

    s, cells = planted_matrix(67, 61, 20)
    s_fit, _ = planted_matrix(67, 61, 20, finite=True)
    for n in (1, 255, 256, 257, 4095, 4096, 4097, 65537):
        list_case(f"list_n{n}", s, s_fit, trial_list(n, 67, 61, cells, 1000 + n))
    for n_rows, n_cols in ((65, 65), (130, 67)):
        s, cells = planted_matrix(n_rows, n_cols, 22)
        s_fit, _ = planted_matrix(n_rows, n_cols, 22, finite=True)
        rl, cl = (np.arange(n_rows) % 7).astype(np.int32), (np.arange(n_cols) % 7).astype(np.int32)
        for skip in (False, True):
            pairs_case(f"pairs_{n_rows}x{n_cols}_skip{int(skip)}", s, s_fit, rl, cl, skip)
    # the report's range and images on the 130 x 67 matrix (s, cells are its)
    s_d = torch.from_numpy(s).to(dev)
    out["report_130x67/range"] = np.asarray(rp.score_range(s_d), dtype=np.float64)
    trials = trial_list(4097, 130, 67, cells, 77)
    for dtype, tag in ((torch.uint8, "u8"), (torch.float32, "f32")):
        for name, img in rp.score_images(s_d, trials, 0.5, -0.3, dtype=dtype).items():
            out[f"report_130x67/{tag}/{name}"] = host(img.contiguous())
    # snorm: a resident-small, a resident-large and a streamed row length on each side of 4096 and 16 384
    for C in (4096, 4097, 16384, 16385):
        rng = np.random.default_rng(C)
        x = rng.normal(-20.0, 8.0, (5, C))
        x[1, ::7] = np.nan
        x[2, 5:40] = x[2, 4]
        x_d = torch.from_numpy(x).to(dev)
        for top_k in (0, 300):
            st = snorm.cohort_stats(x_d, top_k=top_k, skip_col=torch.tensor([-1, 0, 3, C - 1, 17]))
            record(f"snorm_C{C}_k{top_k}", st)
            out[f"snorm_C{C}_k{top_k}/normalised"] = host(snorm.apply_norm(x_d[:, :64], row_stats=st))
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"build {hip.version().split()[-1]}: {len(out)} arrays, {sum(a.size for a in out.values())} elements -> {path}")
    return 0


def compare(a_path, b_path):
    import numpy as np
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for name in sorted(set(a.files) & set(b.files)):
        if not (a[name].shape == b[name].shape and a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes()):
            bad.append(name)
    print(f"{len(a.files)} arrays against {len(b.files)}: " + ("every bit equal" if not bad else "DIFFER: " + ", ".join(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    mode, args = sys.argv[1], sys.argv[2:]
    sys.exit({"lines": lines, "kernels": kernels, "dump": dump, "compare": compare}[mode](*(os.path.abspath(p) for p in args)))
