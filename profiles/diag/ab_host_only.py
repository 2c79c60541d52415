"""A/B of two builds for a HOST-ONLY change (needs no GPU): the gfx950 code of every translation unit must be identical,
and every *_workspace_bytes export must return the same numbers.

    python profiles/diag/ab_host_only.py OTHER_TREE      # OTHER_TREE: a checkout of the other commit, built with `make`

Compares <tree>/speaker-recognition-x-vectors_amd/csrc/*.o (the .hip_fatbin section -> clang-offload-bundler -> llvm-objdump -d of
the gfx950 code object) and the two libxvec_hip.so (ctypes, both loaded side by side).  Exit status 0 iff nothing differs."""
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = "speaker-recognition-x-vectors_amd"
LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def device_disassembly(obj, tmp):
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "code.co")
    if subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj],
                      capture_output=True).returncode:
        return None                        # a unit without kernels (xvec_api.o) carries no device code at all
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    assert "s_endpgm" in text, f"{obj}: no kernel code in the gfx950 code object"
    return text.split("\n", 2)[2]          # (the first two lines name the temporary file)


def workspace_table(lib_path):
    lib = C.CDLL(lib_path)
    i32, i64 = C.c_int32, C.c_int64
    calls = {
        "xvec_score_workspace_bytes": ([i64, i64, i32], [(10, 0, 8), (4874, 0, 512), (4874, 1000, 512), (1, 1, 1), (7, 3, 150),
                                                         (100000, 0, 512), (0, 0, 8), (5, 5, 0)]),
        "xvec_plda_stats_workspace_bytes": ([i64, i32, i32], [(400000, 512, 1211), (2, 1, 1), (1000, 24, 10), (50000, 150, 997),
                                                              (2**31 - 1, 512, 7000), (1, 8, 1), (10, 8, 11)]),
        "xvec_plda_em_workspace_bytes": ([i32, i32], [(10, 4), (1211, 150), (1, 1), (7000, 512), (33, 31), (0, 4)]),
        "xvec_eval_workspace_bytes": ([i64], [(1000,), (2**31 - 1,), (1,), (2048,), (2049,), (37720,), (4874 * 4874,), (0,),
                                              (2**31,)]),
        "xvec_calib_workspace_bytes": ([i64], [(1,), (1000,), (37720,), (4874 * 4874,), (2**31 - 1,), (0,), (2**31,)]),
        "xvec_report_det_workspace_bytes": ([i64], [(1,), (1000,), (37720,), (4874 * 4874,), (2**31 - 1,), (0,), (2**31,)]),
        # rec_start: a tuple of the recordings' counts (passed as their running sum from 0), or None for a null pointer
        "xvec_ahc_workspace_bytes": ([rec, i32], [((1,), 1), ((3, 4, 5), 3), ((64, 65, 1), 3), ((2048,), 1), ((2048,) * 64, 64),
                                                  ((2049,), 1), ((3, 0, 2), 3), ((), 0), (None, 1)]),
        "xvec_vbx_workspace_bytes": ([rec, i32, i32, i32], [((1,), 1, 1, 1), ((40, 50), 2, 128, 8), ((16384,), 1, 512, 64),
                                                           ((16384,) * 16, 16, 512, 64), ((16385,), 1, 128, 8),
                                                           ((40, 0), 2, 128, 8), ((40,), 1, 513, 8), ((40,), 1, 128, 65),
                                                           ((40,), 1, 128, 0), ((), 0, 128, 8), (None, 1, 128, 8)]),
        "xvec_der_workspace_bytes": ([rec, i32, i64, i64], [((1,), 1, 0, 0), ((100, 4097), 2, 3, 4), ((2**31 - 1,), 1, 5, 5),
                                                           ((2**30, 2**30 - 1), 2, 2**31 - 1, 2**31 - 1), ((2**30, 2**30), 2, 1, 1),
                                                           ((5, 0), 2, 1, 1), ((5,), 1, -1, 1), ((5,), 1, 1, 2**31), ((), 0, 1, 1),
                                                           (None, 1, 1, 1)]),
    }
    out = {}
    for name, (argtypes, rows) in calls.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_size_t, [C.POINTER(i64) if t is rec else t for t in argtypes]
        for row in rows:
            out[(name,) + row] = fn(*(rec(a) if t is rec else a for t, a in zip(argtypes, row)))
    return out


def show(arg):
    """An argument of a row as the table prints it: a long run of one count as `(n,) * k`."""
    if isinstance(arg, tuple) and len(arg) > 4 and len(set(arg)) == 1:
        return f"({arg[0]},) * {len(arg)}"
    return repr(arg)


def rec(counts):
    """rec_start of the recordings' `counts`, as the library reads it on the host."""
    if counts is None:
        return None
    starts = [0]
    for n in counts:
        starts.append(starts[-1] + n)
    return (C.c_int64 * len(starts))(*starts)


def main():
    other = os.path.abspath(sys.argv[1])
    bad = 0
    mine = sorted(glob.glob(os.path.join(HERE, PKG, "csrc", "*.o")))
    with tempfile.TemporaryDirectory() as tmp:
        for obj in mine:
            unit = os.path.basename(obj)
            a_text, b_text = device_disassembly(obj, tmp), device_disassembly(os.path.join(other, PKG, "csrc", unit), tmp)
            same = a_text == b_text
            bad += not same
            print(f"device code {unit:20s} {'DIFFERS' if not same else 'identical' if a_text else 'none in either'}")
    a, b = (workspace_table(os.path.join(t, PKG, "libxvec_hip.so")) for t in (HERE, other))
    for key in a:
        same = a[key] == b[key]
        bad += not same
        print(f"{key[0]}({', '.join(map(show, key[1:]))}) = {a[key]}" + ("" if same else f"  DIFFERS: the other tree returns {b[key]}"))
    print(f"{len(mine)} translation units, {len(a)} workspace sizes: " + ("all equal" if not bad else f"{bad} differ"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
