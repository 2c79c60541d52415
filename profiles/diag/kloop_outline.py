#!/usr/bin/env python3
"""Outline of a kernel's K loop from its gfx950 assembly: the order of buffer_load / ds_read / ds_write / s_waitcnt / s_barrier /
MFMA instructions, runs of the same kind folded to `kind xN`.  What profiles/wino_s3_pipeline.txt records.

    hipcc <the Makefile's flags> --cuda-device-only -S csrc/tdnn_wino_s3.hip -o - | profiles/diag/kloop_outline.py tdnn_wino_s3_kernel

Prints every basic block of the named kernel (substring of the mangled symbol) that holds at least `min_mfma` MFMAs (default
12), with its label and the branch that ends it."""
import re
import sys

KINDS = (("mfma", r"v_mfma_"), ("buffer_load", r"buffer_load_"), ("buffer_store", r"buffer_store_"), ("ds_read", r"ds_read"),
         ("ds_write", r"ds_write"), ("s_barrier", r"s_barrier"), ("v_mov64", r"v_mov_b64|v_pk_mov_b32"),
         ("branch", r"s_cbranch|s_branch"))


def blocks(asm, kernel):
    """[(label, [instruction lines])] of the kernel whose symbol contains `kernel`."""
    out, cur, inside = [], None, False
    for line in asm.splitlines():
        s = line.strip()
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
        if m:
            lab = m.group(1)
            if not lab.startswith(".L"):
                inside = kernel in lab
            if inside:
                cur = (lab, [])
                out.append(cur)
            continue
        if inside and cur is not None and s and not s.startswith((".", ";")):
            cur[1].append(s.split(";")[0].strip())
            if s.startswith("s_endpgm"):
                inside = False
    return out


def kind_of(ins):
    if ins.startswith("s_waitcnt"):
        return ins            # kept verbatim: the counts are the point
    for k, pat in KINDS:
        if re.match(pat, ins):
            return k
    return None


def outline(instrs):
    runs = []
    for ins in instrs:
        k = kind_of(ins)
        if k is None:
            continue
        if runs and runs[-1][0] == k and not k.startswith("s_waitcnt"):
            runs[-1][1] += 1
        else:
            runs.append([k, 1])
    return [k if n == 1 else f"{k} x{n}" for k, n in runs]


def main():
    kernel = sys.argv[1]
    min_mfma = int(sys.argv[2]) if len(sys.argv) > 2 else 12
    asm = sys.stdin.read()
    for lab, ins in blocks(asm, kernel):
        if sum(1 for i in ins if i.startswith("v_mfma_")) < min_mfma:
            continue
        print(f"{lab}:  ({len(ins)} instructions)")
        line = "   "
        for item in outline(ins):
            if len(line) + len(item) > 118:
                print(line)
                line = "   "
            line += " " + item + " |"
        print(line)
        print()


if __name__ == "__main__":
    main()
