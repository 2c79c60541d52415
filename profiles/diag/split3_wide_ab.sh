#!/bin/bash
# A/B of the bf16_split3 pooling kernel on 384-channel tiles (csrc/tdnn_split3w.hip) against the parent commit's library, and
# the crossover sweep of its threshold.  Figures: profiles/split3_wide_ab.txt, profiles/split3_wide_crossover.txt.
#   bash profiles/diag/split3_wide_ab.sh ab <parent.so>      A: five interleaved triples parent / new / new at XVEC_SPLIT3_WIDE=0,
#                                                            B: three --full triples (per-kernel event times), C: --dump-outputs
#   bash profiles/diag/split3_wide_ab.sh sweep               wide tile at every size against XVEC_SPLIT3_WIDE=0, by batch size
#   bash profiles/diag/split3_wide_ab.sh trace <parent.so> <dir>   D: rocprofv3 --kernel-trace --stats, a run of its own per build
#   bash profiles/diag/split3_wide_ab.sh pmc <parent.so> <dir>     E: rocprofv3 --pmc, a run of its own per build, no tracing
# <parent.so>: the library built from a checkout of the parent commit (absolute path; loaded through XVEC_LIB, the binding is
# unchanged).  Every GPU step runs under a time limit of its own; the first failure ends the script.
set -e -o pipefail
root=$(cd "$(dirname "$0")/../.." && pwd)
cd $root
line='
import sys, json
d = json.loads(sys.stdin.readline())
k = d.get("roofline", {}).get("per_kernel_ms", {})
print(sys.argv[1], d["value"], d["ms_per_step"], " ".join(f"{n}={v:.4f}" for n, v in k.items()), flush=True)'
run() {   # run <label> <lib or ""> <wide: 1|0> <bench args...>
  local label=$1 lib=$2 wide=$3; shift 3
  XVEC_LIB=$lib XVEC_SPLIT3_WIDE=$wide timeout -k 10 240 python bench.py "$@" 2>/dev/null | python -c "$line" "$label"
}
case "$1" in
ab)
  P=$(realpath $2)
  echo "== A: bench.py --steps 200 --warmup 20"
  for i in 1 2 3 4 5; do
    run "parent" $P 1 --steps 200 --warmup 20
    run "new   " "" 1 --steps 200 --warmup 20
    run "new@w0" "" 0 --steps 200 --warmup 20
  done
  echo "== B: --full --steps 50 --warmup 10 --cpu-budget 0 --no-secondary"
  for i in 1 2 3; do
    run "parent" $P 1 --full --steps 50 --warmup 10 --cpu-budget 0 --no-secondary
    run "new   " "" 1 --full --steps 50 --warmup 10 --cpu-budget 0 --no-secondary
    run "new@w0" "" 0 --full --steps 50 --warmup 10 --cpu-budget 0 --no-secondary
  done
  echo "== C: outputs"
  out=$(mktemp -d)
  XVEC_LIB=$P timeout -k 10 240 python bench.py --steps 20 --warmup 5 --dump-outputs $out/parent > /dev/null 2>&1
  timeout -k 10 240 python bench.py --steps 20 --warmup 5 --dump-outputs $out/new > /dev/null 2>&1
  python -c "
import numpy as np
a, b = np.load('$out/parent/embeddings.npy'), np.load('$out/new/embeddings.npy')
print('embeddings', a.shape, 'finite', bool(np.isfinite(b).all()), 'array_equal', bool(np.array_equal(a, b)))"
  ;;
sweep)
  for B in ${BATCHES:-32 48 64 86 100 115 128 160 192 256}; do
    for w in 0 1; do
      XVEC_SPLIT3_MIN_ROWS=0 XVEC_SPLIT3_WIDE_MIN_ROWS=0 XVEC_SPLIT3_WIDE=$w timeout -k 10 240 python bench.py --full --steps 100 \
        --warmup 20 --batch $B --cpu-budget 0 --no-secondary 2>/dev/null | python -c "
import sys, json
d = json.loads(sys.stdin.readline())
k = d['roofline']['per_kernel_ms']
print('B=$B', 'rows/CU=%.0f' % ($B * 286 / 256), 'wide  ' if $w else 'narrow', d['value'], d['ms_per_step'], 'tdnn5_pool', k['tdnn5_pool'], flush=True)"
    done
  done
  ;;
trace)
  P=$(realpath $2); out=$3; mkdir -p $out
  XVEC_LIB=$P timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $out/before -o before -- python bench.py --gpus 1 --steps 20 --warmup 5 > $out/before.log 2>&1
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $out/after -o after -- python bench.py --gpus 1 --steps 20 --warmup 5 > $out/after.log 2>&1
  ;;
pmc)
  P=$(realpath $2); out=$3; mkdir -p $out
  C="SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_INSTS_VMEM_RD SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT"
  XVEC_LIB=$P timeout -k 10 400 rocprofv3 --pmc $C --output-format csv -d $out/before -o before -- python bench.py --gpus 1 --steps 3 --warmup 1 > $out/before.log 2>&1
  timeout -k 10 400 rocprofv3 --pmc $C --output-format csv -d $out/after -o after -- python bench.py --gpus 1 --steps 3 --warmup 1 > $out/after.log 2>&1
  for b in before after; do echo "== $b"; python profiles/summarize_pmc.py $out/$b | grep -A5 -e split3 ; done
  ;;
*) echo "usage: $0 ab <parent.so> | sweep | trace <parent.so> <dir> | pmc <parent.so> <dir>"; exit 2 ;;
esac
