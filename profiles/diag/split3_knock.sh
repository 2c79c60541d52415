#!/bin/bash
# Upper bound on a 384-channel tile for the bf16_split3 pooling kernel of fp32 layer 5: the knock-out builds of the S3 path of
# csrc/tdnn_layer_impl.h (-DXVEC_KNOCK=1048576 | 2097152, described there; timing only, results are garbage) interleaved with
# the shipped library.  Figures: profiles/split3_wide_bound.txt.
#   bash profiles/diag/split3_knock.sh build             needs hipcc and the shipped library's objects (make -C .../csrc first)
#   bash profiles/diag/split3_knock.sh run [N]           one GPU: N (3) interleaved rounds shipped / each knock-out build,
#                                                        per-kernel event times
# KNOCKS="1048576 2097152" selects the builds.  Every run is held to the four-wave kernel (XVEC_SPLIT3_WIDE=0): the knock-outs are
# in its pooling instantiation, and at the bench batch the planner would otherwise take the 384-channel tile (tdnn_split3w.hip).
set -e -o pipefail
root=$(cd "$(dirname "$0")/../.." && pwd)
csrc=$root/speaker-recognition-x-vectors_amd/csrc
out=$root/build/diag
masks=${KNOCKS:-1048576 2097152}
case "$1" in
build)
  for m in $masks; do
    mkdir -p $out/obj$m
    flags=$(make -s -C $csrc KNOCK=$m --eval='pf: ; @echo $(CXXFLAGS)' pf)       # the build's own flags and build id
    id=$(make -s -C $csrc KNOCK=$m --eval='pi: ; @echo $(BUILD_ID)' pi)
    (cd $csrc && for f in tdnn_split3 xvec_api; do /opt/rocm/bin/hipcc $flags -DXVEC_BUILD_ID="\"$id\"" -c $f.hip -o $out/obj$m/$f.o; done)
    objs=$(ls $csrc/*.o | grep -v -e /tdnn_split3.o -e /xvec_api.o)
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $out/libxvec_hip_knock$m.so $objs $out/obj$m/tdnn_split3.o $out/obj$m/xvec_api.o
  done
  ls -l $out/*.so
  ;;
run)
  cd $root
  for i in $(seq 1 ${2:-3}); do
    for m in 0 $masks; do
      L=; [ $m != 0 ] && L=$out/libxvec_hip_knock$m.so
      # every run under a time limit of its own; the first failure ends the script
      XVEC_LIB=$L XVEC_SPLIT3_WIDE=0 timeout -k 10 240 python bench.py --full --steps 50 --warmup 10 --cpu-budget 0 --no-secondary 2>/dev/null | python -c "
import sys, json
d = json.loads(sys.stdin.readline())
k = d['roofline']['per_kernel_ms']
print('knock=%-7s' % '$m', d['value'], d['ms_per_step'], ' '.join(f'{n}={v:.4f}' for n, v in k.items()), flush=True)"
    done
  done
  ;;
*) echo "usage: $0 build | run [rounds]"; exit 2 ;;
esac
