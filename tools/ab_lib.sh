#!/bin/bash
# A/B two builds of librrte_hip.so on a GPU machine, interleaved rounds (headline + 4K stress).
# usage: bash tools/ab_lib.sh <libA.so> <libB.so>   (build B in-tree, copy the other build to A)
# Logs and the table go to $AB_OUT (default build/ab_lib).
set -o pipefail
A=${1:?libA}; B=${2:?libB}
OUT=${AB_OUT:-build/ab_lib}
mkdir -p $OUT
for r in 1 2; do for v in A B; do
  if [ $v = A ]; then L=$A; else L=$B; fi
  RRTE_HIP_LIB=$L timeout -k 10 200 python -u bench.py --full --no-cpu --no-stock > $OUT/ab_$v.log 2>&1 || exit 1
  tail -1 $OUT/ab_$v.log | python -c 'import json,sys; d=json.loads(sys.stdin.read()); print("'$v' sdf", d["value"], d["ms_per_step"], d["roofline"]["avg_launch_ms"])' | tee -a $OUT/ab.txt
  RRTE_HIP_LIB=$L timeout -k 10 200 python -u bench.py --full --no-cpu --no-stock --scene deformation-stress --width 3840 --height 2160 --steps 10 --warmup 3 > $OUT/ab_s$v.log 2>&1 || exit 1
  tail -1 $OUT/ab_s$v.log | python -c 'import json,sys; d=json.loads(sys.stdin.read()); print("'$v' stress", d["value"], d["ms_per_step"], d["roofline"]["avg_launch_ms"])' | tee -a $OUT/ab.txt
done; done
