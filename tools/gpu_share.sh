#!/bin/bash
# Streams sharing one GPU: bench.py's driver workload (--steps 20 --warmup 5)
# with 1, 2 and 4 ranks on the box's one GPU (each rank its own stream and its
# share of the CUs).  GPU box, repo root:  bash tools/gpu_share.sh [steps]
set -o pipefail
mkdir -p gpurun_out
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
steps=${1:-20}
for n in ${NS:-1 2 4}; do
  # torchrun with n ranks, bench.py --full --no-cpu-baseline (--full: the bit-exactness check); gpu_steps.sh logs it as gpu_share_<n>.log
  o=$(SHARE_STEPS=$steps bash tools/gpu_steps.sh gpu share_$n) || { echo "$o"; exit 1; }
  echo "$o" | grep '^{' | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print($n, 'ranks:', d['value'], 'fps total, bitexact', d['bitexact'], d['pipeline'])"
done
