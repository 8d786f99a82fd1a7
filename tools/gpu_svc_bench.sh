# Config-4 (spatial SVC) bench on one GPU box: all layers on one GPU, a
# 2-rank streams rehearsal (two ranks share the one GPU, one stream each) and
# a 3-rank layer-sharded rehearsal with gloo (three ranks share the one GPU;
# RCCL needs one GPU per rank).  bash tools/gpu_svc_bench.sh <tag>
set -o pipefail
tag=${1:-svc}
mkdir -p gpurun_out
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
bash tools/gpu_steps.sh $tag svc_cpu svc_streams2 svc_layers3 || exit 1  # bench.py --svc --full each
