set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p gpurun_out
for hop in 6 10 14 18 26; do
  # bench.py --svc --full --no-cpu-baseline (--full: the bit-exactness check), logged by gpu_steps.sh as svchop_<hop>_svc.log
  o=$(HL_AMD_PIPE_HOP=$hop bash tools/gpu_steps.sh svchop_$hop svc) || { echo "$o"; exit 1; }
  echo "hop $hop: $(echo "$o" | grep -o '"value": [0-9.]*' | head -1) $(echo "$o" | grep -o '"bitexact": [a-z]*')"
done
