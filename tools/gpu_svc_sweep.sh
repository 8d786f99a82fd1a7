# SVC tests, then bench.py --svc under chunk:pipeline-workgroup settings
#   CFGS="8:0 31:128" NOTEST=1 bash tools/gpu_svc_sweep.sh <tag>
set -o pipefail
tag=${1:-sweep}
mkdir -p gpurun_out
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
[ -n "$NOTEST" ] || bash tools/gpu_svc.sh || exit 1
for cfg in ${CFGS:-8:0 31:0}; do
    c=${cfg%%:*}; w=${cfg##*:}
    # bench.py --svc --full (the bit-exactness check and the CPU baseline), logged by gpu_steps.sh as <tag>_c<c>_w<w>_svc_cpu.log
    o=$(HL_AMD_SVC_CHUNK=$c HL_AMD_PIPE_WG=$w bash tools/gpu_steps.sh ${tag}_c${c}_w${w} svc_cpu) || { echo "$o"; exit 1; }
    echo "chunk $c wg $w: $(echo "$o" | grep -o '"value": [0-9.]*' | head -1) $(echo "$o" | grep -o '"bitexact": [a-z]*')"
done
