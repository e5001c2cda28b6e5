#!/bin/bash
# One GPU session made of named steps (replaces round 5's 35 one-off scripts/sessions/r05*.sh):
#     TAG=r06a bash scripts/session.sh gputest smoke bench_k20 nccl1 ...
# Each step runs under scripts/gpu_session.sh (its own time limit; a crash, abort or timeout ends the session) and
# writes gpurun_out/${TAG}_<step>.log (rocprofv3 steps: gpurun_out/${TAG}_<step>/); scripts/keep_profiles.py ${TAG}_
# then copies the judged pieces into profiles/.  A step that is not a preset name is taken as "name:timeout:command".
cd "${GRAFT_REPO_ROOT:-/root/repo}"
t=${TAG:?set TAG, e.g. TAG=r06a}
W1PORT=${W1PORT:-29631}
# step_logdir: the folder of the running step's log.  scripts/gpu_session.sh points each step's stdout at its log file; a
# rocprofv3 step keeps its trace folder beside it.  Fails the step where stdout is not a file (a pipe, a terminal).
step_logdir() {
  local f; f=$(readlink "/proc/$$/fd/1")
  [ -f "$f" ] || { echo "step_logdir: this step's stdout is not a log file ($f)" >&2; return 1; }
  dirname "$f"
}
export -f step_logdir
steps=()
for s in "$@"; do
  case "$s" in
    gputest)         steps+=("${t}_gputest:420:python -u -m pytest tests -m gpu -q --timeout 120 --timeout-method thread");;
    smoke)           steps+=("${t}_smoke:120:python -c 'import __graft_entry__ as g; g.smoke()'");;
    bench_k20)       steps+=("${t}_bench_k20:240:python bench.py --full --gpus 1 --steps 20 --warmup 5");;
    bench)           steps+=("${t}_bench:360:python bench.py --full --resident");;
    nccl1)           steps+=("${t}_nccl1:300:python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port ${W1PORT} bench.py --full --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline");;
    prof_canonical)  steps+=("${t}_prof_canonical:300:d=\$(step_logdir) && rocprofv3 --kernel-trace --stats -d \$d/${t}_prof_canonical -o run --output-format csv -- python bench.py --full --no-cpu-baseline --steps 200 --sustained-steps 0");;
    bench_ragged)    steps+=("${t}_bench_ragged:400:python bench.py --full --workload ragged");;
    prof_ragged)     steps+=("${t}_prof_ragged:300:d=\$(step_logdir) && rocprofv3 --kernel-trace --stats -d \$d/${t}_prof_ragged -o run --output-format csv -- python bench.py --full --workload ragged --no-cpu-baseline --steps 200 --sustained-steps 0");;
    bench_balance)   steps+=("${t}_bench_balance4096:300:python bench.py --full --workload balance --walkers 4096 --graph --resident --steps 1000 --warmup 100");;
    bench_balance_direct) steps+=("${t}_bench_balance4096_direct:300:python bench.py --full --workload balance --walkers 4096 --resident --steps 1000 --warmup 100 --no-cpu-baseline");;
    bench_chain)     steps+=("${t}_bench_chain:400:python bench.py --full --workload chain --walkers 4096 --chain-points 100 --steps 100 --warmup 10 --cpu-seconds 10");;
    bench_perfdemo)  steps+=("${t}_bench_perfdemo:400:python bench.py --full --workload perfdemo --walkers 4096 --chain-points 100 --steps 100 --warmup 10 --cpu-seconds 10");;
    pmc)             steps+=("${t}_pmc:400:bash scripts/gpu_pmc.sh ${t}_pmc_canonical && WG_WORKLOAD=ragged bash scripts/gpu_pmc.sh ${t}_pmc_ragged");;
    pmc_valu)        steps+=("${t}_pmc_valu:300:bash scripts/gpu_pmc.sh ${t}_valu_canonical valu");;
    *)               steps+=("$s");;
  esac
done
exec bash scripts/gpu_session.sh "${steps[@]}"
