#!/bin/bash
# Bench lines for every workload + rocprofv3 kernel-trace summaries of the single-launch (--lanes 1) runs.
# usage: gpu_bench_all.sh <tag>   (outputs under gpurun_out/<tag>_*)
cd "${GRAFT_REPO_ROOT:-/root/repo}"
t=${1:-r02}
S=scripts/gpu_session.sh
# step_logdir: the folder of the running step's log.  scripts/gpu_session.sh points each step's stdout at its log file; a
# rocprofv3 step keeps its trace folder beside it.  Fails the step where stdout is not a file (a pipe, a terminal).
step_logdir() {
  local f; f=$(readlink "/proc/$$/fd/1")
  [ -f "$f" ] || { echo "step_logdir: this step's stdout is not a log file ($f)" >&2; return 1; }
  dirname "$f"
}
export -f step_logdir
$S "${t}_bench_canonical:300:python bench.py --full --resident" \
   "${t}_prof_canonical:300:d=\$(step_logdir) && rocprofv3 --kernel-trace --stats -d \$d/${t}_prof_canonical -o run --output-format csv -- python bench.py --full --no-cpu-baseline" \
   "${t}_bench_ragged:400:python bench.py --full --workload ragged" \
   "${t}_prof_ragged:300:d=\$(step_logdir) && rocprofv3 --kernel-trace --stats -d \$d/${t}_prof_ragged -o run --output-format csv -- python bench.py --full --workload ragged --no-cpu-baseline" \
   "${t}_bench_balance4096:300:python bench.py --full --workload balance --walkers 4096 --graph --steps 1000 --warmup 100" \
   "${t}_bench_balance65536:300:python bench.py --full --workload balance --no-cpu-baseline" \
   "${t}_bench_chain:400:python bench.py --full --workload chain --walkers 4096 --chain-points 100 --steps 100 --warmup 10 --cpu-seconds 10"
