#!/bin/bash
# Run on the GPU box (gpurun): a short bench per environment setting; prints ms_per_step and the step's parts.  usage: bash tools/sweep_env.sh "A=0" "A=1 B=2" ...
cd "$GRAFT_REPO_ROOT"
T=$(mktemp -d)
for V in "$@"; do
  echo "== $V"
  env $V LSG_TIMING=1 timeout -k 10 200 python3 bench.py --full --steps 8 --warmup 2 --no-cpu-baseline --e2e-reads 0 --no-c4 > $T/sw.log 2> $T/sw.err || { echo bench failed; tail -5 $T/sw.err; continue; }
  python3 -c "
import json
d=json.loads([l for l in open('$T/sw.log') if l.startswith('{')][-1])
print(round(d['ms_per_step'],2), d['config']['step_parts_ms_rank0'], d['config']['recount_ms'], d['config']['sites_counted'], d['config']['step1_candidates'])
"
done
