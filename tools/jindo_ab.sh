#!/bin/bash
# A/B of the Jindo bench lines under environment variants (run on the box via gpurun):
#   tools/jindo_ab.sh VAR "val1 val2 ..." [extra lines, default j14,j16]
# prints commits/s and ms per batch (sampled and injected) for each value of $VAR
# Results go to $RINGO_OUT (default: bench_out/ in the repository).
set -o pipefail
cd $GRAFT_REPO_ROOT
O=${RINGO_OUT:-$PWD/bench_out}
mkdir -p $O
VAR=$1
VALS=$2
LINES=${3:-j14,j16}
for v in $VALS; do
  env $VAR=$v timeout -k 10 240 python bench.py --full --no-ntt --extra $LINES --no-cpu > $O/ab_$v.json 2> $O/ab_$v.err || { echo "bench $v failed"; tail -5 $O/ab_$v.err; exit 1; }
  python3 - "$v" "$O" <<'EOF'
import json, sys
v = sys.argv[1]
d = json.load(open(f"{sys.argv[2]}/ab_{v}.json"))
for k in ("jindo_commit", "jindo_commit_2e16"):
    if k in d:
        print(v, k, round(d[k]["value"]), "ms", round(d[k]["ms_per_batch"], 3), "injected ms", round(d[k]["injected"]["ms_per_batch"], 3))
EOF
done
