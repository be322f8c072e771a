#!/bin/bash
# One-box A/B of library variants (tools/var_build.sh) on bench lines:
#   tools/lib_ab.sh <lines, e.g. j14,j16> <name> ...   (two rounds, alternating order)
# Results go to $RINGO_OUT (default: bench_out/ in the repository).
set -o pipefail
R=$GRAFT_REPO_ROOT
O=${RINGO_OUT:-$R/bench_out}
cd $R && mkdir -p $O
lines=$1; shift
out=$O/lib_ab.txt
: > $out
for rep in 1 2; do
  for v in "$@"; do
    RINGO_LIB=$R/ringo-snark_amd/vlib/libringo_$v.so timeout -k 10 300 python3 bench.py --full --no-ntt --extra $lines --no-cpu > $O/lab_$v.json 2> $O/lab_$v.err || { echo "$v FAILED"; tail -5 $O/lab_$v.err; exit 1; }
    python3 - "$v" "$O" <<'PY' | tee -a $out
import json, sys
v = sys.argv[1]
d = json.load(open(f"{sys.argv[2]}/lab_{v}.json"))
parts = []
for k, x in d.items():
    if isinstance(x, dict) and "value" in x:
        ms = x.get("ms_per_batch", x.get("ms_per_step"))
        parts.append(f"{k} {x['value']:.1f} ms {ms:.3f}" if ms is not None else f"{k} {x['value']:.1f}")
print(v, " | ".join(parts))
PY
  done
done
