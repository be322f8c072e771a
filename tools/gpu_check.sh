#!/bin/bash
# GPU smoke of the tree: parity tests, then the full bench line (run on a GPU machine).
# Results go to $RINGO_OUT (default: bench_out/ in the repository).
set -o pipefail
cd $GRAFT_REPO_ROOT
O=${RINGO_OUT:-$PWD/bench_out}
mkdir -p $O
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $O/gpu_tests.log 2>&1 || { echo TESTS FAILED; tail -30 $O/gpu_tests.log; exit 1; }
tail -2 $O/gpu_tests.log
timeout -k 10 300 python -u bench.py --full ${BENCH_ARGS:-} > $O/bench.json 2> $O/bench.err || { echo BENCH FAILED; tail -20 $O/bench.err; exit 1; }
cat $O/bench.json
