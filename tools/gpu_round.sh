#!/bin/bash
# one GPU round trip: the -m gpu suite (log kept), then the full bench line.   usage: tools/gpu_round.sh <tag> [pytest args]
#   -> $OUT_DIR (default results/)
tag=${1:-r03}; shift
out=${OUT_DIR:-results}
mkdir -p $out
python -m pytest tests -m gpu -q -s "$@" > $out/${tag}_gpu_tests.log 2>&1
echo "pytest rc=$?"; tail -5 $out/${tag}_gpu_tests.log
grep -E "\[sweep|\[fp64-anchored\]|\[strict|\[sinkhorn-anchored\]" $out/${tag}_gpu_tests.log > $out/${tag}_gpu_tests_parity_log.txt
python bench.py --full > $out/${tag}_bench_c3.json 2> $out/${tag}_bench_c3.log
echo "bench rc=$?"; tail -3 $out/${tag}_bench_c3.log; cut -c1-600 $out/${tag}_bench_c3.json
