#!/bin/bash
# the round's measurement set in one GPU session: tools/gpu_final.sh <tag>   (e.g. r06_v1)
#   profiles (bench lines c3 / c2 / c5, kernel stats, PMC traffic + limiter passes) -> $OUT_DIR/<tag>_* (default results/), the two
#   JSON files bench.py reads copied into profiles/ on the box, then the full bench once more WITH them, then the GPU test suite with
#   its parity log
tag=${1:-r06_v1}; round=${tag%%_*}
export OUT_DIR=${OUT_DIR:-$(pwd)/results}; out=$OUT_DIR
mkdir -p $out
tools/gpu_profile_all.sh $tag > $out/${tag}_profile_all.log 2>&1
cp $out/${round}_pmc_traffic.json profiles/${round}_pmc_traffic.json
cp $out/${round}_pmc_limiter.json profiles/${round}_pmc_limiter.json
python bench.py --full > $out/${tag}_bench_c3.json 2> $out/${tag}_bench_c3.log      # again, now WITH the PMC files of this build
if [ -z "$SKIP_TESTS" ]; then
  python -m pytest tests -m gpu -q -s > $out/${tag}_gpu_tests.log 2>&1
  echo "pytest rc=$?"; tail -4 $out/${tag}_gpu_tests.log
  grep -E "\[sweep|\[fp64-anchored\]|\[strict|\[heavy\]|\[scales\]" $out/${tag}_gpu_tests.log > $out/${tag}_gpu_tests_parity_log.txt
fi
tail -1 $out/${tag}_bench_c3.json | cut -c1-300
