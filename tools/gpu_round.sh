#!/bin/bash
# One GPU round: parity tests, bench, rocprofv3 kernel stats.  Each GPU step
# has its own time limit; steps are chained with && so a failure stops it.
set -o pipefail
TAG=${1:-r}
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd "$(dirname "$0")/.."
export OUT=${OUT:-bench_out}  # results directory
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -p no:cacheprovider > $OUT/${TAG}_pytest.log 2>&1 && \
timeout -k 10 400 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err && \
export TMPDIR=/tmp && \
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o run -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/${TAG}_prof.log 2>&1
rc=$?
tail -3 $OUT/${TAG}_pytest.log
cat $OUT/${TAG}_bench.json 2>/dev/null
exit $rc
