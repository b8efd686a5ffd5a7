#!/bin/bash
# Closing measurements without the counter passes: parity suite, rocprofv3
# kernel stats of bench.py, every config, the element-size / block-size modes.
set -o pipefail
TAG=${1:-cs}
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd "$(dirname "$0")/.."
export OUT=${OUT:-bench_out}  # results directory
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread -p no:cacheprovider > $OUT/${TAG}_pytest.log 2>&1 && \
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o run -- python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/${TAG}_prof_bench.json 2> $OUT/${TAG}_prof.err && \
bash tools/bench_all.sh ${TAG}_ball > $OUT/${TAG}_ball.txt 2>&1 && \
GIB=4 timeout -k 10 400 bash tools/bench_modes.sh ${TAG}_modes > $OUT/${TAG}_modes.txt 2>&1
rc=$?
tail -2 $OUT/${TAG}_pytest.log
exit $rc
