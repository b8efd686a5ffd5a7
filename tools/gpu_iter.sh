#!/bin/bash
# Quick GPU iteration: parity tests (optionally -k filter), A/B of encoder
# variants, one bench line.  Each GPU step has its own time limit; steps are
# chained with && so a failure stops the call.
set -o pipefail
TAG=${1:-it}
K=${2:-}
AB=${3:-0,2}
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd "$(dirname "$0")/.."
export OUT=${OUT:-bench_out}  # results directory
mkdir -p $OUT
KARG=()
[ -n "$K" ] && KARG=(-k "$K")
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 600 --timeout-method thread -p no:cacheprovider "${KARG[@]}" > $OUT/${TAG}_pytest.log 2>&1 && \
timeout -k 10 300 python -u tools/ab.py $AB 2 1 3 > $OUT/${TAG}_ab.log 2>&1 && \
timeout -k 10 300 python -u tools/ab.py $AB 2 2 2 > $OUT/${TAG}_ab_g2.log 2>&1 && \
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
rc=$?
tail -4 $OUT/${TAG}_pytest.log
cat $OUT/${TAG}_ab.log $OUT/${TAG}_ab_g2.log $OUT/${TAG}_bench.json 2>/dev/null
exit $rc
