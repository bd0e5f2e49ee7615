# One GPU call for a build: the -m gpu suite, then (only if it is green) the full bench line and the
# rocprofv3 passes of tools/profile_round.sh. Usage: bash tools/gpu_round.sh TAG [skip-tests]
# Outputs go under $OUT_ROOT (default bench_out/).
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
TAG=${1:-r04}
export OUT_ROOT=${OUT_ROOT:-bench_out}
mkdir -p $OUT_ROOT
if [ "$2" != "skip-tests" ]; then
  timeout -k 10 600 python -u -m pytest tests -m gpu -q -rf --timeout 240 --timeout-method thread \
    > $OUT_ROOT/pytest_gpu.log 2>&1
  rc=$?
  tail -25 $OUT_ROOT/pytest_gpu.log
  [ $rc -eq 0 ] || { echo "pytest rc=$rc: no bench"; exit $rc; }
fi
timeout -k 10 420 python -u bench.py --full > $OUT_ROOT/bench_$TAG.json 2> $OUT_ROOT/bench_$TAG.err
rc=$?
cut -c1-600 $OUT_ROOT/bench_$TAG.json
[ $rc -eq 0 ] || { tail -20 $OUT_ROOT/bench_$TAG.err; exit $rc; }
bash tools/profile_round.sh $TAG
