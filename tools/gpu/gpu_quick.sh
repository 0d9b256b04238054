# Quick GPU validation: pytest -m gpu, smoke, default bench.
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$ROOT/bench_out}
cd $ROOT
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/pytest_gpu.log 2>&1
rc=$?; echo "pytest exit $rc" >> $OUT/pytest_gpu.log; tail -8 $OUT/pytest_gpu.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || exit 1
tail -2 $OUT/smoke.log
timeout -k 10 600 python bench.py --full > $OUT/bench_default.log 2>&1 || exit 1
grep '^{' $OUT/bench_default.log
