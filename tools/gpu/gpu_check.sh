set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$ROOT/bench_out}
cd $ROOT
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 600 python -m pytest tests/test_gpu_kernels.py -x -q > $OUT/pytest_gpu.log 2>&1
echo "pytest exit $?" >> $OUT/pytest_gpu.log
timeout -k 10 300 python __graft_entry__.py smoke > $OUT/smoke.log 2>&1 && \
timeout -k 10 300 python bench.py --full --rows 100000000 --steps 3 --warmup 1 > $OUT/bench_100m.log 2>&1 && \
timeout -k 10 600 python bench.py --full --steps 3 --warmup 1 > $OUT/bench_1b.log 2>&1
echo "chain exit $?"
tail -3 $OUT/pytest_gpu.log; cat $OUT/smoke.log $OUT/bench_100m.log $OUT/bench_1b.log | tail -20
