# Radix-join iteration: correctness tests, 1B bench, kernel profile.
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$ROOT/bench_out}
cd $ROOT
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 python -m pytest tests/test_gpu_kernels.py -m gpu -q -k "radix or large_join" > $OUT/pytest_radix.log 2>&1
rc=$?; echo "radix pytest exit $rc" >> $OUT/pytest_radix.log; tail -15 $OUT/pytest_radix.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full --steps 3 --warmup 1 > $OUT/bench_1b.log 2>&1 || exit 1
grep '^{' $OUT/bench_1b.log
cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_join1b -o join -- python3 $ROOT/bench.py --steps 1 --warmup 1 > $OUT/prof_join1b.log 2>&1 || exit 1
cd $ROOT && python tools/prof_summary.py $OUT/prof_join1b/join_results.db 30 > $OUT/prof_join1b_summary.txt; cat $OUT/prof_join1b_summary.txt
