# Full GPU validation: pytest -m gpu, smoke, 1B bench, kernel profile, secondary configs.
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$ROOT/bench_out}
cd $ROOT
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 900 python -m pytest tests -m gpu -q > $OUT/pytest_gpu.log 2>&1
rc=$?; echo "pytest exit $rc" >> $OUT/pytest_gpu.log; tail -8 $OUT/pytest_gpu.log
[ $rc -eq 0 ] || [ $rc -eq 1 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke.log 2>&1 || exit 1
tail -2 $OUT/smoke.log
timeout -k 10 600 python bench.py --full > $OUT/bench_default.log 2>&1 || exit 1
grep '^{' $OUT/bench_default.log
cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_join1b -o join -- python3 $ROOT/bench.py --steps 1 --warmup 1 > $OUT/prof_join1b.log 2>&1 || exit 1
cd $ROOT && python tools/prof_summary.py $OUT/prof_join1b/join_results.db 30 > $OUT/prof_join1b_summary.txt; head -12 $OUT/prof_join1b_summary.txt
timeout -k 10 900 python tools/bench_suite.py > $OUT/bench_suite.log 2>&1 || exit 1
grep -v amdgpu $OUT/bench_suite.log
