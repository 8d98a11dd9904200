set -o pipefail
# usage: bash tools/gpu_wide.sh [OUTPUT_DIR]   (default: a fresh temporary directory)
O=${1:-$(mktemp -d)}; mkdir -p $O; echo "results in $O"
timeout -k 10 300 python -u -m pytest tests/test_gpu_wide.py -x -v --timeout 120 --timeout-method thread > $O/pytest.log 2>&1; rc=$?
tail -30 $O/pytest.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --workload c5 --steps 5 --warmup 2 --no-cpu-baseline > $O/bench_c5.json 2> $O/bench_c5.err; rc=$?
cat $O/bench_c5.json; tail -3 $O/bench_c5.err
exit $rc
