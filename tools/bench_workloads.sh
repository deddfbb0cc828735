# bench lines for non-default workloads (WORKLOADS), pipelined and --no-pipeline (VARIANTS), after the GPU tests in TESTS
# (the full line, bench.py --full: latency, kernel timing, roofline, parity); logs and JSON lines go to $OUT (bench_out/)
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p "$OUT"; export TMPDIR=/tmp
T=${TAG:-wl}
if [ "${SKIP_TESTS:-0}" != 1 ]; then
timeout -k 10 400 python -u -m pytest ${TESTS:-tests/test_gpu_pipeline.py} -x -v --timeout 200 --timeout-method thread -p no:cacheprovider > $OUT/$T.pytest.log 2>&1; rc=$?; tail -4 $OUT/$T.pytest.log; [ $rc -ne 0 ] && exit $rc
fi
for wl in ${WORKLOADS:-config3 config5 config3j}; do
  for v in ${VARIANTS:-pipe serial}; do
    extra=""; [ $v = serial ] && extra="--no-pipeline"
    timeout -k 10 400 python bench.py --full --workload $wl --steps 200 --warmup 20 $extra ${BENCH_ARGS:-} > $OUT/$T.$wl.$v.log 2>&1 || exit $?
    grep '^{' $OUT/$T.$wl.$v.log > $OUT/$T.$wl.$v.json
    V="$wl $v" python3 -c "import json,os; d=json.load(open('$OUT/$T.$wl.$v.json')); print(os.environ['V'], round(d['value']/1e6,2), d['ms_per_step'], d.get('host_submit_ms_per_step'), d['p99_batch_latency_ms'], d['kernel_avg_us'], d['roofline'].get('frac'), d['parity_vs_oracle'])"
  done
done
echo done
