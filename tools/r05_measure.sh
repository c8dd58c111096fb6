# round-5 measurement pass on the GPU box: tests, the driver's bench command with --full (the `configs` block), rocprofv3 kernel stats
# of it, and (PMC=1) the matrix-core counter passes.  Outputs go to $OUT (a new temporary directory unless it is set), named by TAG.
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$(mktemp -d)}
mkdir -p "$OUT" && echo "outputs in $OUT"
cd "$ROOT"
TAG=${TAG:-r05}
if [ "${TESTS:-1}" = "1" ]; then
  python -u -m pytest tests -x -q -m gpu > $OUT/${TAG}_gputests.log 2>&1; echo "tests rc=$? $(tail -1 $OUT/${TAG}_gputests.log)" | tee -a $OUT/${TAG}_progress.log
fi
python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err; echo "bench rc=$?" | tee -a $OUT/${TAG}_progress.log
if [ "${PROF:-1}" = "1" ]; then
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_${TAG} -- python3 $ROOT/bench.py --gpus 1 --steps 20 --warmup 5 --full --no-cpu-baseline > /tmp/prof_${TAG}.log 2>&1; find /tmp/prof_${TAG} -name "*kernel_stats.csv" -exec cp {} $OUT/${TAG}_kernel_stats.csv \; ; grep '^{"metric"' /tmp/prof_${TAG}.log | cut -c1-400 > $OUT/${TAG}_bench_under_rocprof.json)
echo "rocprof done" | tee -a $OUT/${TAG}_progress.log
fi
if [ "${PMC:-0}" = "1" ]; then
  bash tools/pmc_mfma.sh ${TAG}_pmc_mfma.json > $OUT/${TAG}_pmc_mfma.log 2>&1; echo "pmc_mfma rc=$?" | tee -a $OUT/${TAG}_progress.log
fi
