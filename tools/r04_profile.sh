# round-4 profile pass on the GPU box (after tools/r04_measure.sh): kernel stats of the driver's bench command with --full (the configs
# block), HBM traffic of the headline kernels, SQ + traffic counters of every other configuration's kernels.  Logs and kernel stats go
# to $OUT (a new temporary directory unless it is set), the counter files where tools/pmc_traffic.sh and tools/pmc_any.sh put them.
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$(mktemp -d)}
mkdir -p "$OUT" && echo "outputs in $OUT"
cd "$ROOT"
TAG=${TAG:-r04}
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_${TAG} -- python3 $ROOT/bench.py --gpus 1 --steps 20 --warmup 5 --full --no-cpu-baseline > /tmp/prof_${TAG}.log 2>&1; find /tmp/prof_${TAG} -name "*kernel_stats.csv" -exec cp {} $OUT/${TAG}_kernel_stats.csv \; ; grep '^{"metric"' /tmp/prof_${TAG}.log > $OUT/${TAG}_bench_under_rocprof.json)
echo "kernel stats done" | tee -a $OUT/${TAG}_progress.log
PMC_OUT=${TAG}_pmc_traffic.json bash tools/pmc_traffic.sh > $OUT/${TAG}_pmc.log 2>&1; echo "pmc traffic rc=$?" | tee -a $OUT/${TAG}_progress.log
bash tools/pmc_any.sh ${TAG}_pmc_c3.json python3 tools/bench_configs.py c3 > $OUT/${TAG}_pmc_c3.log 2>&1; echo "c3 rc=$?" | tee -a $OUT/${TAG}_progress.log
bash tools/pmc_any.sh ${TAG}_pmc_c5.json python3 tools/bench_configs.py c5 > $OUT/${TAG}_pmc_c5.log 2>&1; echo "c5 rc=$?" | tee -a $OUT/${TAG}_progress.log
bash tools/pmc_any.sh ${TAG}_pmc_c4.json python3 tools/bench_configs.py c4 16 > $OUT/${TAG}_pmc_c4.log 2>&1; echo "c4 rc=$?" | tee -a $OUT/${TAG}_progress.log
bash tools/pmc_any.sh ${TAG}_pmc_c5aem.json python3 tools/bench_configs.py c5aem 128 > $OUT/${TAG}_pmc_c5aem.log 2>&1; echo "c5aem rc=$?" | tee -a $OUT/${TAG}_progress.log
bash tools/pmc_any.sh ${TAG}_pmc_c2b.json python3 tools/bench_configs.py c2b > $OUT/${TAG}_pmc_c2b.log 2>&1; echo "c2b rc=$?" | tee -a $OUT/${TAG}_progress.log
