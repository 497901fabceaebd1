# usage (on the GPU box, from the repo root): bash tools/diag/measure_round2.sh TAG
# bench line + rocprofv3 kernel stats (+ PMC passes with PMC=1) of the default bench command
TAG=${1:-x}
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-build/measure}; mkdir -p "$OUT"     # where the logs and profiles go
python3 bench.py --full --steps 20 --warmup 5 ${BENCH_FLAGS} > $OUT/bench_r02_$TAG.json 2> $OUT/bench_r02_$TAG.err
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o c2 -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-decode --no-wide > $OUT/prof_$TAG.log 2>&1
if [ -n "$PMC" ]; then
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_${TAG}_fetch -o pmc -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-decode --no-wide > $OUT/pmc_${TAG}_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_${TAG}_write -o pmc -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-decode --no-wide > $OUT/pmc_${TAG}_write.log 2>&1
python3 tools/diag/pmc_summary.py $OUT/pmc_${TAG}_fetch
python3 tools/diag/pmc_summary.py $OUT/pmc_${TAG}_write
fi
find $OUT/prof_$TAG -name "*kernel_stats.csv" | head -1 | xargs head -8 | cut -c1-180
python3 -c "
import json
d=json.loads(open('$OUT/bench_r02_$TAG.json').read().strip().splitlines()[-1])
print({k:d[k] for k in ('value','ms_per_step','module_ms_per_step')}, d['roofline']['kernel_ms'], d['roofline']['frac'], d['roofline']['peak_measured'])
"
