# usage (on an MI355X, from the repo root): [ROUND=r06] bash tools/diag/measure.sh TAG [full]
# bench line + rocprofv3 kernel stats + SQ counters (+ FETCH/WRITE passes with PMC=1) of the default bench command;
# ROUND is the prefix of the round's record names
TAG=${1:-x}
ROUND=${ROUND:-r06}
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-build/measure}; mkdir -p "$OUT"     # where the logs and profiles go
FLAGS="--no-cpu-baseline --no-decode --no-wide"
[ "$2" = full ] && python3 bench.py --full --steps 20 --warmup 5 > $OUT/bench_${ROUND}_$TAG.json 2> $OUT/bench_${ROUND}_$TAG.err
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o c2 -- python3 bench.py --full --steps 20 --warmup 5 $FLAGS > $OUT/prof_$TAG.log 2>&1
rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY --output-format csv -d $OUT/pmc_${TAG}_sq -o pmc -- python3 bench.py --full --steps 5 --warmup 2 $FLAGS > $OUT/pmc_${TAG}_sq.log 2>&1
python3 tools/diag/pmc_summary.py $OUT/pmc_${TAG}_sq
if [ -n "$PMC" ]; then
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_${TAG}_fetch -o pmc -- python3 bench.py --full --steps 5 --warmup 2 $FLAGS > $OUT/pmc_${TAG}_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_${TAG}_write -o pmc -- python3 bench.py --full --steps 5 --warmup 2 $FLAGS > $OUT/pmc_${TAG}_write.log 2>&1
python3 tools/diag/pmc_summary.py $OUT/pmc_${TAG}_fetch
python3 tools/diag/pmc_summary.py $OUT/pmc_${TAG}_write
fi
find $OUT/prof_$TAG -name "*kernel_stats.csv" | head -1 | xargs head -8 | cut -c1-180
grep '^{"metric' $OUT/prof_$TAG.log | tail -1 | python3 -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1])
print({k:d[k] for k in ('value','ms_per_step','module_ms_per_step')}, d['roofline']['kernel_ms'], d['roofline']['frac'], d['roofline']['peak_measured'])
"
if [ "$2" = full ]; then
# the other kernel families, the wide-alphabet share in both dtypes, the word-piece shapes
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_others_$TAG -o others -- python3 tools/diag/profile_others.py > $OUT/prof_others_$TAG.log 2>&1 < /dev/null
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_c5_f32_$TAG -o c5 -- python3 tools/diag/profile_c5.py > $OUT/prof_c5_f32_$TAG.log 2>&1 < /dev/null
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_c5_bf16_$TAG -o c5 -- python3 tools/diag/profile_c5.py bf16 > $OUT/prof_c5_bf16_$TAG.log 2>&1 < /dev/null
bash tools/diag/profile_shape.sh wp8k_$TAG 64 256 8000 200 > /dev/null
bash tools/diag/profile_shape.sh wp32k_$TAG 16 150 32000 120 > /dev/null
bash tools/diag/profile_shape.sh mid_$TAG 256 1000 200 200 > /dev/null
fi
if [ "$2" = full ]; then
# the emission regimes with the flagged launch's phases, the cliff scan, the beam's phases
python3 tools/diag/flagged_phases.py > $OUT/${ROUND}_flagged_phases_$TAG.txt 2>&1
python3 tools/diag/cliff_scan.py > $OUT/${ROUND}_cliff_scan_$TAG.txt 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_regimes_$TAG -o regimes -- python3 tools/diag/emission_regimes.py > $OUT/prof_regimes_$TAG.log 2>&1 < /dev/null
fi
