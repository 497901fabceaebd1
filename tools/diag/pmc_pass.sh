# usage (GPU box, repo root): bash tools/diag/pmc_pass.sh TAG "COUNTER COUNTER ..."   (<= 8 SQ counters per pass)
TAG=$1; shift
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-build/measure}; mkdir -p "$OUT"     # where the logs and profiles go
rocprofv3 --pmc $1 --output-format csv -d $OUT/pmc_$TAG -o pmc -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-decode --no-wide > $OUT/pmc_$TAG.log 2>&1
python3 tools/diag/pmc_summary.py $OUT/pmc_$TAG
