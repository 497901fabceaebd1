# usage (on the GPU box): bash tools/diag/profile_shape.sh TAG B T V S -- rocprofv3 kernel stats of one loss call shape
TAG=$1; shift
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-build/measure}; mkdir -p "$OUT"     # where the logs and profiles go
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/shape_$TAG -o s -- python3 tools/diag/time_shape.py "$@" > $OUT/shape_$TAG.log 2>&1 < /dev/null
grep "us per call" $OUT/shape_$TAG.log
f=$(find $OUT/shape_$TAG -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && head -12 "$f" | cut -d, -f1-4 | cut -c1-200
