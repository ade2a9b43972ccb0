set -x
export OUT=${OUT:-out}   # where this script writes
cd $GRAFT_REPO_ROOT
mkdir -p $OUT/prof
export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o r01 -- python bench.py --full --steps 35 --warmup 7 --no-cpu-baseline > $OUT/prof/bench_under_rocprof.json 2> $OUT/prof/err.log
tail -3 $OUT/prof/err.log
find $OUT/prof -type f | head -20
f=$(find $OUT/prof -name '*kernel_stats.csv' | head -1); cat $f
# keep only the small summaries (the per-dispatch trace is large)
find $OUT/prof -name '*kernel_trace.csv' -size +4M -delete
