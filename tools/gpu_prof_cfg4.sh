# rocprofv3 kernel statistics of the 2000 x 1000 problem (BASELINE configs[3], f32 accumulation)
export OUT=${OUT:-out}   # where this script writes
cd $GRAFT_REPO_ROOT
mkdir -p $OUT/cfg4
export TMPDIR=/tmp
timeout -k 10 800 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/cfg4 -o c4 -- python bench.py --full --config 4 --steps 8 --warmup 0 --no-cpu-baseline > $OUT/cfg4/bench.json 2> $OUT/cfg4/err.log || exit 1
find $OUT/cfg4 -name '*.csv' -size +4M -delete
cut -d, -f1-5 $OUT/cfg4/c4_kernel_stats.csv | head -8
