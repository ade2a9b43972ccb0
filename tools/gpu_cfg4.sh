export OUT=${OUT:-out}   # where this script writes
cd $GRAFT_REPO_ROOT
mkdir -p $OUT
timeout -k 10 800 python bench.py --full --config 4 --steps 8 --warmup 0 --no-cpu-baseline > $OUT/bench_cfg4.json 2> $OUT/bench_cfg4.err; tail -3 $OUT/bench_cfg4.err; cat $OUT/bench_cfg4.json
timeout -k 10 600 python bench.py --full --config 5 --steps 40 --warmup 10 --no-cpu-baseline > $OUT/bench_cfg5.json 2> $OUT/bench_cfg5.err; tail -3 $OUT/bench_cfg5.err; cat $OUT/bench_cfg5.json
timeout -k 10 600 python bench.py --full --config 2 --visibility 0.25 --steps 40 --warmup 10 --no-cpu-baseline > $OUT/bench_v025.json 2> $OUT/bench_v025.err; tail -3 $OUT/bench_v025.err; cat $OUT/bench_v025.json
