set -x
export OUT=${OUT:-out}   # where this script writes
cd $GRAFT_REPO_ROOT
mkdir -p $OUT
timeout -k 10 900 python -m pytest tests -m gpu -x -q 2>&1 | tail -15 > $OUT/pytest_gpu.log; cat $OUT/pytest_gpu.log
grep -q passed $OUT/pytest_gpu.log && ! grep -q failed $OUT/pytest_gpu.log && bash tools/gpu_stamps.sh && timeout -k 10 600 python bench.py --full --no-cpu-baseline > $OUT/bench.json 2> $OUT/bench.err; tail -3 $OUT/bench.err; cat $OUT/bench.json
