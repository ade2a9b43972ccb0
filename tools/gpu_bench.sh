set -x
export OUT=${OUT:-out}   # where this script writes
cd $GRAFT_REPO_ROOT
mkdir -p $OUT
timeout -k 10 600 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; tail -5 $OUT/bench.err; cat $OUT/bench.json
