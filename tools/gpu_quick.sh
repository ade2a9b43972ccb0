# Quick loop: kernel tests, bench line, rocprofv3 per-kernel stats of a short bench run.
set -x
export OUT=${OUT:-out}   # where this script writes
cd $GRAFT_REPO_ROOT
mkdir -p $OUT/q
export TMPDIR=/tmp
timeout -k 10 300 python -m pytest tests/test_gpu_kernels.py tests/test_gpu_solve.py -x -q 2>&1 | tail -3 || exit 1
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $OUT/q/bench.json 2> $OUT/q/bench.err || exit 1
python -c "
import json; d=json.load(open('$OUT/q/bench.json')); print(d['value'], d['ms_per_step']); print({k:round(v['ms']*1000,1) for k,v in d['kernels'].items()})"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/q -o prof -- python bench.py --full --steps 35 --warmup 7 --no-cpu-baseline > $OUT/q/bench_prof.json 2> $OUT/q/prof_err.log || exit 1
python - <<'PY'
import os
import csv, glob
f = glob.glob(os.environ["OUT"] + "/q/**/prof_kernel_stats.csv", recursive=True)
rows = list(csv.DictReader(open(f[0])))
for r in rows[:16]:
    print("%-70s calls %6s avg %9.1f ns  %5.1f%%" % (r["Name"][:70], r["Calls"], float(r["AverageNs"]), float(r["Percentage"])))
PY
find $OUT/q -name '*.csv' -size +6M -delete
