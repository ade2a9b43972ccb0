#!/usr/bin/env python3
"""What vmm_ba_predict_localization_joint achieves on the cases of tests/test_gpu_predict_joint.py: one JSON line per case,
appended to profiles/predict_joint_accuracy.jsonl -- the deviations of the two float64 CPU references from the longdouble
truth (tests/predict_joint_cases.py), the device's deviation per quantity (cov = cov_px, prop = cov_map, the sigmas) and
its ratio to the bound the tests assert (8 x the references' larger deviation; the tests fail above ratio 1).  The
block-diagonal cases also say how far cov_map lies from vmm_ba_predict_localization's.  Needs the GPU.

    python tools/predict_joint_accuracy.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import predict_joint_cases as pj  # noqa: E402
import test_gpu_predict_joint as T  # noqa: E402
from finished_map_accuracy import g4, rounded  # noqa: E402


def all_records(eng, O, adjusted):
    for n_tags in pj.JOINT_TAGS:
        for kind in T.KINDS:
            yield T.run_accuracy(eng, O, n_tags, kind, adjusted)
    for n_tags in (2, 65, 129):
        yield T.run_against_independent(eng, O, n_tags)
    yield T.run_edges(eng, O, adjusted)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_joint_accuracy.jsonl"))
    args = ap.parse_args()
    from oracle import oracle as O
    from visual_marker_mapping_amd import engine as eng
    O.build()
    adjusted = T.bundle_adjusted()
    worst, failures = {}, []
    with open(args.out, "a") as f:
        for bad, recs in all_records(eng, O, adjusted):
            failures += bad
            for rec in recs:
                line = rounded(rec)
                for k in ("gap_to_independent_entry", "bound_of_independent_entry"):
                    if k in line:
                        line[k] = g4(line[k])
                f.write(json.dumps(line) + "\n")
                f.flush()
                for q, r in rec["ratio_to_bound"].items():
                    worst[q] = max(worst.get(q, 0.0), r)
    for q, r in worst.items():
        print("predict_joint  %-9s worst ratio to the bound %.3f" % (q, r))
    for line in failures[:60]:
        print("FAILED", line)
    print("wrote", args.out)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
