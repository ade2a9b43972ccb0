#!/usr/bin/env python3
"""What the covariance entries achieve on the cases of tests/test_gpu_cov_accuracy.py (all pairs on the 24 x 12 scenes, the
request edges, reduced systems above 256 rows, tag_translation_covariance, intrinsics_system): one JSON line per case,
appended to profiles/covariance_accuracy.jsonl -- scene, elimination, request, the deviations of the two float64 CPU
references from the longdouble inverse (A: numpy's inverse, B: the device's scheme in numpy; tests/cov_cases.py), the
device's deviation and its ratio to the bound the tests assert (8 x the references' larger deviation; the tests fail
above ratio 1).  Needs the GPU.

    python tools/covariance_accuracy.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_cov_accuracy as T  # noqa: E402


def g4(x):
    return float("%.4g" % x)


def rounded(rec):
    out = dict(rec)
    out["reference_deviation"] = {k: g4(v) for k, v in rec["reference_deviation"].items()}
    for k in ("bound", "deviation", "ratio_to_bound"):
        out[k] = g4(rec[k])
    return out


def all_records(eng, O):
    """(part, record, failures) of every case of the test module."""
    for name in T.ALL_PAIRS_SCENES:
        for elim in T.ELIMS:
            bad, recs, _ = T.run_all_pairs(eng, name, elim)
            yield "all pairs", recs, bad
    for elim in T.ELIMS:
        bad, recs = T.run_request_edges(eng, elim)
        yield "request edges", recs, bad
    for name, elim in T.BIG_SCENES:
        bad, recs = T.run_big(eng, name, elim)
        yield "more than 256 rows", recs, bad
    for name in T.TRANSLATION_SCENES:
        for elim in T.ELIMS:
            bad, recs = T.run_translation(eng, name, elim)
            yield "tag translations", recs, bad
    for name in ("ragged_tags", "ragged_cams"):
        for elim in T.ELIMS:
            bad, recs = T.run_model(eng, O, name, elim)
            yield "intrinsics_system", recs, bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance_accuracy.jsonl"))
    args = ap.parse_args()
    from oracle import oracle as O
    from visual_marker_mapping_amd import engine as eng
    O.build()
    worst, failures = {}, []
    with open(args.out, "a") as f:
        for part, recs, bad in all_records(eng, O):
            failures += bad
            for rec in recs:
                f.write(json.dumps(dict(part=part, **rounded(rec))) + "\n")
                worst[part] = max(worst.get(part, 0.0), rec["ratio_to_bound"])
    for part, r in worst.items():
        print("%-20s worst ratio to the bound %.3f" % (part, r))
    for line in failures[:40]:
        print("FAILED", line)
    print("wrote", args.out)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
