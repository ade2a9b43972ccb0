#!/usr/bin/env python3
"""What the two joint refinements over the arrowhead solver achieve on the cases of tests/test_gpu_arrowhead_accuracy.py
(calibrate, rig_calibrate): one JSON line per case and stage, appended to profiles/arrowhead_accuracy.jsonl -- entry
point, stage (covariance stage, result, one trial), case and the counts it exercises, the deviations of the two float64 CPU
references from the longdouble truth at the device's state (A: the oracle's functor, numpy's inverse and solve; B: the
device's scheme in numpy; tests/arrowhead_cases.py), the device's deviation per quantity (cost, rms, shared_cov = intr_cov /
ext_cov, item_cov = cam_cov / rig_cov, step_shared, step_pose) and its ratio to the bound the tests assert (8 x the
references' larger deviation; the tests fail above ratio 1).  Needs the GPU.

    python tools/arrowhead_accuracy.py [--out FILE] [--only ENTRY]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import arrowhead_cases as ah  # noqa: E402
import test_gpu_arrowhead_accuracy as T  # noqa: E402


def g4(x):
    return float("%.4g" % x)


def rounded(rec):
    out = dict(rec)
    out["reference_deviation"] = {ref: {q: g4(v) for q, v in d.items()} for ref, d in rec["reference_deviation"].items()}
    for k in ("bound", "deviation", "ratio_to_bound"):
        out[k] = {q: g4(v) for q, v in rec[k].items()}
    for k in ("decrement_over_cost", "truth_correction"):
        if k in out:
            out[k] = g4(out[k])
    return out


def all_runs(only):
    """(function, arguments) of every case of the test module that leaves a record."""
    if only in (None, "calibrate"):
        for args in ah.CALIB_EDGE_CASES:
            yield T.run_stage, (ah.observation_edges, args)
        yield T.run_stage, (*T.ONE_TAG[0], 1)
        for args in ah.CALIB_EDGE_CASES:
            yield T.run_result, (ah.observation_edges, args)
        for n in ah.ITEM_COUNTS:
            yield T.run_result, (ah.item_edges, (n,))
        for args in ah.CALIB_TRIAL_CASES:
            yield T.run_trial, (ah.observation_edges, args)
    if only in (None, "rig_calibrate"):
        for args in ah.RIG_EDGE_CASES:
            yield T.run_stage, (ah.rig_edges, args)
        yield T.run_stage, (*T.ONE_TAG[1], 1)
        for args in ah.RIG_EDGE_CASES:
            yield T.run_result, (ah.rig_edges, args)
        for args in T.FRAME_CASES:
            yield T.run_result, (ah.frame_edges, args)
        for args in ah.RIG_TRIAL_CASES:
            yield T.run_trial, (ah.rig_edges, args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arrowhead_accuracy.jsonl"))
    ap.add_argument("--only", default=None, help="one entry point: calibrate, rig_calibrate")
    args = ap.parse_args()
    from oracle import oracle as O
    from visual_marker_mapping_amd import engine as eng
    O.build()
    worst, failures = {}, []
    with open(args.out, "a") as f:
        for run, (build, *rest) in all_runs(args.only):
            bad, rec = run(eng, O, build, *rest)
            failures += bad
            if rec:
                f.write(json.dumps(rounded(rec)) + "\n")
                f.flush()
                for q, r in rec["ratio_to_bound"].items():
                    key = (rec["entry"], rec["stage"], q)
                    worst[key] = max(worst.get(key, 0.0), r)
    for (entry, stage, q), r in worst.items():
        print("%-14s %-16s %-11s worst ratio to the bound %.3f" % (entry, stage, q, r))
    for line in failures[:80]:
        print("FAILED", line)
    print("wrote", args.out)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
