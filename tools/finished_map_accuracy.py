#!/usr/bin/env python3
"""What the stateless calls against a finished map achieve on the cases of tests/test_finished_map_accuracy.py (localize,
rig_localize, locate_tags, triangulate, predict_localization): one JSON line per case, appended to
profiles/finished_map_accuracy.jsonl -- entry point, case, the deviations of the two float64 CPU references from the
longdouble truth at the device's state (A: the oracle's functor, numpy's inverse; B: the device's scheme in numpy;
tests/finished_map_cases.py), the device's deviation per quantity (cost, rms, cov, prop = the propagated part, the sigmas)
and its ratio to the bound the tests assert (8 x the references' larger deviation; the tests fail above ratio 1).
Needs the GPU.

    python tools/finished_map_accuracy.py [--out FILE] [--only ENTRY]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import finished_map_cases as fm  # noqa: E402
import test_finished_map_accuracy as T  # noqa: E402


def g4(x):
    return float("%.4g" % x)


def rounded(rec):
    out = dict(rec)
    out["reference_deviation"] = {ref: {q: g4(v) for q, v in d.items()} for ref, d in rec["reference_deviation"].items()}
    for k in ("bound", "deviation", "ratio_to_bound"):
        out[k] = {q: g4(v) for q, v in rec[k].items()}
    if "cost_above_host_optimum" in out:
        out["cost_above_host_optimum"] = g4(out["cost_above_host_optimum"])
    return out


def all_records(eng, O, only):
    """(records, failures) of every case of the test module."""
    for entry, (_, cases) in fm.BUILDERS.items():
        if only in (None, entry):
            for args in cases:
                bad, rec = T.run_case(eng, O, entry, args)
                yield ([rec] if rec else []), bad
    if only in (None, "triangulate"):
        for args, max_pair in T.PAIR_VIEWS:
            bad, rec = T.run_case(eng, O, "triangulate", args, options=dict(max_pair_views=max_pair))
            yield ([rec] if rec else []), bad
    if only in (None, "predict"):
        for n_tags, with_map in fm.PREDICT_CASES:
            bad, recs = T.run_predict(eng, O, n_tags, with_map)
            yield recs, bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finished_map_accuracy.jsonl"))
    ap.add_argument("--only", default=None, help="one entry point: localize, rig_localize, locate_tags, triangulate, predict")
    args = ap.parse_args()
    from oracle import oracle as O
    from visual_marker_mapping_amd import engine as eng
    O.build()
    worst, failures = {}, []
    with open(args.out, "a") as f:
        for recs, bad in all_records(eng, O, args.only):
            failures += bad
            for rec in recs:
                f.write(json.dumps(rounded(rec)) + "\n")
                f.flush()
                for q, r in rec["ratio_to_bound"].items():
                    key = (rec["entry"], q)
                    worst[key] = max(worst.get(key, 0.0), r)
    for (entry, q), r in worst.items():
        print("%-14s %-9s worst ratio to the bound %.3f" % (entry, q, r))
    for line in failures[:60]:
        print("FAILED", line)
    print("wrote", args.out)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
