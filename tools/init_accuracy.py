#!/usr/bin/env python3
"""What the one-shot map initialisation achieves on the cases of tests/test_gpu_init_accuracy.py (vmm_ba_quad_poses and
vmm_ba_initialize stage by stage: the planar solver, selection alone, one trial, the converged refinement, growth, sweep,
report): one JSON line per case, appended to profiles/init_accuracy.jsonl -- stage, case, the deviations of the two float64
CPU references from the longdouble truth at the device's state (tests/init_cases.py), the device's deviation and its ratio
to the bound the tests assert (8 x the references' larger deviation; the tests fail above ratio 1), and for the costs how
far they lie above the host optimum's (1e-9 is asked).  Needs the GPU.

    python tools/init_accuracy.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import finished_map_cases as fm  # noqa: E402
import init_cases as ic  # noqa: E402
import test_gpu_init_accuracy as T  # noqa: E402


def g4(x):
    return float("%.4g" % x) if isinstance(x, float) else x


def rounded(rec):
    return {k: ({q: ({r: g4(v) for r, v in d.items()} if isinstance(d, dict) else g4(d)) for q, d in v.items()}
                if isinstance(v, dict) else g4(v)) for k, v in rec.items()}


def all_records(eng, O):
    for model in fm.MODELS:
        yield T.run_chain(eng, model)
        for n in ic.QUAD_SIZES:
            yield T.run_quad(eng, model, n)
        yield T.run_quad_exact(eng, model)
        for fam in ic.FAMILIES:
            for winners in (False, True):
                yield T.run_select(eng, fam, model, winners)
            yield T.run_trial(eng, O, fam, model)
            yield T.run_refined(eng, O, fam, model)
        for variant in T.GROWTH_CASES:
            yield T.run_growth(eng, model, variant)
        for cap in (ic.SCORE_CAP_PX, ic.TIE_CAP_PX):
            yield T.run_sweep(eng, model, cap)
        for variant in T.REPORT_CASES:
            yield T.run_report(eng, O, model, variant)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_accuracy.jsonl"))
    args = ap.parse_args()
    from oracle import oracle as O
    from visual_marker_mapping_amd import engine as eng
    O.build()
    worst, failures = {}, []
    with open(args.out, "a") as f:
        for bad, rec in all_records(eng, O):
            failures += bad
            if rec is None:
                continue
            f.write(json.dumps(rounded(rec)) + "\n")
            f.flush()
            for q, r in rec.get("ratio_to_bound", {}).items():
                worst[(rec["entry"], q)] = max(worst.get((rec["entry"], q), 0.0), r)
    for (entry, q), r in worst.items():
        print("%-12s %-9s worst ratio to the bound %.3f" % (entry, q, r))
    for line in failures[:60]:
        print("FAILED", line)
    print("wrote", args.out)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
