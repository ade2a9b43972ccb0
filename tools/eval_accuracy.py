#!/usr/bin/env python3
"""What the evaluation kernels achieve entry by entry on the cases of tests/test_gpu_eval_accuracy.py (three Huber widths,
the ragged task-edge scenes, the hard records alone and in a batch, f32 accumulation): one JSON line per case and
array, appended to profiles/eval_accuracy.jsonl -- the device's deviation from the longdouble reference (per entry,
relative to the entry's magnitude; tests/eval_cases.py) in the worst of the kernel configurations the test runs the case
in (elimination, two-pass or fused, group size), the deviations of the CPU references (A: the oracle's functor, B:
float64, F: float32 products) and the ratio to the bound the tests assert (8 x the references' larger deviation; the
tests fail above ratio 1).  Needs the GPU.

    python tools/eval_accuracy.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import eval_cases as ec  # noqa: E402
import test_gpu_eval_accuracy as T  # noqa: E402


def setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def g4(x):
    return float("%.4g" % x)


def records(part, name, case, results, bound=None):
    """One record per array: the worst of the kernel configurations in `results` ({configuration: run_blocks' result})."""
    bound = bound or case.bound
    worst = {}
    for conf, (b, _, c) in results.items():
        dev = ec.deviation(b, case.ref, case.mag)
        dev["cost()"] = ec.deviation(dict(b, cost=c), case.ref, case.mag)["cost"]
        for k, (d, zeros_ok) in dev.items():
            w = worst.setdefault(k, [-1.0, None, True])
            w[2] = w[2] and zeros_ok
            if d > w[0]:
                w[0], w[1] = d, conf
    for k, (d, conf, zeros_ok) in worst.items():
        kb = "cost" if k == "cost()" else k
        yield dict(part=part, case=name, array=k, configurations=len(results), worst=conf, deviation=g4(d),
                   zero_where_magnitude_is_zero=zeros_ok, bound=g4(bound[kb]),
                   reference_deviation={n: g4(r[kb][0]) for n, r in case.refs.items()},
                   ratio_to_bound=g4(d / bound[kb] if bound[kb] else float(d > 0)))


def all_records(eng, O):
    kats = ec.load_kats()
    four = [(elim, mode) for elim in ("cams", "tags") for mode in ("twopass", "fused")]
    for a in (0.5, 1.0, 2.5):
        for robust in (True, False):
            case = T.mixed_case(O, a, robust)
            yield from records("widths", "mixed a=%g robust=%d" % (a, robust), case, {
                "%s %s" % em: T.run_blocks(eng, setenv, case.scene, *em, robust=robust, a=a) for em in four})
    for few in ("tags", "cams"):
        for masked in (False, True):
            for const in (False, True):
                case = T.ragged_case(O, few, masked, const)
                res = {}
                for elim in ("cams", "tags"):
                    res.update(T.ragged_results(eng, setenv, case, elim))
                yield from records("task edges", "ragged few=%s mask=%d const=%d" % (few, masked, const), case, res)
    for i, rec in enumerate(kats["obs_hard"]):
        for robust in T._robust_settings(rec):
            case = T.record_case(O, kats, "obs_hard", i, robust)
            yield from records("hard record", "%s robust=%d" % (rec["what"], robust), case,
                               {"cams twopass": T.run_blocks(eng, setenv, case.scene, robust=robust)})
    for strong in (False, True):
        for robust in (True, False):
            case = T.hard_batch_case(O, kats, strong, robust)
            yield from records("hard batch", "hard batch strong=%d robust=%d" % (strong, robust), case, {
                "%s %s" % em: T.run_blocks(eng, setenv, case.scene, *em, robust=robust) for em in four})
    for label, case in T.f32_cases(O):
        yield from records("f32 accumulation", "f32 " + label, case, {
            "%s %s" % (elim, mode): T.run_blocks(eng, setenv, case.scene, elim, mode, group, a=case.a,
                                                 precision=eng.PRECISION_F32_ACCUM)
            for elim in ("cams", "tags") for mode, group in (("twopass", None), ("fused", 7))}, case.bound_f32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_accuracy.jsonl"))
    args = ap.parse_args()
    from oracle import oracle as O
    from visual_marker_mapping_amd import engine as eng
    O.build()
    worst = {}
    with open(args.out, "a") as f:
        for rec in all_records(eng, O):
            f.write(json.dumps(rec) + "\n")
            key = (rec["part"], rec["array"])
            worst[key] = max(worst.get(key, 0.0), rec["ratio_to_bound"])
    for (part, array), r in sorted(worst.items()):
        print("%-18s %-7s worst ratio to the bound %.3f" % (part, array, r))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
