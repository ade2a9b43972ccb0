#!/usr/bin/env python3
"""What the linear-algebra kernels achieve on the accuracy cases of tests/test_gpu_linear_accuracy.py (every factorisation
path, the boundary orders, scaling by powers of two) and tests/test_gpu_lm_step.py (one LM iteration per elimination
path): one JSON line per case, appended to profiles/linear_accuracy.jsonl -- the case, the kernel's backward and forward
error, the two CPU references' errors and the ratio to the bound the tests assert (8 x the references' error; the tests
fail above ratio 1).  Needs the GPU.

    python tools/linear_accuracy.py [--out FILE] [--skip-lm]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import linalg_cases as lc  # noqa: E402


def solve_record(eng, part, c, A, b, unscale=None, **what):
    x, info = eng.dense_spd_solve(A, b)
    if unscale is not None:
        x = np.ldexp(x, unscale)
    be = lc.backward_error(c["A"], c["b"], x, c["norm_A"], c["A_ld"])
    fe = lc.forward_error(x, c["x_ref"])
    rec = dict(part=part, n=c["n"], kappa=c["kappa"], info=info, backward=be, forward=fe,
               reference_backward={k: r["backward"] for k, r in c["refs"].items()},
               reference_forward={k: r["forward"] for k, r in c["refs"].items()},
               backward_ratio_to_bound=be / (lc.MARGIN * c["bound"]) if c["bound"] else float(be > 0),
               forward_ratio_to_bound=fe / (lc.MARGIN * c["forward_bound"]) if c["forward_bound"] else float(fe > 0))
    rec.update(what)
    return rec, x


def linear_records(eng):
    for n, kappa in lc.PATH_CASES:
        c = lc.case_bounds(n, kappa, 0)
        yield solve_record(eng, "3a path", c, c["A"], c["b"], path="default")[0]
    for env, n, kappa in lc.FALLBACK_CASES:
        c = lc.case_bounds(n, kappa, 0)
        os.environ[env] = "1"
        try:
            yield solve_record(eng, "3a fallback", c, c["A"], c["b"], path=env + "=1")[0]
        finally:
            del os.environ[env]
    for n in lc.BOUNDARY_ORDERS:
        c = lc.case_bounds(n, lc.BOUNDARY_KAPPA, 0)
        yield solve_record(eng, "3b boundary order", c, c["A"], c["b"])[0]
    for n, kappa in lc.SCALING_CASES:
        c = lc.case_bounds(n, kappa, 0)
        _, x = solve_record(eng, "3c", c, c["A"], c["b"])
        e = np.random.default_rng(n).integers(-40, 41, n)
        rec, xs = solve_record(eng, "3c scaling", c, np.ldexp(np.ldexp(c["A"], e[:, None]), e[None, :]),
                               np.ldexp(c["b"], e), unscale=e, scaling="D A D, D = diag(2^e), e in [-40, 40]")
        rec["same_bits_as_unscaled"] = bool(np.array_equal(xs, x))
        yield rec
        for p in (400, -400):
            rec, xs = solve_record(eng, "3c scaling", c, np.ldexp(c["A"], p), np.ldexp(c["b"], p),
                                   scaling="A 2^%d, b 2^%d" % (p, p))
            rec["same_bits_as_unscaled"] = bool(np.array_equal(xs, x))
            yield rec


def lm_records(eng):
    def setenv(name, value):
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value

    for case in lc.LM_CASES:
        out, got, three, bound, _ = lc.run_lm_case(eng, case, setenv)
        dev = lc.lm_deviation(got, three["ref"])
        refs = {k: lc.lm_deviation(three[k], three["ref"]) for k in ("cholesky", "schur")}
        yield dict(part="4 lm step", case=lc.lm_case_id(case), block_sparse=out["block_sparse"],
                   tree_ordering=out["tree_ordering"], step_is_successful=out["trace"][1]["step_is_successful"],
                   deviation=dev, reference_deviation=refs, bound=bound,
                   ratio_to_bound={k: dev[k] / bound[k] if bound[k] else float(dev[k] > 0) for k in dev})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_accuracy.jsonl"))
    ap.add_argument("--skip-lm", action="store_true")
    args = ap.parse_args()
    from visual_marker_mapping_amd import engine as eng
    with open(args.out, "a") as f:
        for rec in linear_records(eng):
            f.write(json.dumps(rec) + "\n")
            f.flush()
        if not args.skip_lm:
            for rec in lm_records(eng):
                f.write(json.dumps(rec) + "\n")
                f.flush()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
