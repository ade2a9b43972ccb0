"""One Levenberg-Marquardt iteration on the device against an extended-precision restatement, on every elimination path.

Whole solves are compared with the oracle on cost and radius per iteration; LM corrects itself, so a slightly wrong
Schur complement, damping or Jacobi scale reaches the same optimum through nearly the same costs.  Here ONE step is
pinned: the blocks of the start state (eval_blocks) are assembled into the full normal equations in numpy and the
step of oracle/vmm_oracle.c (vo_solve) is restated in np.longdouble (tests/linalg_cases.py: LmProblem,
lm_step_reference; checked against the oracle itself in tests/test_linalg_cases_cpu.py).  Every bound is 8 x the larger
deviation from that reference of two f64 numpy solves of the same step -- a plain Cholesky of the damped system and a
block elimination of the case's own family -- with the Plus KAT tolerance as the floor of the state.
"""
import numpy as np
import pytest

import linalg_cases as lc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", lc.LM_CASES, ids=lc.lm_case_id)
def test_one_lm_step_matches_the_extended_precision_restatement(monkeypatch, case):
    from visual_marker_mapping_amd import engine as eng

    def setenv(name, value):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)

    out, got, three, bound, extra = lc.run_lm_case(eng, case, setenv)
    trace, ref = out["trace"], three["ref"]
    dev = lc.lm_deviation(got, ref)
    for k in sorted(dev):
        print("%s: %s deviation %.3e, bound %.3e (ratio %.2f)" % (lc.lm_case_id(case), k, dev[k], bound[k],
                                                                  dev[k] / bound[k]))
    # the path the case names
    if "VMM_BA_SCHUR" in case["env"]:
        assert out["block_sparse"] == (1 if case["env"]["VMM_BA_SCHUR"] == "sparse" else 0)
    if "VMM_BA_ORDER" in case["env"]:
        assert (out["tree_ordering"] > 0) == (case["env"]["VMM_BA_ORDER"] == "nd"), out["tree_ordering"]
    assert out["elimination"] == (eng.ELIM_CAMERAS if case["elim"] == "cams" else eng.ELIM_TAGS)
    # a valid, successful step
    assert out["iterations"] == 2 and len(trace) == 2
    assert trace[1]["step_is_valid"] == 1 and trace[1]["step_is_successful"] == 1
    assert trace[0]["cost"] == pytest.approx(extra["start_cost"], rel=1e-14)
    # the step itself
    assert dev["state"] <= bound["state"]
    for k in lc.LM_SCALARS:
        assert dev[k] <= bound[k], k
    # constant poses have not moved at all
    s = extra["scene"]
    np.testing.assert_array_equal(got["tag"][extra["tag_const"]], s.tag_init[extra["tag_const"]])
    if extra["cam_const"] is not None:
        cc = extra["cam_const"].astype(bool)
        np.testing.assert_array_equal(got["cam"][cc], s.cam_init[cc])
    # identities between the device's own numbers
    assert trace[1]["cost"] == pytest.approx(extra["cost_after"], rel=1e-14)
    assert trace[1]["cost_change"] == trace[0]["cost"] - trace[1]["cost"]
    assert trace[1]["relative_decrease"] == pytest.approx(trace[1]["cost_change"] / trace[1]["model_cost_change"],
                                                          rel=1e-14)
