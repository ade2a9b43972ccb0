#!/usr/bin/env python3
"""Times the bundle adjustment that refines the camera model (vmm_ba_intrinsics_system, vmm_ba_solve_selfcal).

One JSON line per scene.  The handle starts at the scene's true poses; the camera model starts off the truth by --perturb
times (+200, -150, +30, -25, +0.02, -0.05, +1e-3, -1e-3, +0.02), the start of the tests.  Host clocks around calls that
end in a blocking copy back; every call runs once untimed first (code-object load, graph capture), then --reps times:
median with minimum and maximum.
  system_ms        one vmm_ba_intrinsics_system, beside covariance_ms: vmm_ba_covariance_blocks for one pair on the same
                   handle -- the two share the preamble (evaluation, elimination, rank-k update, factorisation)
  selfcal_ms       vmm_ba_solve_selfcal from the perturbed start (state and model reset before every repetition), beside
                   solve_ms: a plain vmm_ba_solve from the same start with the perturbed model held; with the outer and
                   inner iteration counts of both
  recapture_ms     what capturing the iteration graph again costs: a solve of zero iterations behind vmm_ba_set_intrinsics
                   minus one that finds its graph; recapture_share = that times the captures of one selfcal call (one per
                   trial, one more behind every rejected trial) over selfcal_ms

Needs an MI355X; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCENES = {
    "20x10": (1, dict()),
    "500x200": (2, dict(n_cams=500, n_tags=200)),
}
PERTURB = np.array([200.0, -150.0, 30.0, -25.0, 0.02, -0.05, 1e-3, -1e-3, 0.02])


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def _timed(call, reps, before=None):
    out = []
    for _ in range(reps + 1):   # the first one is the warm-up
        if before:
            before()
        t0 = time.perf_counter()
        res = call()
        out.append(1e3 * (time.perf_counter() - t0))
    return out[1:], res


def bench(name, reps, perturb, robust, device_name):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = SCENES[name]
    s = make_scene(cfg, **kw)
    truth = np.concatenate([s.intr, s.dist])
    k0 = truth + perturb * PERTURB
    ba = eng.BundleAdjuster(k0[:4], k0[4:], s.cam_gt, s.tag_gt, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px)
    # the inner solves as TagReconstructor.doBundleAdjustment(refineCameraModel=True) runs them; the plain solve alike
    opts = eng.default_options(robustify=int(robust), function_tolerance=1e-14, parameter_tolerance=1e-12)

    def reset():
        ba.set_state(s.cam_gt, s.tag_gt)
        ba.set_intrinsics(k0[:4], k0[4:])

    t_sys, _ = _timed(lambda: ba.intrinsics_system(robustify=robust), reps)
    t_cov, _ = _timed(lambda: ba.covariance_blocks([[0, 0]], robustify=robust), reps)
    t_solve, plain = _timed(lambda: ba.solve(opts), reps, before=lambda: ba.set_state(s.cam_gt, s.tag_gt))
    zero = eng.default_options(robustify=int(robust), max_num_iterations=0)
    t_keep, _ = _timed(lambda: ba.solve(zero), reps, before=lambda: ba.set_state(s.cam_gt, s.tag_gt))
    t_drop, _ = _timed(lambda: ba.solve(zero), reps, before=reset)
    t_self, (intr, dist, cov, rep, inner) = _timed(lambda: ba.solve_selfcal(opts), reps, before=reset)
    ba.close()
    k = np.concatenate([intr, dist])
    recapture = statistics.median(t_drop) - statistics.median(t_keep)
    captures = rep["outer_iterations"] + (rep["outer_iterations"] - rep["accepted"])
    line = {"metric": "selfcal", "device": device_name, "scene": name, "cameras": len(s.cam_gt), "tags": len(s.tag_gt),
            "observations": len(s.obs_cam), "reps": reps, "perturb": perturb, "robustify": int(robust),
            "system_ms": _spread(t_sys), "covariance_ms": _spread(t_cov),
            "selfcal_ms": _spread(t_self), "solve_ms": _spread(t_solve),
            "selfcal": {"status": rep["status"], "outer_iterations": rep["outer_iterations"], "accepted": rep["accepted"],
                        "inner_lm_iterations": rep["inner_lm_iterations"], "initial_cost": rep["initial_cost"],
                        "final_cost": rep["final_cost"]},
            "solve": {"iterations": plain["iterations"], "num_lm_iterations": plain["num_lm_iterations"],
                      "final_cost": plain["final_cost"]},
            "recapture_ms": recapture, "captures_per_call": captures,
            "recapture_share": captures * recapture / statistics.median(t_self),
            "error_to_truth_rel": (np.abs(k - truth) / np.maximum(np.abs(truth), 1.0)).tolist(),
            "sigma": np.sqrt(np.diag(cov)).tolist(), "unit": "ms", "dtype": "f64", "data": "synthetic"}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="20x10,500x200", help="comma-separated names out of: %s" % ", ".join(SCENES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--perturb", type=float, default=1.0, help="multiple of the start perturbation")
    ap.add_argument("--plain", action="store_true", help="no Huber loss (default: robust, as the mapping step's adjustments)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_selfcal.py needs an MI355X: no GPU visible")
    names = [n for n in a.scenes.split(",") if n]
    for n in names:
        if n not in SCENES:
            raise SystemExit("unknown scene %r" % n)
    for n in names:
        bench(n, a.reps, a.perturb, not a.plain, torch.cuda.get_device_name(0))


if __name__ == "__main__":
    main()
