#!/usr/bin/env python3
"""Times the one-shot map initialisation (vmm_ba_initialize) and the closing sequence that follows it.

One JSON line per scene.  Every time is a host clock around calls that end in a device synchronisation; every scene
is run once untimed first (code-object load, graph capture) and then --reps times, and the line carries the median
with the minimum and maximum.  Lines:

  * "initialize": handle with placeholder poses -> initialize -> BA(1500, robust) -> BA(1500, plain), beside the same
    two solves from the scene generator's perturbed ground truth (iterations of both, for the quality of the start);
  * "driver" (--driver): TagReconstructor.startReconstructionGlobal against startReconstruction on the scene of
    `bench.py --workload incremental`, alternating, whole wall time of each (host PnP and prunings included).

Needs an MI355X; there is no CPU fallback.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCENES = {
    "20x10": (1, {}),
    "100x60_vis0.30": (1, dict(n_cams=100, n_tags=60, visibility=0.30)),
    "bench_incremental_100x60": (2, dict(n_cams=100, n_tags=60, visibility=0.30)),
    "closeup_60x80": (2, dict(n_cams=60, n_tags=80, neighbors_min=6, neighbors_max=10)),
    "config5_30x40": (5, dict(n_cams=30, n_tags=40, visibility=0.5)),
    "small_tags_30x200": (2, dict(n_cams=30, n_tags=200, visibility=0.4)),
    "500x200": (2, dict(n_cams=500, n_tags=200)),
}


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def _placeholders(s):
    cam = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 1.0]), (len(s.cam_gt), 1))
    tag = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0.0]), (len(s.tag_gt), 1))
    tag[s.fixed_tag] = s.tag_gt[s.fixed_tag]
    return cam, tag


def _closing(eng, ba):
    t0 = time.perf_counter()
    a = ba.solve(eng.default_options(robustify=1, max_num_iterations=1500))
    b = ba.solve(eng.default_options(robustify=0, max_num_iterations=1500))
    return time.perf_counter() - t0, a, b


def bench_initialize(name, reps, sweeps):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = SCENES[name]
    s = make_scene(cfg, **kw)
    cam0, tag0 = _placeholders(s)
    t_init, t_init_lib, t_close, t_close_ref = [], [], [], []
    with eng.BundleAdjuster(s.intr, s.dist, cam0, tag0, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px) as ba:
        for rep in range(reps + 1):
            ba.set_state(cam0, tag0)
            t0 = time.perf_counter()
            report, cam_ok, tag_ok = ba.initialize(sweeps=sweeps)
            dt = time.perf_counter() - t0
            dc, a, b = _closing(eng, ba)
            ba.set_state(s.cam_init, s.tag_init)
            dr, ar, br = _closing(eng, ba)
            if rep:   # the first pass is the warm-up
                t_init.append(dt)
                t_init_lib.append(report["time_s"])
                t_close.append(dc)
                t_close_ref.append(dr)
    print(json.dumps({
        "metric": "global_init", "scene": name, "cams": len(s.cam_gt), "tags": len(s.tag_gt), "observations": s.n_obs,
        "sweeps": sweeps, "reps": reps, "rounds": report["rounds"], "cams_reached": report["cams_reached"],
        "tags_reached": report["tags_reached"], "avg_reprojection_px_after_initialize": report["avg_reprojection_px"],
        "initialize_s": _spread(t_init), "initialize_library_s": _spread(t_init_lib),
        "closing_sequence_s": _spread(t_close), "closing_sequence_from_perturbed_truth_s": _spread(t_close_ref),
        "robust_iterations": a["iterations"], "plain_iterations": b["iterations"],
        "robust_iterations_from_perturbed_truth": ar["iterations"],
        "plain_iterations_from_perturbed_truth": br["iterations"],
        "final_cost": b["final_cost"], "final_cost_from_perturbed_truth": br["final_cost"],
        "termination": [a["termination_type"], b["termination_type"]], "unit": "s", "dtype": "f64", "data": "synthetic"}))


def bench_driver(reps):
    from visual_marker_mapping_amd.synthetic import make_scene
    from visual_marker_mapping_amd.tag_reconstructor import CameraModel, TagReconstructor, detection_result_from_arrays
    n_cams, n_tags, vis = 100, 60, 0.3           # the scene of bench.py --workload incremental
    s = make_scene(2, n_cams=n_cams, n_tags=n_tags, visibility=vis)
    times = {"global": [], "incremental": []}
    info = {}
    for rep in range(reps + 1):
        for mode in ("global", "incremental"):    # alternating; the first pass is the warm-up
            det = detection_result_from_arrays(s.obs_cam, s.obs_tag, s.obs_px, s.tag_wh, n_cams)
            rec = TagReconstructor(det)
            rec.setCameraModel(CameraModel(*[float(v) for v in s.intr], s.dist, 4000, 6000))
            buf = io.StringIO()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(buf):
                if mode == "global":
                    rec.startReconstructionGlobal(1)
                else:
                    rec.startReconstruction(1, deviceResident=True)
            dt = time.perf_counter() - t0
            if rep:
                times[mode].append(dt)
            info[mode] = dict(bundle_adjustments=buf.getvalue().count("Solution "), cameras=len(rec.reconstructedCameras),
                              tags=len(rec.reconstructedTags), final_cost=rec.lastSummary["final_cost"],
                              last_iterations=rec.lastSummary["iterations"])
            if mode == "global":
                info[mode]["initialize"] = rec.lastInitReport
            rec.close()
    print(json.dumps({
        "metric": "global_vs_incremental_driver", "scene": "bench_incremental_100x60", "cams": n_cams, "tags": n_tags,
        "observations": s.n_obs, "reps": reps, "start_reconstruction_global_s": _spread(times["global"]),
        "start_reconstruction_s": _spread(times["incremental"]), "global": info["global"],
        "incremental": info["incremental"],
        "relative_final_cost_difference": abs(info["global"]["final_cost"] - info["incremental"]["final_cost"])
        / info["incremental"]["final_cost"], "unit": "s", "dtype": "f64", "data": "synthetic"}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="100x60_vis0.30,bench_incremental_100x60,500x200",
                    help="comma-separated names out of: %s; 'all'" % ", ".join(SCENES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", default="1", help="comma-separated values of vmm_ba_init_options.sweeps, a line for each")
    ap.add_argument("--driver", action="store_true", help="also time startReconstructionGlobal against startReconstruction")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_global_init.py needs an MI355X: no GPU visible")
    names = list(SCENES) if a.scenes == "all" else [n for n in a.scenes.split(",") if n]
    for n in names:
        if n not in SCENES:
            raise SystemExit("unknown scene %r" % n)
    for n in names:
        for sw in a.sweeps.split(","):
            bench_initialize(n, a.reps, int(sw))
    if a.driver:
        bench_driver(a.reps)


if __name__ == "__main__":
    main()
