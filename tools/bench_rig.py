#!/usr/bin/env python3
"""Times the localisation and the calibration of a three-camera rig against a finished map (vmm_ba_rig_localize,
vmm_ba_rig_calibrate) beside the per-image localisation of the same images (vmm_ba_localize, one call per camera).

One JSON line per scene, printed and appended to --output (default profiles/rig.jsonl).  The map is the scene's ground
truth, the extrinsics are yaw 0 / 4 / -15 degrees with baselines of 0.3 and 0.2 m, the pixels carry the generator's
default noise.  Each figure is a host clock around a call that ends in blocking copies back, so uploads, kernels and
downloads are all inside; one untimed call first (code-object load), then --reps: median with minimum and maximum,
frames per second from the median.  "gap": the largest distance between the rig poses and the ground truth, for scale.
The calibration starts from the true extrinsics (so it measures the refinement near its optimum: the localisation, the
trial loop with one small copy back per trial, three passes, the covariances) with the default mask.

Needs an MI355X; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {
    "20x10": (1, dict()),
    "closeup_60x80": (2, dict(n_cams=60, n_tags=80, neighbors_min=6, neighbors_max=10)),
    "500x200": (2, dict(n_cams=500, n_tags=200)),
}


def _yaw(deg, t):
    a = np.radians(deg) / 2
    return [np.cos(a), 0.0, np.sin(a), 0.0, t[0], t[1], t[2]]


EXT = np.array([_yaw(0.0, (0, 0, 0)), _yaw(4.0, (-0.3, 0, 0)), _yaw(-15.0, (0.2, 0.05, 0))])


def _timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return {"median": statistics.median(out), "min": min(out), "max": max(out)}


def main(argv=None):
    from visual_marker_mapping_amd import _lib, engine as eng
    from visual_marker_mapping_amd.synthetic import make_rig_scene
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", nargs="*", default=["20x10", "closeup_60x80"], choices=sorted(SCENES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "rig.jsonl"))
    a = ap.parse_args(argv)
    for name in a.scenes:
        cfg, kw = SCENES[name]
        s = make_rig_scene(cfg, EXT, seed=1, **kw)
        K, F = s.n_rig_cams, s.n_frames
        rig = lambda: eng.rig_localize(s.intr, s.dist, s.ext_qt, s.tag_gt, s.tag_wh, s.img_start, s.obs_tag, s.obs_px)
        per_cam = []
        for c in range(K):
            own = np.arange(F) * K + c
            idx = np.concatenate([np.arange(s.img_start[i], s.img_start[i + 1]) for i in own]).astype(np.int64)
            start = np.zeros(F + 1, np.int64)
            start[1:] = np.cumsum(np.diff(s.img_start)[own])
            per_cam.append((s.intr[c], s.dist[c], s.tag_gt, s.tag_wh, start, s.obs_tag[idx], s.obs_px[idx]))
        images = lambda: [eng.localize(*args) for args in per_cam]
        cal = lambda: eng.rig_calibrate(s.intr, s.dist, s.ext_qt, s.tag_gt, s.tag_wh, s.img_start, s.obs_tag, s.obs_px)
        t_rig, t_img, t_cal = _timed(rig, a.reps), _timed(images, a.reps), _timed(cal, a.reps)
        report = cal()[6]
        rig_qt, _, inl, res = rig()
        gap = float(max(np.abs(rig_qt[:, 4:] - s.rig_gt[:, 4:]).max(),
                        np.abs(np.abs(np.sum(rig_qt[:, :4] * s.rig_gt[:, :4], axis=1)) - 1.0).max()))
        line = {"scene": name, "rig_cams": K, "frames": F, "observations": int(len(s.obs_tag)),
                "rig_localize_s": t_rig, "frames_per_s": F / t_rig["median"], "localize_per_camera_s": t_img,
                "rig_calibrate_s": t_cal, "calibrate_trials": report["trials"],
                "calibrate_status": _lib.CAL_STATUS_NAMES[report["status"]], "calibrate_rms_px": report["final_rms_px"],
                "frames_ok": int(sum(r["status"] == _lib.LOC_OK for r in res)), "inliers": int(inl.sum()), "gap": gap}
        print(json.dumps(line))
        os.makedirs(os.path.dirname(a.output), exist_ok=True)
        with open(a.output, "a") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
