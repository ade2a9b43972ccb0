#!/usr/bin/env python3
"""Times the prediction of the localisation accuracy over a survey of hypothetical poses (vmm_ba_predict_localization).

One JSON line per case, printed and appended to --output (default profiles/coverage_speed.jsonl).  The map is a scene's
ground-truth tags, the poses a grid over the box of the scene's camera centres (engine.grid_poses) with eight optical
axes around the cameras' mean axis; the image is 6000 x 4000 like synthetic.write_project's camera model.
  500x200_grid131072          the 200 tags of the 500 x 200 scene against 64 x 64 x 4 nodes x 8 axes, without tag_cov
  500x200_grid131072_tag_cov  the same with a covariance on every tag but the origin (k_predict<true>)
  100x60_grid16384            the 60 tags of the 100 x 60 scene against 32 x 32 x 2 nodes x 8 axes, with tag_cov
  500x200_grid131072_joint    the 500x200_grid131072_tag_cov survey with the tags' joint covariance (k_predict_joint): the
  100x60_grid16384_joint      same scene, poses and visible sets; the covariance is BundleAdjuster.tag_joint_covariance on
                              the scene at its ground truth.  These lines go to profiles/coverage_joint_speed.jsonl and
                              also say the mean and the largest number of visible tags per pose, which set the pair work;
                              the yardstick is the _tag_cov row of the same session.
"call_ms": engine.predict_localization on the whole batch with both covariances, the records and the visible bytes asked
for -- a host clock around a call that ends in blocking copies back, so upload, the four kernels and download are all
inside; run once untimed first (code-object load), then --reps times: median with minimum and maximum, poses per second
from the median.  No time is gated: the entry has no predecessor to compare with.  "host_model_ms_per_pose": the numpy
host model of the tests (tests/predict_cases.py) on --host-poses of the poses, for scale only.

--kernels-only runs each case's device call once after a warm-up and nothing else: the process to put under
`rocprofv3 --kernel-trace --stats` for per-kernel times.

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
sys.path.insert(0, os.path.join(ROOT, "tests"))

IMAGE = (6000, 4000)
CASES = {
    "500x200_grid131072": ((2, dict(n_cams=500, n_tags=200)), (64, 64, 4), False),
    "500x200_grid131072_tag_cov": ((2, dict(n_cams=500, n_tags=200)), (64, 64, 4), True),
    "100x60_grid16384": ((1, dict(n_cams=100, n_tags=60, visibility=0.30)), (32, 32, 2), True),
    "500x200_grid131072_joint": ((2, dict(n_cams=500, n_tags=200)), (64, 64, 4), "joint"),
    "100x60_grid16384_joint": ((1, dict(n_cams=100, n_tags=60, visibility=0.30)), (32, 32, 2), "joint"),
}
JOINT_OUTPUT = os.path.join(ROOT, "profiles", "coverage_joint_speed.jsonl")


def joint_covariance(s):
    """The tags' joint covariance of the scene's bundle adjustment at its ground truth."""
    from visual_marker_mapping_amd import engine as eng
    ba = eng.BundleAdjuster(s.intr, s.dist, s.cam_gt, s.tag_gt, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px, device=0)
    joint = ba.tag_joint_covariance()
    ba.close()
    return joint


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def survey(s, shape):
    """The grid over the box of the scene's camera centres, eight axes 15 degrees around the cameras' mean optical axis."""
    import predict_cases as pc
    import yardstick as ys
    from visual_marker_mapping_amd import engine as eng
    centres = np.array([pc.camera_centre(q) for q in s.cam_gt])
    mean = np.mean([ys.rotation(q)[2] for q in s.cam_gt], axis=0)
    mean /= np.linalg.norm(mean)
    up = np.eye(3)[int(np.argmin(np.abs(mean)))]
    e1 = np.cross(mean, up)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(mean, e1)
    tilt = np.tan(np.radians(15.0))
    axes = [mean + tilt * (i * e1 + j * e2) for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0)]
    return eng.grid_poses(centres.min(axis=0), centres.max(axis=0), shape, axes, up)


def bench(name, reps, host_poses, kernels_only):
    import predict_cases as pc
    from oracle import oracle as O
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    (cfg, kw), shape, with_cov = CASES[name]
    s = make_scene(cfg, **kw)
    poses = survey(s, shape)
    if with_cov == "joint":
        joint = joint_covariance(s)
        call = lambda: eng.predict_localization(s.intr, s.dist, s.tag_gt, s.tag_wh, poses, IMAGE, tag_cov_joint=joint, want_visible=True)
        cov_px, cov_map, res, vis = call()   # warm-up
        if kernels_only:
            call()
            return None
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
        ok = np.array([r["status"] == 0 for r in res])
        sig = np.array([r["sigma_pos_m"] for r in res])[ok]
        v = vis.sum(axis=1)
        return {"metric": "coverage", "case": name, "tags": len(s.tag_gt), "poses": len(poses), "tag_cov": "joint", "reps": reps,
                "call_ms": _spread([1e3 * t for t in times]), "poses_per_s": len(poses) / statistics.median(times),
                "status_ok": int(ok.sum()), "visible_pairs": int(vis.sum()), "visible_per_pose_mean": float(v.mean()),
                "visible_per_pose_max": int(v.max()), "pair_terms": int((v * (v + 1) // 2).sum()),
                "sigma_pos_m_median": float(np.median(sig)) if len(sig) else None, "joint_covariance_bytes": int(joint.nbytes),
                "unit": "ms", "dtype": "f64", "data": "synthetic"}
    tag_cov = pc.random_tag_cov(len(s.tag_gt), fixed=s.fixed_tag) if with_cov else None
    call = lambda: eng.predict_localization(s.intr, s.dist, s.tag_gt, s.tag_wh, poses, IMAGE, tag_cov=tag_cov, want_visible=True)
    cov_px, cov_map, res, vis = call()   # warm-up
    if kernels_only:
        call()
        return None
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    ok = np.array([r["status"] == 0 for r in res])
    sig = np.array([r["sigma_pos_m"] for r in res])[ok]
    # the host model of the tests on a sample, for scale only
    O.build()
    sample = np.linspace(0, len(poses) - 1, min(host_poses, len(poses))).astype(int)
    case = dict(intr=s.intr, dist=s.dist, size=IMAGE, tag_qt=s.tag_gt, tag_wh=s.tag_wh, cam_qt=poses[sample])
    t0 = time.perf_counter()
    host_vis, _ = pc.host_visible(case)
    for p in range(len(sample)):
        if host_vis[p].any():
            pc.host_pose(O, case, p, host_vis[p], tag_cov=tag_cov)
    host_s = time.perf_counter() - t0
    return {"metric": "coverage", "case": name, "tags": len(s.tag_gt), "poses": len(poses), "tag_cov": with_cov, "reps": reps,
            "call_ms": _spread([1e3 * t for t in times]), "poses_per_s": len(poses) / statistics.median(times),
            "status_ok": int(ok.sum()), "visible_pairs": int(vis.sum()), "tags_never_seen": int((vis.sum(axis=0) == 0).sum()),
            "visible_per_pose_mean": float(vis.sum(axis=1).mean()), "visible_per_pose_max": int(vis.sum(axis=1).max()),
            "sigma_pos_m_median": float(np.median(sig)) if len(sig) else None,
            "host_model_poses": len(sample), "host_model_ms_per_pose": 1e3 * host_s / len(sample),
            "host_model_flags_differing": int((host_vis != vis[sample]).sum()),
            "unit": "ms", "dtype": "f64", "data": "synthetic"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default=",".join(n for n in CASES if not n.endswith("_joint")),
                    help="comma-separated names out of: %s" % ", ".join(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-poses", type=int, default=256, help="poses the numpy host model is timed on")
    ap.add_argument("--kernels-only", action="store_true", help="one device call per case after a warm-up, no timing")
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "coverage_speed.jsonl"))
    ap.add_argument("--joint-output", default=JOINT_OUTPUT, help="where the lines of the _joint cases go")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_coverage.py needs an MI355X: no GPU visible")
    names = [n for n in a.cases.split(",") if n]
    for n in names:
        if n not in CASES:
            raise SystemExit("unknown case %r" % n)
    for n in names:
        line = bench(n, a.reps, a.host_poses, a.kernels_only)
        if line is not None:
            print(json.dumps(line), flush=True)
            with open(a.joint_output if n.endswith("_joint") else a.output, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
