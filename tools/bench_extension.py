#!/usr/bin/env python3
"""Times TagReconstructor.extendReconstruction beside startReconstructionGlobal on the same images.

The scene is split as tests/test_gpu_constant_poses.py splits it: tags [0, n_tags / 2) are the finished map at ground
truth, the new images are the cameras that see a map tag.  extendReconstruction gets the map and the new images'
detections; startReconstructionGlobal gets the same detections and no map (it rebuilds everything the images see, in its
own coordinate frame).  Whole wall time of each on the host clock, prunings and packing included, alternating; the first
pass is the warm-up; one JSON line with the median, minimum and maximum.  --once: a single extension run and nothing
else (the run to put under rocprofv3 --kernel-trace --stats).

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
    "closeup_60x80": (2, dict(n_cams=60, n_tags=80, neighbors_min=6, neighbors_max=10)),
    "100x60_vis0.30": (1, dict(n_cams=100, n_tags=60, visibility=0.30)),
}


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def _split(s):
    from visual_marker_mapping_amd.tag_reconstructor import ReconstructedTag, detection_result_from_arrays
    n_t = len(s.tag_gt)
    map_tags = np.arange(n_t) < n_t // 2
    new_images = np.unique(s.obs_cam[map_tags[s.obs_tag]])
    keep = np.isin(s.obs_cam, new_images)
    det = detection_result_from_arrays(np.searchsorted(new_images, s.obs_cam[keep]), s.obs_tag[keep], s.obs_px[keep],
                                       s.tag_wh, len(new_images))
    tags = {int(t): ReconstructedTag(int(t), "apriltag_36h11", s.tag_gt[t, :4], s.tag_gt[t, 4:], s.tag_wh[t, 0],
                                     s.tag_wh[t, 1]) for t in np.flatnonzero(map_tags)}
    return det, tags, int(keep.sum())


def _run(s, mode):
    from visual_marker_mapping_amd.tag_reconstructor import CameraModel, TagReconstructor
    det, tags, _ = _split(s)
    rec = TagReconstructor(det)
    rec.setCameraModel(CameraModel(*[float(v) for v in s.intr], s.dist, 4000, 6000))
    buf = io.StringIO()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(buf):
        if mode == "extend":
            rec.setReconstructedTags(tags)
            rec.extendReconstruction(1)
        else:
            rec.startReconstructionGlobal(1)
    dt = time.perf_counter() - t0
    info = dict(cameras=len(rec.reconstructedCameras), tags=len(rec.reconstructedTags),
                final_cost=rec.lastSummary["final_cost"], last_iterations=rec.lastSummary["iterations"],
                initialize=rec.lastInitReport)
    rec.close()
    return dt, info


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="closeup_60x80", choices=sorted(SCENES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="one extension run, no timing line")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_extension.py needs an MI355X: no GPU visible")
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = SCENES[a.scene]
    s = make_scene(cfg, **kw)
    if a.once:
        _run(s, "extend")
        return
    times, info = {"extend": [], "global": []}, {}
    for rep in range(a.reps + 1):
        for mode in ("extend", "global"):
            dt, info[mode] = _run(s, mode)
            if rep:
                times[mode].append(dt)
    det, tags, n_obs = _split(s)
    print(json.dumps({
        "metric": "extend_vs_global_driver", "scene": a.scene, "new_images": len(det.images), "map_tags": len(tags),
        "tags_in_scene": len(s.tag_gt), "observations": n_obs, "reps": a.reps,
        "extend_reconstruction_s": _spread(times["extend"]), "start_reconstruction_global_s": _spread(times["global"]),
        "extend": info["extend"], "global": info["global"], "unit": "s", "dtype": "f64", "data": "synthetic"}))


if __name__ == "__main__":
    main()
