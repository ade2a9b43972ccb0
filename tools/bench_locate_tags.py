#!/usr/bin/env python3
"""Times the location of tags from known cameras (vmm_ba_locate_tags).

One JSON line per scene.  The cameras are the scene's ground truth with a covariance each (so the propagation runs), the
detections carry the generator's default noise.  "call_ms": engine.locate_tags on the whole batch -- a host clock around
a call that ends in blocking copies back, so upload, the three kernels and download are all inside; run once untimed
first (code-object load), then --reps times: median with minimum and maximum, tags per second from the median.  No time
is gated: the entry has no predecessor to compare with.

--kernels-only runs each scene's device call once after a warm-up and nothing else: the process to put under
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCENES = {
    "100x60_vis0.30": (1, dict(n_cams=100, n_tags=60, visibility=0.30)),
    "500x200": (2, dict(n_cams=500, n_tags=200)),
}


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def _csr(s):
    start = np.zeros(len(s.tag_gt) + 1, np.int64)
    start[1:] = np.cumsum(np.bincount(s.obs_tag, minlength=len(s.tag_gt)))
    order = np.lexsort((s.obs_cam, s.obs_tag))
    return start, s.obs_cam[order].astype(np.int32), s.obs_px[order].copy()


def _gap(a, b):
    qa, qb = a[:4] / np.linalg.norm(a[:4]), b[:4] / np.linalg.norm(b[:4])
    return (float(np.linalg.norm(qa * np.sign(qa @ qb) - qb)),
            float(np.linalg.norm(a[4:] - b[4:]) / max(np.linalg.norm(b[4:]), 1.0)))


def bench(name, reps, kernels_only):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = SCENES[name]
    s = make_scene(cfg, **kw)
    start, cam, px = _csr(s)
    cam_cov = np.tile(np.eye(6) * 1e-8, (len(s.cam_gt), 1, 1))
    call = lambda: eng.locate_tags(s.intr, s.dist, s.cam_gt, s.tag_wh, start, cam, px, cam_cov=cam_cov)
    tag, cov, cams, inl, res = call()   # warm-up
    if kernels_only:
        call()
        return
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    seen = [t for t in range(len(tag)) if res[t]["status"] == 0]
    gq, gt = zip(*[_gap(tag[t], s.tag_gt[t]) for t in seen])
    line = {"metric": "locate_tags", "scene": name, "cameras": len(s.cam_gt), "tags": len(tag), "observations": len(cam),
            "longest_tag": int(np.diff(start).max()), "reps": reps, "call_ms": _spread([1e3 * t for t in times]),
            "tags_per_s": len(tag) / statistics.median(times), "status_ok": len(seen),
            "inlier_observations": int(inl.sum()), "trials": _spread([r["trials"] for r in res]),
            "rms_px_median": statistics.median(r["rms_px"] for r in res),
            "max_gap_to_ground_truth": {"dq": max(gq), "dt": max(gt)},
            "unit": "ms", "dtype": "f64", "data": "synthetic"}
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="100x60_vis0.30,500x200", help="comma-separated names out of: %s" % ", ".join(SCENES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="one device call per scene after a warm-up, no timing")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_locate_tags.py needs an MI355X: no GPU visible")
    names = [n for n in a.scenes.split(",") if n]
    for n in names:
        if n not in SCENES:
            raise SystemExit("unknown scene %r" % n)
    for n in names:
        bench(n, a.reps, kernels_only=a.kernels_only)


if __name__ == "__main__":
    main()
