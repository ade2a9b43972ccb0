#!/usr/bin/env python3
"""Times the localisation of images against a finished map (vmm_ba_localize) beside the host path.

One JSON line per scene.  The map is the scene's ground truth, the detections carry the generator's default noise.
"device": engine.localize on the whole batch -- a host clock around a call that ends in blocking copies back, so
upload, the three kernels and download are all inside; run once untimed first (code-object load), then --reps times:
median with minimum and maximum, images per second from the median.  "host": a loop over
TagReconstructor.computeRelativeCameraPoseFromImg (pnp.solvePnPRansac, one image at a time) over --host-images
evenly spaced images, seconds per image, and its pose gap to the device result.

--kernels-only runs each scene's device call once after a warm-up and nothing else: the process to put under
`rocprofv3 --kernel-trace --stats` for per-kernel times.

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
    "100x60_vis0.30": (1, dict(n_cams=100, n_tags=60, visibility=0.30)),
    "500x200": (2, dict(n_cams=500, n_tags=200)),
    "closeup_2000": (2, dict(n_cams=2000, n_tags=1000, neighbors_min=6, neighbors_max=10)),
}


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def _csr(s):
    start, order = s.by_image()
    return start, s.obs_tag[order].astype(np.int32), s.obs_px[order].copy()


def _gap(a, b):
    qa, qb = a[:4] / np.linalg.norm(a[:4]), b[:4] / np.linalg.norm(b[:4])
    return (float(np.linalg.norm(qa * np.sign(qa @ qb) - qb)),
            float(np.linalg.norm(a[4:] - b[4:]) / max(np.linalg.norm(b[4:]), 1.0)))


def bench(name, reps, host_images, kernels_only):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    from visual_marker_mapping_amd.tag_reconstructor import (CameraModel, ReconstructedTag, TagReconstructor,
                                                             detection_result_from_arrays)
    cfg, kw = SCENES[name]
    s = make_scene(cfg, **kw)
    start, tag, px = _csr(s)
    call = lambda: eng.localize(s.intr, s.dist, s.tag_gt, s.tag_wh, start, tag, px)
    cam, cov, inl, res = call()   # warm-up
    if kernels_only:
        call()
        return
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    gq, gt = zip(*[_gap(cam[i], s.cam_gt[i]) for i in range(len(cam))])
    line = {"metric": "localize", "scene": name, "images": len(cam), "tags": len(s.tag_gt), "observations": len(tag),
            "reps": reps, "call_ms": _spread([1e3 * t for t in times]),
            "images_per_s": len(cam) / statistics.median(times),
            "status_ok": sum(r["status"] == 0 for r in res), "inlier_observations": int(inl.sum()),
            "trials": _spread([r["trials"] for r in res]), "rms_px_median": statistics.median(r["rms_px"] for r in res),
            "max_gap_to_ground_truth": {"dq": max(gq), "dt": max(gt)}}
    if host_images > 0:
        det = detection_result_from_arrays(s.obs_cam, s.obs_tag, s.obs_px, s.tag_wh, len(s.cam_gt))
        rec = TagReconstructor(det)
        rec.setCameraModel(CameraModel(*[float(v) for v in s.intr], s.dist, 4000, 6000))
        rec.setReconstructedTags({t: ReconstructedTag(t, "apriltag_36h11", s.tag_gt[t, :4], s.tag_gt[t, 4:], s.tag_wh[t, 0],
                                                      s.tag_wh[t, 1]) for t in range(len(s.tag_gt))})
        by_img = {}
        for ob in det.tagObservations:
            by_img.setdefault(ob.imageId, []).append(ob)
        sample = sorted(set(np.linspace(0, len(cam) - 1, min(host_images, len(cam))).astype(int).tolist()))
        per, hq, ht = [], [], []
        for i in sample:
            with contextlib.redirect_stdout(io.StringIO()):
                t0 = time.perf_counter()
                out = rec.computeRelativeCameraPoseFromImg(i, s.intr, s.dist, observations=by_img.get(i, []))
                per.append(time.perf_counter() - t0)
            if out is not None:
                g = _gap(np.concatenate([out[0], out[1]]), cam[i])
                hq.append(g[0])
                ht.append(g[1])
        line["host"] = {"images_timed": len(sample), "s_per_image": _spread(per),
                        "images_per_s": 1.0 / statistics.median(per),
                        "max_gap_to_device": {"dq": max(hq), "dt": max(ht)} if hq else None}
        line["device_over_host_images_per_s"] = line["images_per_s"] / line["host"]["images_per_s"]
    line.update({"unit": "ms", "dtype": "f64", "data": "synthetic"})
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="100x60_vis0.30,500x200,closeup_2000",
                    help="comma-separated names out of: %s" % ", ".join(SCENES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-images", type=int, default=10, help="images the host loop is timed on (0: skip it)")
    ap.add_argument("--kernels-only", action="store_true", help="one device call per scene after a warm-up, no timing")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_localize.py needs an MI355X: no GPU visible")
    names = [n for n in a.scenes.split(",") if n]
    for n in names:
        if n not in SCENES:
            raise SystemExit("unknown scene %r" % n)
    for n in names:
        bench(n, a.reps, a.host_images, a.kernels_only)


if __name__ == "__main__":
    main()
