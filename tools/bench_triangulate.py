#!/usr/bin/env python3
"""Times the triangulation of free points against a finished map (vmm_ba_triangulate) beside a plain numpy solver.

One JSON line per scene, printed and appended to --output (default profiles/triangulate.jsonl).  The cameras are the
scene's ground truth, the points are the four corners of every tag, the pixels carry the generator's default noise.
"device": engine.triangulate on the whole batch -- a host clock around a call that ends in blocking copies back, so
upload, the two kernels and download are all inside; run once untimed first (code-object load), then --reps times:
median with minimum and maximum, points per second from the median.  "host": for scale only, a plain numpy
Levenberg-Marquardt of the same objective over the device's inlier sets, started at the ground truth, over
--host-points evenly spaced points: seconds per point, and its gap to the device result.

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {
    "100x60_vis0.30": (1, dict(n_cams=100, n_tags=60, visibility=0.30)),
    "closeup_60x80": (2, dict(n_cams=60, n_tags=80, neighbors_min=6, neighbors_max=10)),
    "500x200": (2, dict(n_cams=500, n_tags=200)),
}


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def _rotations(qt):
    q = qt[:, :4] / np.linalg.norm(qt[:, :4], axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)


def _tracks(s):
    """The four world corners of every tag as free points; point 4 t + k is corner k of tag t, its track sorted by camera."""
    order = np.lexsort((s.obs_cam, s.obs_tag))
    counts = np.bincount(s.obs_tag, minlength=len(s.tag_gt))
    R = _rotations(s.tag_gt)
    start, cam, uv, truth = [0], [], [], []
    b = 0
    for t in range(len(s.tag_gt)):
        idx = order[b:b + counts[t]]
        b += counts[t]
        for k, (sx, sy) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
            cam.append(s.obs_cam[idx])
            uv.append(s.obs_px[idx, 2 * k:2 * k + 2])
            start.append(start[-1] + len(idx))
            truth.append(R[t] @ [0.5 * sx * s.tag_wh[t, 0], 0.5 * sy * s.tag_wh[t, 1], 0.0] + s.tag_gt[t, 4:])
    return np.array(start, np.int64), np.concatenate(cam).astype(np.int32), np.concatenate(uv).copy(), np.array(truth)


def _sums(K, D, R, t, uv, X, a=1.0):
    """cost, J^T J and J^T r of one point over its views with the cost functor's projection and the Huber corrector."""
    P = R @ X + t
    iz = 1.0 / P[:, 2]
    x, y = P[:, 0] * iz, P[:, 1] * iz
    k1, k2, p1, p2, k3 = D
    r2 = x * x + y * y
    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    dr = k1 + r2 * (2 * k2 + 3 * k3 * r2)
    r = np.stack([K[0] * (x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) + K[2] - uv[:, 0],
                  K[1] * (y * rad + 2 * p2 * x * y + p1 * (r2 + 2 * y * y)) + K[3] - uv[:, 1]], axis=1)
    d00 = rad + 2 * x * x * dr + 2 * p1 * y + 6 * p2 * x
    d01 = 2 * x * y * dr + 2 * p1 * x + 2 * p2 * y
    d11 = rad + 2 * y * y * dr + 2 * p2 * x + 6 * p1 * y
    G = np.stack([np.stack([K[0] * d00 * iz, K[0] * d01 * iz, -K[0] * (d00 * x + d01 * y) * iz], axis=1),
                  np.stack([K[1] * d01 * iz, K[1] * d11 * iz, -K[1] * (d01 * x + d11 * y) * iz], axis=1)], axis=1)
    J = G @ R
    sq = np.einsum("ij,ij->i", r, r)
    big = sq > a * a
    root = np.sqrt(np.where(big, sq, 1.0))
    rho = np.where(big, 2 * a * root - a * a, sq)
    w = np.where(big, a / root, 1.0)
    return 0.5 * rho.sum(), np.einsum("i,ijk,ijl->kl", w, J, J), np.einsum("i,ijk,ij->k", w, J, r)


def _host_lm(K, D, R, t, uv, X0):
    X = np.array(X0, np.float64)
    cost, A, g = _sums(K, D, R, t, uv, X)
    lam = 1e-3
    for _ in range(30):
        step = np.linalg.solve(A + lam * np.diag(np.maximum(np.diag(A), 1e-12)), -g)
        if np.abs(step).max() < 1e-14:
            break
        c2, A2, g2 = _sums(K, D, R, t, uv, X + step)
        if c2 < cost:
            X, cost, A, g, lam = X + step, c2, A2, g2, max(lam * 0.1, 1e-12)
        elif c2 - cost <= 1e-10 * cost + 1e-20:
            break
        else:
            lam *= 10.0
    return X


def bench(name, reps, host_points, kernels_only):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = SCENES[name]
    s = make_scene(cfg, **kw)
    start, cam, uv, truth = _tracks(s)
    cam_cov = np.tile(np.diag([1e-6] * 3 + [1e-7] * 3), (len(s.cam_gt), 1, 1))
    call = lambda: eng.triangulate(s.intr, s.dist, s.cam_gt, start, cam, uv, cam_cov=cam_cov)
    xyz, cov, cov_cams, inl, res = call()   # warm-up
    if kernels_only:
        call()
        return None
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    ok = np.array([r["status"] == 0 for r in res])
    line = {"metric": "triangulate", "scene": name, "cameras": len(s.cam_gt), "points": len(xyz), "observations": len(cam),
            "track_length": _spread([int(v) for v in np.diff(start)]), "reps": reps,
            "call_ms": _spread([1e3 * t for t in times]), "points_per_s": len(xyz) / statistics.median(times),
            "status_ok": int(ok.sum()), "inlier_observations": int(inl.sum()),
            "trials": _spread([r["trials"] for r in res]), "rms_px_median": statistics.median(r["rms_px"] for r in res),
            "max_gap_to_ground_truth_m": float(np.linalg.norm(xyz - truth, axis=1)[ok].max()) if ok.any() else None}
    if host_points > 0:
        R, t = _rotations(s.cam_gt), s.cam_gt[:, 4:]
        sample = sorted(set(np.linspace(0, len(xyz) - 1, min(host_points, len(xyz))).astype(int).tolist()))
        per, gap = [], []
        for p in sample:
            keep = np.arange(start[p], start[p + 1])[inl[start[p]:start[p + 1]]]
            if len(keep) < 2:
                continue
            t0 = time.perf_counter()
            X = _host_lm(s.intr, s.dist, R[cam[keep]], t[cam[keep]], uv[keep], truth[p])
            per.append(time.perf_counter() - t0)
            gap.append(float(np.abs(X - xyz[p]).max()))
        if per:
            line["host"] = {"points_timed": len(per), "s_per_point": _spread(per),
                            "points_per_s": 1.0 / statistics.median(per), "max_gap_to_device_m": max(gap)}
            line["device_over_host_points_per_s"] = line["points_per_s"] / line["host"]["points_per_s"]
    line.update({"unit": "ms", "dtype": "f64", "data": "synthetic"})
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default=",".join(SCENES), help="comma-separated names out of: %s" % ", ".join(SCENES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-points", type=int, default=40, help="points the numpy solver is timed on (0: skip it)")
    ap.add_argument("--kernels-only", action="store_true", help="one device call per scene after a warm-up, no timing")
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "triangulate.jsonl"),
                    help="file the JSON lines are appended to ('' for none)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_triangulate.py needs an MI355X: no GPU visible")
    names = [n for n in a.scenes.split(",") if n]
    for n in names:
        if n not in SCENES:
            raise SystemExit("unknown scene %r" % n)
    for n in names:
        line = bench(n, a.reps, a.host_points, a.kernels_only)
        if line is None:
            continue
        print(json.dumps(line), flush=True)
        if a.output:
            with open(a.output, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
