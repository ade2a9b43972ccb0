#!/usr/bin/env python3
"""Times the calibration of a camera against a finished map (vmm_ba_calibrate) beside scipy on the same problem.

One JSON line per scene.  The map is the scene's ground truth, the detections carry the generator's default noise, the
camera model starts off the truth by --perturb times (+200, -150, +30, -25, +0.02, -0.05, +1e-3, -1e-3, +0.02).
"device": engine.calibrate on the whole batch, non-robust, no reclassification -- a host clock around a call that ends
in blocking copies back, so upload, the localisation, every LM trial with its read-back of the control block, the
covariances and the download are all inside; run once untimed first (code-object load), then --reps times: median with
minimum and maximum.  The line records the device, the sizes, and the trial counts of the device and of scipy.
"host": scipy.optimize.least_squares (trf, sparse Jacobian: 6 columns per image + 9 shared) on the same residuals over
the same observations, started at the true poses (cam_gt) and the same perturbed model; residuals
and Jacobian in vectorised numpy (the closed forms of the cost functor); its wall time, its evaluations and its
parameter gap to the device result in standard deviations of the device's covariance.

--kernels-only runs each scene's device call once after a warm-up and nothing else: the process to put under a
kernel-trace profiler for per-kernel times.

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
    "100x60_vis0.30": (1, dict(n_cams=100, n_tags=60, visibility=0.30)),
    "500x200": (2, dict(n_cams=500, n_tags=200)),
}
PERTURB = np.array([200.0, -150.0, 30.0, -25.0, 0.02, -0.05, 1e-3, -1e-3, 0.02])


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def _csr(s):
    start, order = s.by_image()
    return start, s.obs_cam[order].astype(np.int64), s.obs_tag[order].astype(np.int32), s.obs_px[order].copy()


def _rot(q):
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1).reshape(q.shape[:-1] + (3, 3))


def _world_corners(tag_qt, tag_wh):
    R = _rot(tag_qt[:, :4])
    sx, sy = np.array([-1.0, 1, 1, -1]), np.array([-1.0, -1, 1, 1])
    loc = np.stack([sx[None, :] * tag_wh[:, :1] / 2, sy[None, :] * tag_wh[:, 1:] / 2, np.zeros((len(tag_wh), 4))], axis=2)
    return np.einsum("tij,tkj->tki", R, loc) + tag_qt[:, None, 4:]


def _host_problem(s, img, tag, px):
    """(fun, jac, n_img) of scipy's problem: x = 6 rotation-vector/translation numbers per image about cam_gt (the
    rotation left-multiplied as exp([w]x)), then the nine of the model.  Jacobian by the closed forms."""
    n_img, n = len(s.cam_gt), len(tag)
    W = _world_corners(s.tag_gt, s.tag_wh)[tag]                  # (n, 4, 3)
    R0 = _rot(s.cam_gt[:, :4])
    uv = px.reshape(n, 4, 2)

    def project(x, want_jac):
        k = x[6 * n_img:]
        d = x[:6 * n_img].reshape(n_img, 6)
        th = np.linalg.norm(d[:, 3:], axis=1)
        K = np.zeros((n_img, 3, 3))
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = (-d[:, 5], d[:, 4], d[:, 5], -d[:, 3],
                                                                                   -d[:, 4], d[:, 3])
        a = np.where(th > 1e-12, np.sin(th) / np.maximum(th, 1e-300), 1.0)
        b = np.where(th > 1e-12, (1 - np.cos(th)) / np.maximum(th * th, 1e-300), 0.5)
        E = np.eye(3)[None] + a[:, None, None] * K + b[:, None, None] * (K @ K)
        R = E @ R0
        Bp = np.einsum("nij,nkj->nki", R[img], W)               # rotated points (n, 4, 3)
        P = Bp + (s.cam_gt[img, 4:] + d[img, :3])[:, None, :]
        x_, y_ = P[..., 0] / P[..., 2], P[..., 1] / P[..., 2]
        r2 = x_ * x_ + y_ * y_
        rad = 1 + r2 * (k[4] + r2 * (k[5] + r2 * k[8]))
        xd = x_ * rad + 2 * k[6] * x_ * y_ + k[7] * (r2 + 2 * x_ * x_)
        yd = y_ * rad + 2 * k[7] * x_ * y_ + k[6] * (r2 + 2 * y_ * y_)
        res = np.stack([k[0] * xd + k[2] - uv[..., 0], k[1] * yd + k[3] - uv[..., 1]], axis=2)   # (n, 4, 2)
        if not want_jac:
            return res.reshape(-1)
        dr = k[4] + r2 * (2 * k[5] + 3 * k[8] * r2)
        D00 = rad + 2 * x_ * x_ * dr + 2 * k[6] * y_ + 6 * k[7] * x_
        D01 = 2 * x_ * y_ * dr + 2 * k[6] * x_ + 2 * k[7] * y_
        D11 = rad + 2 * y_ * y_ * dr + 2 * k[7] * x_ + 6 * k[6] * y_
        iz = 1 / P[..., 2]
        G = np.zeros((n, 4, 2, 3))
        G[..., 0, 0], G[..., 0, 1], G[..., 0, 2] = k[0] * D00 * iz, k[0] * D01 * iz, -k[0] * (D00 * x_ + D01 * y_) * iz
        G[..., 1, 0], G[..., 1, 1], G[..., 1, 2] = k[1] * D01 * iz, k[1] * D11 * iz, -k[1] * (D01 * x_ + D11 * y_) * iz
        Jp = np.zeros((n, 4, 2, 6))
        Jp[..., :3] = G
        # d(exp([w]x) R0 p)/dw = -[b]x J_l(w), J_l the left Jacobian of SO(3): I + b K + c K^2
        Jp[..., 3] = Bp[..., None, 1] * G[..., 2] - Bp[..., None, 2] * G[..., 1]
        Jp[..., 4] = Bp[..., None, 2] * G[..., 0] - Bp[..., None, 0] * G[..., 2]
        Jp[..., 5] = Bp[..., None, 0] * G[..., 1] - Bp[..., None, 1] * G[..., 0]
        c = np.where(th > 1e-4, (th - np.sin(th)) / np.maximum(th ** 3, 1e-300), 1.0 / 6.0)
        Jl = np.eye(3)[None] + b[:, None, None] * K + c[:, None, None] * (K @ K)
        Jp[..., 3:] = np.einsum("nkrj,nji->nkri", Jp[..., 3:], Jl[img])
        Jk = np.zeros((n, 4, 2, 9))
        Jk[..., 0, 0], Jk[..., 1, 1], Jk[..., 0, 2], Jk[..., 1, 3] = xd, yd, 1.0, 1.0
        for col, (cu, cv) in ((4, (x_ * r2, y_ * r2)), (5, (x_ * r2 ** 2, y_ * r2 ** 2)), (8, (x_ * r2 ** 3, y_ * r2 ** 3)),
                              (6, (2 * x_ * y_, r2 + 2 * y_ * y_)), (7, (r2 + 2 * x_ * x_, 2 * x_ * y_))):
            Jk[..., 0, col], Jk[..., 1, col] = k[0] * cu, k[1] * cv
        return res.reshape(-1), Jp.reshape(8 * n, 6), Jk.reshape(8 * n, 9)

    rows = np.repeat(np.arange(8 * n), 6)
    cols = (6 * np.repeat(img, 8)[:, None] + np.arange(6)[None, :]).reshape(-1)

    def jac(x):
        from scipy.sparse import csr_matrix, hstack
        _, Jp, Jk = project(x, True)
        return hstack([csr_matrix((Jp.reshape(-1), (rows, cols)), shape=(8 * n, 6 * n_img)), csr_matrix(Jk)]).tocsr()

    return (lambda x: project(x, False)), jac, n_img


def bench(name, reps, perturb, with_host, kernels_only, device_name):
    from visual_marker_mapping_amd import engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = SCENES[name]
    s = make_scene(cfg, **kw)
    start, img, tag, px = _csr(s)
    k0 = np.concatenate([s.intr, s.dist]) + perturb * PERTURB
    call = lambda: eng.calibrate(k0[:4], k0[4:], s.tag_gt, s.tag_wh, start, tag, px, robustify=0, reclassify_passes=0,
                                 inlier_px=1e4, loc_inlier_px=1e4)
    intr, dist, icov, cam, ccov, inl, res, rep = call()   # warm-up
    if kernels_only:
        call()
        return
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    k = np.concatenate([intr, dist])
    line = {"metric": "calibrate", "device": device_name, "scene": name, "images": len(cam), "tags": len(s.tag_gt),
            "observations": len(tag), "reps": reps, "perturb": perturb, "call_ms": _spread([1e3 * t for t in times]),
            "status": rep["status"], "trials": rep["trials"], "accepted": rep["accepted"], "passes": rep["passes"],
            "images_used": rep["n_images_used"], "observations_used": rep["n_obs_used"],
            "ms_per_trial": statistics.median(times) * 1e3 / max(rep["trials"], 1),
            "rms_px": {"initial": rep["initial_rms_px"], "final": rep["final_rms_px"]},
            "error_to_truth_rel": (np.abs(k - np.concatenate([s.intr, s.dist]))
                                   / np.maximum(np.abs(np.concatenate([s.intr, s.dist])), 1.0)).tolist(),
            "sigma": np.sqrt(np.diag(icov)).tolist()}
    if with_host:
        from scipy.optimize import least_squares
        fun, jac, n_img = _host_problem(s, img, tag, px)
        x0 = np.concatenate([np.zeros(6 * n_img), k0])
        t0 = time.perf_counter()
        sol = least_squares(fun, x0, jac=jac, method="trf", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=200)
        t_host = time.perf_counter() - t0
        sig = np.sqrt(np.diag(icov))
        line["host"] = {"solver": "scipy.optimize.least_squares trf, sparse Jacobian", "s": t_host, "nfev": int(sol.nfev),
                        "njev": int(sol.njev), "cost": float(sol.cost),
                        "gap_to_device_sigma": (np.abs(sol.x[6 * n_img:] - k) / np.where(sig > 0, sig, 1.0)).tolist()}
        line["device_cost"] = rep["final_cost"]
        line["host_over_device_time"] = t_host / statistics.median(times)
    line.update({"unit": "ms", "dtype": "f64", "data": "synthetic"})
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="20x10,100x60_vis0.30,500x200", help="comma-separated names out of: %s" % ", ".join(SCENES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--perturb", type=float, default=1.0, help="multiple of the start perturbation")
    ap.add_argument("--no-host", action="store_true", help="skip the scipy run")
    ap.add_argument("--kernels-only", action="store_true", help="one device call per scene after a warm-up, no timing")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_calibrate.py needs an MI355X: no GPU visible")
    names = [n for n in a.scenes.split(",") if n]
    for n in names:
        if n not in SCENES:
            raise SystemExit("unknown scene %r" % n)
    for n in names:
        bench(n, a.reps, a.perturb, not a.no_host, a.kernels_only, torch.cuda.get_device_name(0))


if __name__ == "__main__":
    main()
