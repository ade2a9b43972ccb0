#!/usr/bin/env python3
"""Times the covariance entries, vmm_ba_tag_translation_covariance against the parent commit's library.

    tools/bench_covariance.py --parent-lib <libvmm_ba.so of the parent commit> [--scenes ...] [--reps 5] [--rounds 2]

Per scene a handle at the ground truth (no solve) and three host-clocked calls, each ending in blocking copies back:
  (a) vmm_ba_tag_translation_covariance, in the parent library and in this one,
  (b) vmm_ba_covariance_blocks asked for exactly the tag marginals (this library only),
  (c) vmm_ba_covariance_blocks asked for all pose marginals (this library only).
Every library runs in a fresh child process of its own (VMM_BA_LIB is read when the package is imported), parent and
new alternating --rounds times in one session; a child runs each of its calls once untimed (code-object load, first
allocation), then --reps times.  One JSON line per child and scene, then one summary line per scene with the pooled
repetitions: median, minimum and maximum of (a) in both libraries, of (b) and (c), the bar of DESIGN.md section 9 for an
A/B against the parent (median (a, new) - median (a, parent) <= max (a, parent) - min (a, parent)), and the flop count
of the substitution of (c), n_blk (n_blk - 1) 64^2 ldb, as a rate and as a fraction of --peak-tflops.

--kernels-only runs (b) and (c) of each scene once after a warm-up with the library in use and nothing else: the
process to put under `rocprofv3 --kernel-trace --stats` for per-kernel times.

Needs an MI355X; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {
    "100x60_vis0.30": (1, dict(n_cams=100, n_tags=60, visibility=0.30)),
    "500x200": (2, dict(n_cams=500, n_tags=200)),
    "closeup_2000": (2, dict(n_cams=2000, n_tags=1000, neighbors_min=6, neighbors_max=10)),
}


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def _timed(call, reps):
    call()   # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def child(name, reps, which, kernels_only):
    from visual_marker_mapping_amd import _lib, engine as eng
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = SCENES[name]
    s = make_scene(cfg, **kw)
    n_c, n_t = len(s.cam_gt), len(s.tag_gt)
    tags = np.arange(n_c, n_c + n_t)
    every = np.arange(n_c + n_t)
    line = {"metric": "pose_covariance_child", "scene": name, "library": which, "lib_path": _lib.LIB_PATH, "reps": reps}
    with eng.BundleAdjuster(s.intr, s.dist, s.cam_gt, s.tag_gt, s.tag_wh, 0, s.obs_cam, s.obs_tag, s.obs_px) as ba:
        b = lambda: ba.covariance_blocks(np.stack([tags, tags], axis=1))
        c = lambda: ba.covariance_blocks(np.stack([every, every], axis=1))
        if kernels_only:
            for f in (b, c, b, c):
                f()
            return
        line["a_ms"] = _timed(lambda: ba.tag_translation_covariance(), reps)
        if which == "new":
            line["b_ms"] = _timed(b, reps)
            line["c_ms"] = _timed(c, reps)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="500x200,closeup_2000", help="comma-separated names out of: %s" % ", ".join(SCENES))
    ap.add_argument("--parent-lib", default=None, help="libvmm_ba.so built from the parent commit (omit: no (a), no bar)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="parent / new alternations, a fresh process each")
    ap.add_argument("--peak-tflops", type=float, default=78.6, help="f64 MFMA peak the fraction of (c) is quoted against")
    ap.add_argument("--kernels-only", action="store_true", help="(b) and (c) once per scene after a warm-up, no timing")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    names = [n for n in a.scenes.split(",") if n]
    for n in names:
        if n not in SCENES:
            raise SystemExit("unknown scene %r" % n)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_covariance.py needs an MI355X: no GPU visible")
    if a.child or a.kernels_only:
        for n in names:
            child(n, a.reps, a.child or "new", a.kernels_only)
        return
    pooled = {n: {"parent_a_ms": [], "a_ms": [], "b_ms": [], "c_ms": []} for n in names}
    for _ in range(a.rounds):
        for which, lib in (("parent", a.parent_lib), ("new", None)):
            if which == "parent" and lib is None:
                continue
            env = dict(os.environ, PYTHONPATH=ROOT)
            env.pop("VMM_BA_LIB", None)
            if lib is not None:
                env["VMM_BA_LIB"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--scenes", ",".join(names),
                                  "--reps", str(a.reps)], env=env, check=True, stdout=subprocess.PIPE, text=True).stdout
            for row in out.splitlines():
                if not row.startswith("{"):
                    continue
                print(row, flush=True)
                r = json.loads(row)
                for k in ("a_ms", "b_ms", "c_ms"):
                    pooled[r["scene"]]["parent_a_ms" if (k, r["library"]) == ("a_ms", "parent") else k] += r.get(k, [])
    from visual_marker_mapping_amd.synthetic import make_scene
    for n in names:
        cfg, kw = SCENES[n]
        s = make_scene(cfg, **kw)
        n_c, n_t = len(s.cam_gt), len(s.tag_gt)
        n_pad = -(-6 * min(n_c, n_t) // 64) * 64      # the larger family is eliminated (ELIM_AUTO)
        n_blk, ldb = n_pad // 64, -(-6 * (n_c + n_t) // 64) * 64
        p = pooled[n]
        line = {"metric": "pose_covariance", "scene": n, "cameras": n_c, "tags": n_t, "observations": int(s.n_obs),
                "reps_pooled": len(p["b_ms"]), "rounds": a.rounds,
                "a_tag_translation_covariance_ms": _spread(p["a_ms"]),
                "b_tag_marginals_ms": _spread(p["b_ms"]), "c_all_pose_marginals_ms": _spread(p["c_ms"])}
        flops = float(n_blk) * (n_blk - 1) * 64 * 64 * ldb
        line["c_substitution"] = {"n_blk": n_blk, "ldb": ldb, "flops": flops,
                                  "tflops_over_whole_call": flops / (1e9 * line["c_all_pose_marginals_ms"]["median"]),
                                  "fraction_of_peak_over_whole_call":
                                      flops / (1e9 * line["c_all_pose_marginals_ms"]["median"]) / a.peak_tflops,
                                  "peak_tflops": a.peak_tflops}
        if p["parent_a_ms"]:
            sa = _spread(p["parent_a_ms"])
            line["a_parent_tag_translation_covariance_ms"] = sa
            line["a_minus_parent_a_median_ms"] = line["a_tag_translation_covariance_ms"]["median"] - sa["median"]
            line["parent_a_max_minus_min_ms"] = sa["max"] - sa["min"]
            line["bar_met"] = bool(line["a_minus_parent_a_median_ms"] <= line["parent_a_max_minus_min_ms"])
        line.update({"unit": "ms", "dtype": "f64", "data": "synthetic"})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
