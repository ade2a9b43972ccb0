#!/usr/bin/env python3
"""Times small bundle adjustments three ways in one process: engine.solve_small (one launch, the whole LM loop in one
workgroup per problem), the handle path (a resident BundleAdjuster: set_state + solve + get_state, the graph of nine
kernels per LM iteration with host polls), and the CPU oracle (DENSE_NORMAL, one thread) on the host.

One JSON line per case.  The legs alternate inside every repetition (small, handle, oracle, small, ...), after one
untimed round of all three (code-object load, graph capture); every figure is the median over --reps repetitions with
minimum and maximum.  A host clock around calls that end in blocking copies back: uploads, the launch(es), the polls and
the download are inside.  All legs start from the same poses and stop by the same rules; the line records each leg's
iteration count and final cost.
  single   one problem per call: 3x2, 20x10 (robust), 70x24 at visibility 0.3 -- milliseconds per solve
  batch    256 and 4096 copies of 20x10 (robust) in one solve_small call -- problems per second; the handle and the oracle
           solve --batch-serial of them one after the other (their rate does not depend on the count)
  incremental   bench.py's --workload incremental scene (100 x 60, visibility 0.3): wall time of startReconstruction with
           oneLaunch False and True, alternating, after one untimed run of each

Run it in several sessions (processes) to see the spread between them: --session tags the lines.
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

SINGLE = {
    "3x2": (1, dict(n_cams=3, n_tags=2)),
    "20x10": (1, dict()),
    "70x24_vis0.30": (1, dict(n_cams=70, n_tags=24, visibility=0.3)),
}


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def _problem(s):
    return (s.intr, s.dist, s.cam_init, s.tag_init, s.tag_wh, s.fixed_tag, s.obs_cam, s.obs_tag, s.obs_px)


class Legs:
    """The three ways to solve scene s from its initial poses; each returns (iterations, final cost)."""

    def __init__(self, s):
        from oracle import oracle as O
        from visual_marker_mapping_amd import engine as eng
        self.s, self.O, self.eng = s, O, eng
        self.opts = eng.default_options(robustify=1)
        self.oopts = O.default_options(robustify=1, linear_solver=O.DENSE_NORMAL, num_threads=1)
        self.ba = eng.BundleAdjuster(*_problem(s))
        self.sc = O.Scene(*_problem(s))

    def small(self, copies=1):
        out = self.eng.solve_small([_problem(self.s)] * copies, options=self.opts)
        return out[0][2]["iterations"], out[0][2]["final_cost"]

    def handle(self):
        self.ba.set_state(self.s.cam_init, self.s.tag_init)
        out = self.ba.solve(self.opts)
        self.ba.get_state()
        return out["iterations"], out["final_cost"]

    def oracle(self):
        self.sc.cam_qt[:] = self.s.cam_init
        self.sc.tag_qt[:] = self.s.tag_init
        summ, _ = self.O.solve(self.sc, self.oopts, trace_capacity=1)
        return summ["iterations"], summ["final_cost"]

    def close(self):
        self.ba.close()


def _timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def bench_single(name, reps, base):
    from visual_marker_mapping_amd.synthetic import make_scene
    cfg, kw = SINGLE[name]
    s = make_scene(cfg, **kw)
    legs = Legs(s)
    order = (("solve_small", legs.small), ("handle", legs.handle), ("oracle_host", legs.oracle))
    result = {k: fn() for k, fn in order}   # untimed round
    times = {k: [] for k, _ in order}
    for _ in range(reps):
        for k, fn in order:
            times[k].append(1e3 * _timed(fn)[0])
    legs.close()
    line = dict(base, case="single", scene=name, images=len(s.cam_gt), tags=len(s.tag_gt), observations=len(s.obs_cam),
                reps=reps, unit="ms per solve", ms={k: _spread(v) for k, v in times.items()},
                iterations={k: r[0] for k, r in result.items()}, final_cost={k: r[1] for k, r in result.items()})
    line["handle_over_small"] = line["ms"]["handle"]["median"] / line["ms"]["solve_small"]["median"]
    line["oracle_over_small"] = line["ms"]["oracle_host"]["median"] / line["ms"]["solve_small"]["median"]
    return line


def bench_batch(copies, reps, serial, base):
    from visual_marker_mapping_amd.synthetic import make_scene
    s = make_scene(1)
    legs = Legs(s)
    many = lambda fn: (lambda: [fn() for _ in range(serial)][0])
    order = (("solve_small", lambda: legs.small(copies), copies), ("handle", many(legs.handle), serial),
             ("oracle_host", many(legs.oracle), serial))
    result = {k: fn() for k, fn, _ in order}   # untimed round
    rate = {k: [] for k, _, _ in order}
    for _ in range(reps):
        for k, fn, n in order:
            rate[k].append(n / _timed(fn)[0])
    legs.close()
    line = dict(base, case="batch", scene="20x10", copies=copies, serial_solves_of_the_other_legs=serial, reps=reps,
                unit="problems per second", problems_per_s={k: _spread(v) for k, v in rate.items()},
                iterations={k: r[0] for k, r in result.items()})
    line["small_over_handle"] = line["problems_per_s"]["solve_small"]["median"] / line["problems_per_s"]["handle"]["median"]
    line["small_over_oracle"] = line["problems_per_s"]["solve_small"]["median"] / line["problems_per_s"]["oracle_host"]["median"]
    return line


def bench_incremental(reps, base):
    from visual_marker_mapping_amd.synthetic import make_scene
    from visual_marker_mapping_amd.tag_reconstructor import CameraModel, TagReconstructor, detection_result_from_arrays
    n_cams, n_tags, vis = 100, 60, 0.3
    s = make_scene(2, n_cams=n_cams, n_tags=n_tags, visibility=vis)
    seconds, info = {False: [], True: []}, {}
    for rep in range(reps + 1):   # the first round is untimed
        for one_launch in (False, True):
            rec = TagReconstructor(detection_result_from_arrays(s.obs_cam, s.obs_tag, s.obs_px, s.tag_wh, n_cams))
            rec.setCameraModel(CameraModel(*[float(v) for v in s.intr], s.dist, 4000, 6000))
            calls = [0]
            if one_launch:
                from visual_marker_mapping_amd import engine as eng
                inner = eng.solve_small

                def counted(*a, **k):
                    calls[0] += 1
                    return inner(*a, **k)
                eng.solve_small = counted
            buf = io.StringIO()
            try:
                with contextlib.redirect_stdout(buf):
                    dt, _ = _timed(lambda: rec.startReconstruction(1, oneLaunch=one_launch))
            finally:
                if one_launch:
                    eng.solve_small = inner
            if rep > 0:
                seconds[one_launch].append(dt)
            info[one_launch] = dict(bundle_adjustments=buf.getvalue().count("Solution "), through_solve_small=calls[0],
                                    cameras=len(rec.getReconstructedCameras()), tags=len(rec.getReconstructedTags()))
            rec.close()
    return dict(base, case="incremental", scene="100x60_vis0.30", observations=int(s.n_obs), reps=reps, unit="s per run",
                seconds={"handle": _spread(seconds[False]), "oneLaunch": _spread(seconds[True])},
                runs={"handle": info[False], "oneLaunch": info[True]},
                handle_over_one_launch=statistics.median(seconds[False]) / statistics.median(seconds[True]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="single,batch,incremental")
    ap.add_argument("--reps", type=int, default=100, help="repetitions of a single-problem case")
    ap.add_argument("--batch-reps", type=int, default=5)
    ap.add_argument("--batch-serial", type=int, default=64, help="solves per repetition of the handle and oracle legs of a batch case")
    ap.add_argument("--incremental-reps", type=int, default=2)
    ap.add_argument("--session", type=int, default=0)
    ap.add_argument("--out", help="append the lines to this file as well")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_small.py needs an MI355X: no GPU visible")
    base = {"metric": "small_ba", "device": torch.cuda.get_device_name(0), "session": a.session, "dtype": "f64",
            "data": "synthetic"}
    lines = []
    cases = [c for c in a.cases.split(",") if c]
    if "single" in cases:
        lines += [bench_single(n, a.reps, base) for n in SINGLE]
    if "batch" in cases:
        lines += [bench_batch(n, a.batch_reps, a.batch_serial, base) for n in (256, 4096)]
    if "incremental" in cases:
        lines.append(bench_incremental(a.incremental_reps, base))
    for line in lines:
        print(json.dumps(line))
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
