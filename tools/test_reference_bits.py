#!/usr/bin/env python3
"""SHA-256 of every scene array, truth, reference A and B and bound that the test-support modules under tests/ hand the
CPU tests, at the states those tests use: one line per case and quantity, written as JSON.  Run on two checkouts and
compared line by line it shows whether a change to the support modules moved anything a test asserts.

    python tools/test_reference_bits.py --out bits.json [--root OTHER_CHECKOUT]

A longdouble is hashed as the pair of doubles (x rounded, the remainder), so the padding bytes of its storage do not count.
"""
import argparse
import hashlib
import json
import os
import struct
import sys

import numpy as np

CONTAINERS = ("Scene", "CovScene", "Handle", "Pick", "SyntheticScene")


def feed(h, v):
    if isinstance(v, np.generic):
        v = np.asarray(v)
    if isinstance(v, np.ndarray):
        if v.dtype == object:
            return feed(h, v.tolist())
        h.update(("<%s %s>" % (v.dtype.str, v.shape)).encode())
        if v.dtype == np.longdouble:
            hi = v.astype(np.float64)
            with np.errstate(invalid="ignore"):
                lo = np.where(np.isfinite(hi), v - hi, 0).astype(np.float64)
            v = np.stack([hi, lo])
        return h.update(np.ascontiguousarray(v).tobytes())
    if isinstance(v, float):
        return h.update(b"f" + struct.pack("<d", v))
    if v is None or isinstance(v, (bool, int, str, bytes)):
        return h.update(repr(v).encode())
    if isinstance(v, dict):
        for k in sorted(v, key=repr):
            h.update(repr(k).encode())
            feed(h, v[k])
        return h.update(b"}")
    if isinstance(v, (list, tuple, range)):
        for x in v:
            feed(h, x)
        return h.update(b"]")
    if type(v).__name__ in CONTAINERS:
        return feed(h, {k: x for k, x in v.__dict__.items() if not callable(x)})
    raise TypeError(type(v))


OUT = {}


def put(label, value):
    h = hashlib.sha256()
    feed(h, value)
    assert label not in OUT, label
    OUT[label] = h.hexdigest()


def eval_lines(O, kats):
    import eval_cases as ec
    import test_eval_cases_cpu as t
    for a in (0.5, 1.0, 2.5):
        put("eval scene mixed %g" % a, ec.mixed_scene(a))
    for few in ("tags", "cams"):
        s = ec.ragged_scene(few)
        put("eval scene ragged %s" % few, [s, ec.ragged_mask(s), ec.ragged_constants(s), ec.task_counts(s)])
    cases = list(t._cpu_cases(O, kats)) + [("mixed a=1 f32", ec.Case(O, ec.mixed_scene(1.0), a=1.0, f32=True))]
    for label, c in cases:
        put("eval %s scene" % label, c.scene)
        put("eval %s truth" % label, [c.ref, c.mag])
        put("eval %s refs" % label, c.refs)
        put("eval %s bound" % label, [c.bound, getattr(c, "bound_f32", None)])


def cov_lines(O):
    import cov_cases as cc
    for name, elims in cc.SCENES.items():
        put("cov scene %s" % name, cc.scene(name))
        for elim in elims:
            c = cc.cpu_case(name, elim)
            put("cov %s %s truth" % (name, elim), [c.H, c.truth, c.last_correction, c.min_eig, c.pos])
            put("cov %s %s refs" % (name, elim), c.refs)
            put("cov %s %s bound" % (name, elim), c.bound)
    for name in ("ragged_tags", "ragged_cams"):
        for variant, _, _ in cc.MODEL_VARIANTS:
            c = cc.model_case(O, name, variant)
            put("cov model %s %s truth" % (name, variant), [c.k, c.mask, c.Sk, c.rk, c.cov, c.step, c.sigma, c.oracle])
            put("cov model %s %s refs" % (name, variant), c.refs)
            put("cov model %s %s bound" % (name, variant), [c.bound_cov, c.bound_step])
    for elim in ("cams", "tags"):
        put("cov requests %s" % elim, [list(r) for r in cc.edge_requests(elim)])
    put("cov pairs", [cc.all_pairs(36), cc.marginals_and_cross(36)])


def linalg_lines(O):
    import linalg_cases as lc
    import test_linalg_cases_cpu as t
    from visual_marker_mapping_amd.synthetic import make_scene
    for n, kappa in t._gpu_cases_up_to_1408():
        c = lc.case_bounds(n, kappa, 0)
        put("linalg %d %.0e system" % (n, kappa), [c["A"], c["b"], c["norm_A"], c["x_ref"]])
        put("linalg %d %.0e refs" % (n, kappa), c["refs"])
        put("linalg %d %.0e bound" % (n, kappa), [c["bound"], c["forward_bound"]])
    s = make_scene(1)
    for robust in (0, 1):
        blk = lc.blocks_from_oracle(O, s, s.cam_init, s.tag_init, robust, s.fixed_tag)
        prob = lc.LmProblem(blk, s.obs_cam, s.obs_tag, s.cam_init, s.tag_init, None, np.arange(len(s.tag_init)) == s.fixed_tag)
        for radius in (1e4, 1e12):
            for elim in ("cams", "tags"):
                three = lc.lm_step_reference(prob, radius, elim)
                put("linalg lm robust%d %.0e %s three" % (robust, radius, elim), three)
                put("linalg lm robust%d %.0e %s bound" % (robust, radius, elim), lc.lm_bounds(three))


def evaluation(label, ev, more=()):
    put(label + " truth", ev.truth)
    put(label + " refs", ev.refs)
    put(label + " bound", [ev.bound] + list(more))


def finished_map_lines(O):
    import finished_map_cases as fm
    for entry, (build, cases) in fm.BUILDERS.items():
        for args in cases:
            case = build(*args)
            label = "fm %s %s" % (entry, fm.case_id(args))
            put(label + " scene", case.scene)
            states, flags, costs = fm.host_states(O, case)
            put(label + " state", [states, flags, costs, [case.classify(i, states[i]) for i in range(case.n_items)]])
            ev = case.evaluate(O, states, flags)
            evaluation(label, ev, [ev.floor, ev.reference_deviation])
    for n_tags, with_map in fm.PREDICT_CASES:
        for n_poses in fm.PREDICT_POSES:
            case = fm.PredictCase(n_tags, n_poses, with_map)
            label = "fm predict %d x %d %s" % (n_tags, n_poses, "map" if with_map else "nomap")
            visible, on_rounding = case.host_visible()
            put(label + " scene", [case.case, case.tag_cov, visible, on_rounding])
            evaluation(label, case.evaluate(O, visible))


def arrowhead_lines(O):
    import arrowhead_cases as ah
    import test_arrowhead_cases_cpu as t
    for lam, cases in ((None, t.ALL_CASES), (ah.LAM_INIT, t.TRIAL_CASES)):
        for name, args in cases:
            case = t.BUILD[name](*args)
            label = "ah %s %s%s" % (name, ah.case_id(args), "" if lam is None else " trial")
            state = t._start_state(case)
            put(label + " scene", [case.scene, case.mask, case.exercises, state])
            evaluation(label, case.evaluate(O, *state, **({} if lam is None else dict(lam=lam))))
    case = ah.observation_edges("distorted", True, "huber0.5")
    evaluation("ah one tag", case.evaluate(O, *t._start_state(case, 1)))
    for name, args in (("items", (5,)), ("frames", (5,)), ("frames", (5, "huber0.5", True))):
        case = t.BUILD[name](*args)
        shared, poses, cost = case.host_optimum(O)
        flags = case.flags_list(case.scene.label)
        put("ah %s %s optimum" % (name, ah.case_id(args)), [shared, poses, cost, case.truth(shared, poses, flags, case.participants(flags))])


def init_lines(O):
    import finished_map_cases as fm
    import init_cases as ic
    import test_init_cases_cpu as t
    rng = np.random.default_rng(6)
    q = rng.normal(size=(400, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    a, b = np.c_[q[:200], rng.normal(size=(200, 3))], np.c_[q[200:], rng.normal(size=(200, 3))]
    put("init quat_from_R", [ic.quat_from_R(ic.chain(fam, a, b, dtype)[0], dtype) for fam in ic.FAMILIES for dtype in (np.float64, np.longdouble)])
    for fam in ic.FAMILIES:
        put("init chained %s" % fam, [ic.chained_pose(fam, a, b), ic.chained_pose_a(fam, a, b), ic.chained_pose(fam, a, b, np.float64)])
    for model in fm.MODELS:
        intr, dist = fm.camera_model(model)
        pc = ic.chain_points(model)
        put("init chain %s" % model, [pc, ic.project_cm(intr, dist, pc), ic.project_cm_a(intr, dist, pc), ic.project_cm(intr, dist, pc, np.float64)])
        s = ic.exact_batch(model)
        put("init exact %s" % model, [s, ic.branches_of(s.qt_gt), ic.host_quad(s.intr, s.dist, s.wh, s.px), ic.exact_references(s),
                                      ic.quad_weak_starts(s.intr, s.dist, s.wh, s.px)])
        for n in ic.QUAD_SIZES:
            s = ic.quad_batch(model, n)
            put("init quad %s %d scene" % (model, n), s)
            for fallback in (False, True):
                qt2, rms2 = ic.host_quad(s.intr, s.dist, s.wh, s.px, fallback=fallback)
                opt = [ic.quad_optimum(s.intr, s.dist, qt2[:, k], s.wh, s.px) for k in range(2)]
                put("init quad %s %d host fallback=%s" % (model, n, fallback), [qt2, rms2, opt])
            put("init quad %s %d rms" % (model, n), [[ic.quad_rms(s.intr, s.dist, qt2[:, k], s.wh, s.px), ic.quad_rms_a(s.intr, s.dist, qt2[:, k], s.wh, s.px),
                                                      ic.quad_sums(s.intr, s.dist, qt2[:, k], s.wh, s.px)] for k in range(2)])
        for fam in ic.FAMILIES:
            for winners in (False, True):
                h, quads, res = t._host_state(fam, model, winners)
                label = "init select %s %s %s" % (fam, model, "winners" if winners else "noisy")
                put(label + " scene", [h, quads])
                put(label + " restated", res)
                put(label + " refs", [ic.pick_references(f, pk) for (f, p), pk in res["picks"].items()])
            h, (qt2, rms2), _ = t._host_state(fam, model)
            p = h.counts.index(513)
            oth = h.tag_qt if fam == "cam" else h.cam_qt
            put("init tie %s %s" % (fam, model), ic.select_pose(fam, h, p, h.lists(fam)[p], np.ones(len(oth), bool), oth, qt2, rms2, ic.TIE_CAP_PX))
            h, _, res = t._host_state(fam, model, counts=ic.TRIAL_COUNTS)
            oth = h.tag_qt if fam == "cam" else h.cam_qt
            state = res["cam_qt"] if fam == "cam" else res["tag_qt"]
            put("init trial %s %s" % (fam, model), [h, [[ic.trial(O, fam, h, p, state[p], lst, oth), ic.refine_model(fam, h, p, state[p], lst, oth)]
                                                        for p, lst in enumerate(h.lists(fam))]])
        for variant in ("corridor", "cross links", "cut", "constant camera", "degenerate end"):
            h = ic.growth_handle(model, variant)
            qt2, rms2 = ic.host_quad(h.intr, h.dist, h.tag_wh[h.obs_tag], h.obs_px)
            res = ic.restate(h, qt2, rms2, ic.SCORE_CAP_PX, 2)
            put("init growth %s %s" % (model, variant), [h, qt2, rms2, res, ic.reach(h), [ic.pick_references(f, pk) for (f, p), pk in res["picks"].items()]])
        for masked in (False, True):
            for unreached in (False, True):
                h = ic.report_handle(model, masked, unreached)
                cam_ok, tag_ok, _ = ic.reach(h, 1)
                args = (h, h.cam_gt, h.tag_gt, cam_ok, tag_ok)
                put("init report %s masked=%s unreached=%s" % (model, masked, unreached),
                    [h, ic.report_truth(*args), ic.report_a(O, *args), ic.report_b(*args), ic.report_floor(*args)])


def predict_lines(O):
    import finished_map_cases as fm
    import predict_cases as pc
    import predict_joint_cases as pj
    for name, case in pc.all_cases() + [("lanes_relief_%d" % n, pc.lanes(n, pj.JOINT_POSES, relief=fm.PREDICT_RELIEF)) for n in pj.JOINT_TAGS]:
        vis, sl = pc.host_visible(case)
        put("predict %s" % name, [case, vis, sl])
    case = pc.scene()
    cov = pc.random_tag_cov(len(case["tag_qt"]), fixed=case["fixed_tag"])
    vis, _ = pc.host_visible(case)
    put("predict scene host_pose", [cov, [pc.host_pose(O, case, p, vis[p], tag_cov=cov) for p in range(len(vis)) if vis[p].any()],
                                    [pc.centre_jacobian(q) for q in case["cam_qt"]]])
    for n_tags in (2, 65):
        diag = pc.random_tag_cov(n_tags, fixed=[], seed=20261204)
        jc = pj.JointCase(n_tags, pj.JOINT_POSES, pj.block_diagonal(diag))
        vis, _ = jc.host_visible()
        ev = jc.evaluate(O, vis)
        evaluation("predict joint block diagonal %d" % n_tags, ev, [[pj.independent_prop(jc, p, vis[p], diag) for p in ev.items]])
    Sw = pj.world_covariance()
    jc = pj.JointCase(65, pj.JOINT_POSES, pj.rigid(pc.lanes(65, 1, relief=fm.PREDICT_RELIEF)["tag_qt"], Sw))
    vis, _ = jc.host_visible()
    evaluation("predict joint rigid 65", jc.evaluate(O, vis), [Sw, jc.joint, [pj.rigid_camera(q, np.longdouble) for q in jc.case["cam_qt"]],
                                                               [pj.rigid_tag(q, np.longdouble) for q in jc.case["tag_qt"]]])
    put("predict joint covariances", [pj.dense_spd(3, seed=5), pj.tiled(pj.dense_spd(4), 9, (0, 2, 3)), pj.lower_symmetric(pj.dense_spd(3))])


def yardstick_lines(O):
    import rig_cases as rc
    import tag_cases as tc
    import yardstick as ys
    from visual_marker_mapping_amd.synthetic import make_scene
    rng = np.random.default_rng(7)
    q = rng.normal(size=(64, 7))
    put("yardstick rotation", [ys.rotation(p) for p in q])
    put("yardstick pose_gap", ys.pose_gap(q[:32], q[32:]))
    put("tag pose_minus", [tc.pose_minus(O, a, b) for a, b in zip(q[:32], q[32:])])
    put("rig compose", [rc.compose(a, b) for a, b in zip(q[:32], q[32:])])
    s = make_scene(1)
    k = np.concatenate([s.intr, s.dist]) + 0.01 * ys.PERTURB
    put("yardstick intrinsic_columns", [ys.intrinsic_columns(k, s.cam_gt[c], s.tag_gt[t], s.tag_wh[t]) for c, t in zip(s.obs_cam[:40], s.obs_tag[:40])])
    put("yardstick const_sets", ys.const_sets(s, 3, 2))
    blk = ys.pose_blocks(O, s, s.cam_gt, s.tag_gt, True, fixed_tag=s.fixed_tag)
    cam_const, tag_const = ys.const_sets(s, 3, 2)
    put("yardstick blocks", [blk, ys.free_system(s, blk, cam_const, tag_const)])
    put("yardstick joint_system", ys.joint_system(O, k, s.cam_gt, s.tag_gt, *ys.scene_args(s), robust=True, want_magnitude=True))
    for name in sorted(rc.SCENES):
        r = rc.rig_scene(name)
        put("rig %s" % name, [r, rc.rig_system(O, r, r.rig_gt, r.ext_qt, None, True)])
    start, order = tc.by_tag(s)
    t = 3
    obs = order[start[t]:start[t + 1]]
    put("tag optimum", tc.tag_optimum(O, s.intr, s.dist, s.tag_gt[t], s.cam_gt, s.tag_wh[t], s.obs_cam[obs], s.obs_px[obs], True))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to hash")
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default=None, help="comma-separated families: eval, cov, linalg, finished_map, arrowhead, init, predict, yardstick")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path[:0] = [root, os.path.join(root, "tests")]
    from oracle import oracle as O
    O.build()
    with open(os.path.join(root, "tests", "golden", "kat_residual.json")) as f:
        kats = json.load(f)
    families = dict(eval=lambda: eval_lines(O, kats), cov=lambda: cov_lines(O), linalg=lambda: linalg_lines(O),
                    finished_map=lambda: finished_map_lines(O), arrowhead=lambda: arrowhead_lines(O), init=lambda: init_lines(O),
                    predict=lambda: predict_lines(O), yardstick=lambda: yardstick_lines(O))
    for name in (args.only.split(",") if args.only else families):
        families[name]()
        print("%s: %d lines so far" % (name, len(OUT)), flush=True)
    with open(args.out, "w") as f:
        json.dump(OUT, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %d lines to %s" % (len(OUT), args.out))


if __name__ == "__main__":
    main()
