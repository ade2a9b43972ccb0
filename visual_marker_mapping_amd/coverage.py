"""Command-line coverage step: how well would a camera be localised against a finished map, and where is the map too thin?

    python -m visual_marker_mapping_amd.coverage --project_path DIR [--map FILE] [--uncertainty FILE [--correlated]] \\
        (--poses FILE | --grid X0 X1 NX Y0 Y1 NY Z0 Z1 NZ --axis X Y Z [--axis ...] --up X Y Z) \\
        [--sigma_px S] [--margin_px M] [--max_view_angle_deg A] [--min_side_px P] [--min_tags N] [--covariances] \\
        [--output FILE] [--device N]

The reference has no such executable.  The tags come from the map (default <project>/reconstruction.json), the camera
model and the image size from <project>/camera_intrinsics.json.  The poses are hypothetical: no image stands behind them.
`--poses` names any file with a `reconstructed_cameras` list (world->camera, as the map holds its cameras); `--grid` puts
one pose on every node of a box and for every optical axis given (unit vectors in the world), the roll fixed by `--up`
(engine.grid_poses).  `--uncertainty` names a reconstruction_uncertainty.json: the part of a pose's covariance that the
tags' own uncertainty causes is propagated tag by tag (vmm_ba_predict_localization, include/vmm_ba.h, which also says
what the prediction ignores: occlusion, the correlations between tags, the planar ambiguity of a single tag).  All poses
go through one device call.  `--correlated` propagates the tags' joint covariance instead, cross blocks included
(vmm_ba_predict_localization_joint): the uncertainty file must have been written with `uncertainty.py --joint`, and
coverage.json then says "map_covariance": "joint" at its top level.

coverage.json:
    {"options": {image_width, image_height, sigma_px, margin_px, min_depth, max_view_angle_deg, min_side_px, min_tags},
     "poses": [{"id", "rotation", "translation", "status", "num_visible_tags", "sigma_pos_m", "sigma_rot_rad"
                [, "covariance": {rows, cols, coefficents}, "covariance_map": {...} with --covariances]}],
     "tags": [{"id", "num_poses"}],
     "tags_never_seen": [ids]}
"""
import argparse
import os
import sys

import numpy as np

from . import _lib, engine as _engine
from . import io as _io
from .tag_reconstructor import DetectionResult, TagReconstructor
from .triangulation import read_cameras, read_tag_covariances
from .uncertainty import read_tag_joint_covariance


def coverage_tree(options, report, tag_ids, covariances=False):
    """The property tree of coverage.json from the options (a dict), the result of
    TagReconstructor.predictLocalizationAccuracy and the ids of the map's tags.  Poses by ascending id."""
    seen = {int(t): 0 for t in tag_ids}
    poses = []
    for i in sorted(report):
        r = report[i]
        entry = dict(_io.pose_tree(i, r["pose"]), status=_lib.PRED_STATUS_NAMES[r["status"]],
                     num_visible_tags=int(r["n_visible"]), sigma_pos_m=float(r["sigma_pos_m"]),
                     sigma_rot_rad=float(r["sigma_rot_rad"]))
        if covariances:
            entry["covariance"] = _io.matrix_tree(r["covariance"])
            entry["covariance_map"] = _io.matrix_tree(r["covariance_map"])
        poses.append(entry)
        for t in r["visible_tags"]:
            seen[int(t)] += 1
    return {"options": dict(options), "poses": poses,
            "tags": [{"id": t, "num_poses": seen[t]} for t in sorted(seen)],
            "tags_never_seen": [t for t in sorted(seen) if seen[t] == 0]}


def summary_line(report, n_never_seen):
    """poses, share with status ok, median and worst sigma_pos_m among them, tags never seen."""
    ok = [r["sigma_pos_m"] for r in report.values() if r["status"] == _lib.PRED_OK]
    share = 100.0 * len(ok) / len(report) if report else 0.0
    if not ok:
        return "Predicted %d poses: %.1f %% ok; %d tags never seen" % (len(report), share, n_never_seen)
    return ("Predicted %d poses: %.1f %% ok, sigma_pos_m median %.3g worst %.3g; %d tags never seen"
            % (len(report), share, float(np.median(ok)), max(ok), n_never_seen))


def main(argv=None):
    ap = argparse.ArgumentParser(description="Predicts the localisation accuracy of hypothetical poses against a finished map")
    ap.add_argument("--project_path", required=True, help="Path to the project (holds camera_intrinsics.json and the map)")
    ap.add_argument("--map", default=None, help="map file (default: <project>/reconstruction.json)")
    ap.add_argument("--uncertainty", default=None, help="reconstruction_uncertainty.json with the tags' 6x6 covariances")
    ap.add_argument("--correlated", action="store_true",
                    help="propagate the tags' joint covariance (an --uncertainty file written with --joint)")
    ap.add_argument("--poses", default=None, help="file with a reconstructed_cameras list: the poses to predict")
    ap.add_argument("--grid", type=float, nargs=9, default=None, metavar=("X0", "X1", "NX", "Y0", "Y1", "NY", "Z0", "Z1", "NZ"),
                    help="a box of NX x NY x NZ nodes, one pose per node and --axis")
    ap.add_argument("--axis", type=float, nargs=3, action="append", default=None, metavar=("X", "Y", "Z"),
                    help="optical axis in the world (with --grid; repeatable)")
    ap.add_argument("--up", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="the world's up (with --grid)")
    for name, typ in (("sigma_px", float), ("margin_px", float), ("max_view_angle_deg", float), ("min_side_px", float),
                      ("min_tags", int)):
        ap.add_argument("--" + name, type=typ, default=None, help="vmm_ba_predict_options.%s" % name)
    ap.add_argument("--covariances", action="store_true", help="write the two 6x6 matrices of every pose")
    ap.add_argument("--output", default=None, help="output file (default: <project>/coverage.json)")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    a = ap.parse_args(argv)
    if (a.poses is None) == (a.grid is None):
        ap.error("give either --poses or --grid")
    if a.grid is not None and (not a.axis or a.up is None):
        ap.error("--grid needs at least one --axis and --up")
    if a.correlated and a.uncertainty is None:
        ap.error("--correlated needs --uncertainty")
    out = a.output or os.path.join(a.project_path, "coverage.json")
    recon = _io.project_file(a.project_path, a.map, "reconstruction.json", "map", "no map to predict against")
    intrinsics = _io.project_file(a.project_path, None, "camera_intrinsics.json", "camera model")
    for f, what in ((a.uncertainty, "uncertainty file"), (a.poses, "pose file")):
        if f is not None:
            _io.project_file(a.project_path, f, None, what)
    tags, _, _ = _io.parseReconstructions(recon)
    rec = TagReconstructor(DetectionResult(), device=a.device)
    rec.setCameraModel(_io.readCameraModel(intrinsics))
    rec.setReconstructedTags(tags)
    if a.poses is not None:
        cameras = read_cameras(a.poses)
    else:
        g = a.grid
        cameras = _engine.grid_poses((g[0], g[3], g[6]), (g[1], g[4], g[7]), (int(g[2]), int(g[5]), int(g[8])), a.axis, a.up)
    given = {k: getattr(a, k) for k in ("sigma_px", "margin_px", "max_view_angle_deg", "min_side_px", "min_tags")
             if getattr(a, k) is not None}
    model = rec.getCameraModel()
    o = _engine.default_predict_options(image_width=int(model.horizontalResolution), image_height=int(model.verticalResolution),
                                        **given)
    if a.correlated:
        joint = read_tag_joint_covariance(a.uncertainty)
        if joint is None:
            raise RuntimeError("Could not find a joint covariance in %s: write it with uncertainty.py --joint." % a.uncertainty)
        report = rec.predictLocalizationAccuracy(cameras, tagJointCovariance=joint, **given)
    else:
        report = rec.predictLocalizationAccuracy(cameras, tagCovariances=read_tag_covariances(a.uncertainty) if a.uncertainty else None,
                                                 **given)
    tree = coverage_tree(_engine._struct_dict(o), report, sorted(tags), covariances=a.covariances)
    if a.correlated:
        tree["map_covariance"] = "joint"
    _io.write_json(out, tree)
    print(summary_line(report, len(tree["tags_never_seen"])) + "; wrote %s!" % out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
