"""Command-line uncertainty step: how well a finished map is known.

    python -m visual_marker_mapping_amd.uncertainty --project_path DIR [--map FILE] [--output FILE] [--joint]

Reads <project>/camera_intrinsics.json, <project>/marker_detections.json and the map (default
<project>/reconstruction.json), builds the bundle-adjustment problem of the map at its poses (no solve) and writes
reconstruction_uncertainty.json: the 6x6 covariance of every reconstructed tag and camera in tangent order (translation,
then rotation), conditional on the origin tag, from one vmm_ba_covariance_blocks call.  The reference reports the
tags' translation blocks only (src/TagReconstructor.cpp:744-783).

    {"origin_tag_id": .., "robustify": ..,
     "reconstructed_tags":    [{"id", "sigma": [6 square roots of the diagonal],
                                "covariance": {"rows": 6, "cols": 6, "coefficents": [36 row-major values]}}],
     "reconstructed_cameras": [the same]}

(the dynamic-matrix form of SURVEY.md Appendix B, spelling included, as localization.json uses it).  `--joint` adds the
tags' joint covariance, cross blocks included, from one more vmm_ba_covariance_blocks call:

     "tag_joint_covariance": {"tag_ids": [T ids], "covariance": {"rows": 6T, "cols": 6T, "coefficents": [...]}}

with rows 6 i .. 6 i + 5 those of tag_ids[i]: what coverage.py --correlated and localization.py --uncertainty read
(read_tag_joint_covariance).
"""
import argparse
import os
import sys

import numpy as np

from . import io as _io
from .tag_reconstructor import TagReconstructor


def uncertainty_tree(origin_tag_id, robustify, tag_cov, cam_cov, tag_joint=None):
    """The property tree of reconstruction_uncertainty.json from plain values: tag_cov and cam_cov map an id to its
    6x6 covariance.  Entries are written by ascending id.  tag_joint: (tag ids, (T, T, 6, 6)) or None."""
    def entries(cov):
        out = []
        for i in sorted(cov):
            m = np.asarray(cov[i], np.float64).reshape(6, 6)
            out.append({"id": int(i), "sigma": [float(v) for v in np.sqrt(np.diag(m))], "covariance": _io.matrix_tree(m)})
        return out
    tree = {"origin_tag_id": int(origin_tag_id), "robustify": bool(robustify),
            "reconstructed_tags": entries(tag_cov), "reconstructed_cameras": entries(cam_cov)}
    if tag_joint is not None:
        ids, joint = tag_joint
        T = len(ids)
        joint = np.asarray(joint, np.float64)
        if joint.size != 36 * T * T:
            raise ValueError("the joint covariance does not have one 6x6 block per pair of its %d tag ids" % T)
        dense = joint.reshape(T, T, 6, 6).transpose(0, 2, 1, 3).reshape(6 * T, 6 * T)
        tree["tag_joint_covariance"] = {"tag_ids": [int(t) for t in ids], "covariance": _io.matrix_tree(dense)}
    return tree


def write_uncertainty(path, origin_tag_id, robustify, tag_cov, cam_cov, tag_joint=None):
    """Writes reconstruction_uncertainty.json (every scalar a quoted string, like the reference's output files)."""
    _io.write_json(path, uncertainty_tree(origin_tag_id, robustify, tag_cov, cam_cov, tag_joint))


def read_tag_joint_covariance(path):
    """(tag ids, (T, T, 6, 6)) from the `tag_joint_covariance` of a reconstruction_uncertainty.json written with --joint;
    None when the file has none."""
    tree = _io.read_json(path)
    if not isinstance(tree, dict) or "tag_joint_covariance" not in tree:
        return None
    pt = tree["tag_joint_covariance"]
    ids = [int(t) for t in _io._children(pt, "tag_ids")]
    T = len(ids)
    dense = _io.matrixFromPropertyTree(pt["covariance"], 6 * T, 6 * T)
    return ids, np.ascontiguousarray(dense.reshape(T, 6, T, 6).transpose(0, 2, 1, 3))


def main(argv=None):
    ap = argparse.ArgumentParser(description="6x6 covariance of every tag and camera of a finished map")
    ap.add_argument("--project_path", required=True, help="Path to the project (holds camera_intrinsics.json, "
                    "marker_detections.json and the map)")
    ap.add_argument("--map", default=None, help="map file (default: <project>/reconstruction.json)")
    ap.add_argument("--output", default=None, help="output file (default: <project>/reconstruction_uncertainty.json)")
    ap.add_argument("--start_tag_id", type=int, default=-1,
                    help="Id of the marker in the origin of the model (default: the lowest id of the map)")
    ap.add_argument("--robustify", action="store_true", help="apply the Huber loss of the mapping step to J")
    ap.add_argument("--joint", action="store_true", help="also write the tags' joint covariance, cross blocks included")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    a = ap.parse_args(argv)
    recon = _io.project_file(a.project_path, a.map, "reconstruction.json", None)
    intrinsics = _io.project_file(a.project_path, None, "camera_intrinsics.json", None)
    detections = _io.project_file(a.project_path, None, "marker_detections.json", None)
    out = a.output or os.path.join(a.project_path, "reconstruction_uncertainty.json")
    tags, cams, _ = _io.parseReconstructions(recon)
    rec = TagReconstructor(_io.readDetectionResult(detections), device=a.device)
    rec.setCameraModel(_io.readCameraModel(intrinsics))
    rec.setReconstructedTags(tags)
    rec.setReconstructedCameras(cams)
    origin = a.start_tag_id if a.start_tag_id != -1 else min(tags)
    if origin not in tags:
        raise RuntimeError("Could not use tag with id %d as origin tag, because it is not in the map." % origin)
    rec.setOriginTagId(origin)
    cov = rec.computePoseCovariances(robustify=a.robustify, jointTags=a.joint)
    rec.close()
    write_uncertainty(out, origin, a.robustify, cov["tags"], cov["cameras"], cov.get("tag_joint") if a.joint else None)
    print("Covariance of %d tags and %d cameras; wrote %s!" % (len(cov["tags"]), len(cov["cameras"]), out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
