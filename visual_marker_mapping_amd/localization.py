"""Command-line localisation step: <project>/reconstruction.json + marker_detections.json -> localization.json.

The reference has no such executable; its library member for the job is
TagReconstructor::computeRelativeCameraPoseFromImg (src/TagReconstructor.cpp:280-312), one image at a time.  Here
every image of the detection file is localised against the finished map in one device call (vmm_ba_localize).

    python -m visual_marker_mapping_amd.localization --project_path DIR [--detections FILE] [--output FILE] \\
        [--uncertainty FILE]

localization.json (layout in DESIGN.md section 9) holds `reconstructed_cameras` as reconstruction.json does, every
camera extended by `status`, `num_observations`, `num_inlier_observations`, `rms_px` and `covariance`
({rows, cols, coefficents}: the row-major 6x6 covariance of the pose in tangent order, translation then rotation).
`--uncertainty` names a reconstruction_uncertainty.json written with `uncertainty.py --joint`: every camera then also gets
`map_covariance` (the part the map's own uncertainty adds, the tags' correlations included; one
vmm_ba_predict_localization_joint call over the inlier tags of every image) and `sigma_pos_m` / `sigma_rot_rad`, the
totals of the pixel part at sigma_px = 1 and the map part.
"""
import argparse
import os
import sys

from . import io as _io
from .tag_reconstructor import TagReconstructor
from .uncertainty import read_tag_joint_covariance


def localization_tree(ids, report):
    """The property tree of localization.json for the per-image report of computeRelativeCameraPosesFromImgs; with the
    keys of localizationMapCovariances where the report has them."""
    out = []
    for i in ids:
        entry = _io.localized_pose_tree(i, report[i])
        if "map_covariance" in report[i]:
            entry.update(map_covariance=_io.matrix_tree(report[i]["map_covariance"]), sigma_pos_m=float(report[i]["sigma_pos_m"]),
                         sigma_rot_rad=float(report[i]["sigma_rot_rad"]))
        out.append(entry)
    return {"reconstructed_cameras": out}


def main(argv=None):
    ap = argparse.ArgumentParser(description="Localises the images of a detection file against a finished map")
    ap.add_argument("--project_path", required=True, help="Path to the project (holds reconstruction.json)")
    ap.add_argument("--detections", default=None, help="detection file (default: <project>/marker_detections.json)")
    ap.add_argument("--output", default=None, help="output file (default: <project>/localization.json)")
    ap.add_argument("--uncertainty", default=None,
                    help="reconstruction_uncertainty.json written with --joint: adds the map's part of every covariance")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    a = ap.parse_args(argv)
    recon = _io.project_file(a.project_path, None, "reconstruction.json", "map", "no map to localise against")
    detections = _io.project_file(a.project_path, a.detections, "marker_detections.json", "detection file")
    out = a.output or os.path.join(a.project_path, "localization.json")
    joint = None
    if a.uncertainty is not None:
        joint = read_tag_joint_covariance(_io.project_file(a.project_path, a.uncertainty, None, "uncertainty file"))
        if joint is None:
            raise RuntimeError("Could not find a joint covariance in %s: write it with uncertainty.py --joint." % a.uncertainty)
    tags, _, model = _io.parseReconstructions(recon)
    det = _io.readDetectionResult(detections)
    rec = TagReconstructor(det, device=a.device)
    rec.setCameraModel(model)
    rec.setReconstructedTags(tags)
    cams = rec.computeRelativeCameraPosesFromImgs()
    if joint is not None:
        rec.localizationMapCovariances(joint)
    ids = sorted(rec.lastLocalizationReport)
    _io.write_json(out, localization_tree(ids, rec.lastLocalizationReport))
    print("Localised %d of %d images; wrote %s!" % (len(cams), len(ids), out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
