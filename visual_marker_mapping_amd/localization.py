"""Command-line localisation step: <project>/reconstruction.json + marker_detections.json -> localization.json.

The reference has no such executable; its library member for the job is
TagReconstructor::computeRelativeCameraPoseFromImg (src/TagReconstructor.cpp:280-312), one image at a time.  Here
every image of the detection file is localised against the finished map in one device call (vmm_ba_localize).

    python -m visual_marker_mapping_amd.localization --project_path DIR [--detections FILE] [--output FILE]

localization.json (layout in DESIGN.md section 9) holds `reconstructed_cameras` as reconstruction.json does, every
camera extended by `status`, `num_observations`, `num_inlier_observations`, `rms_px` and `covariance`
({rows, cols, coefficents}: the row-major 6x6 covariance of the pose in tangent order, translation then rotation).
"""
import argparse
import os
import sys

from . import _lib
from . import io as _io
from .tag_reconstructor import TagReconstructor


def localization_tree(ids, report):
    """The property tree of localization.json for the per-image report of computeRelativeCameraPosesFromImgs."""
    cams = []
    for i in ids:
        r = report[i]
        cams.append({"id": int(i), "rotation": [float(v) for v in r["pose"][:4]],
                     "translation": [float(v) for v in r["pose"][4:]],
                     "status": _lib.LOC_STATUS_NAMES[r["status"]],
                     "num_observations": int(r["n_obs"]),
                     "num_inlier_observations": int(r["n_inlier_obs"]),
                     "rms_px": float(r["rms_px"]),
                     "covariance": {"rows": 6, "cols": 6,
                                    "coefficents": [float(v) for v in r["covariance"].reshape(-1)]}})
    return {"reconstructed_cameras": cams}


def main(argv=None):
    ap = argparse.ArgumentParser(description="Localises the images of a detection file against a finished map")
    ap.add_argument("--project_path", required=True, help="Path to the project (holds reconstruction.json)")
    ap.add_argument("--detections", default=None, help="detection file (default: <project>/marker_detections.json)")
    ap.add_argument("--output", default=None, help="output file (default: <project>/localization.json)")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    a = ap.parse_args(argv)
    recon = os.path.join(a.project_path, "reconstruction.json")
    detections = a.detections or os.path.join(a.project_path, "marker_detections.json")
    out = a.output or os.path.join(a.project_path, "localization.json")
    if not os.path.isfile(recon):
        raise FileNotFoundError("no map to localise against: '%s' does not exist (run the mapping step first: "
                                "python -m visual_marker_mapping_amd.mapping --project_path %s)" % (recon, a.project_path))
    if not os.path.isfile(detections):
        raise FileNotFoundError("detection file '%s' does not exist" % detections)
    tags, _, model = _io.parseReconstructions(recon)
    det = _io.readDetectionResult(detections)
    rec = TagReconstructor(det, device=a.device)
    rec.setCameraModel(model)
    rec.setReconstructedTags(tags)
    cams = rec.computeRelativeCameraPosesFromImgs()
    ids = sorted(rec.lastLocalizationReport)
    _io.write_json(out, localization_tree(ids, rec.lastLocalizationReport))
    print("Localised %d of %d images; wrote %s!" % (len(cams), len(ids), out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
