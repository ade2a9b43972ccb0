"""Command-line calibration step: a finished map + detections + a starting camera model -> a calibrated camera model.

The reference has no calibration step: it reads camera_intrinsics.json as given (src/CameraUtilities.cpp:45-66).  A
finished map of tags of known size is a calibration target; this step refines the nine numbers of the camera model
together with one pose per image on the device (vmm_ba_calibrate), the map held fixed.

    python -m visual_marker_mapping_amd.calibration --project_path DIR [--map FILE] [--intrinsics FILE] [--output FILE]
                                                    [--option NAME=VALUE ...]

Reads <project>/reconstruction.json (--map), <project>/marker_detections.json and the starting
<project>/camera_intrinsics.json (--intrinsics); writes <project>/camera_intrinsics_calibrated.json (--output) in the
format of camera_intrinsics.json and, next to it, calibration.json: the report of vmm_ba_calibrate, the parameters in the
order fx, fy, cx, cy, k1, k2, p1, p2, k3, their standard deviations and the row-major 9x9 covariance
({rows, cols, coefficents}).  --option sets a field of vmm_ba_calibrate_options (loc_NAME: of the initial localisation),
e.g. --option refine_mask=15 --option inlier_px=4.
"""
import argparse
import os
import sys

from . import _lib
from . import io as _io
from .tag_reconstructor import TagReconstructor

PARAMETER_NAMES = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")


def parameters_tree(report):
    """The tail calibration.json and selfcalibration.json share: the nine parameters with their names, standard
    deviations and 9x9 covariance."""
    return {"parameter_names": list(PARAMETER_NAMES), "parameters": [float(v) for v in report["intrinsics"]],
            "standard_deviations": [float(v) for v in report["std"]], "covariance": _io.matrix_tree(report["covariance"])}


def calibration_tree(report):
    """The property tree of calibration.json for the report of TagReconstructor.refineCameraModel."""
    tree = {"status": _lib.CAL_STATUS_NAMES[report["status"]]}
    tree.update((k, int(report[k])) for k in ("trials", "accepted", "passes", "n_images_used", "n_obs_used"))
    tree.update((k, float(report[k])) for k in ("initial_cost", "final_cost", "initial_rms_px", "final_rms_px", "time_s"))
    return dict(tree, **parameters_tree(report))


def main(argv=None):
    ap = argparse.ArgumentParser(description="Calibrates a camera against a finished map")
    ap.add_argument("--project_path", required=True, help="Path to the project (holds reconstruction.json)")
    ap.add_argument("--map", default=None, help="map file (default: <project>/reconstruction.json)")
    ap.add_argument("--intrinsics", default=None, help="starting camera model (default: <project>/camera_intrinsics.json)")
    ap.add_argument("--detections", default=None, help="detection file (default: <project>/marker_detections.json)")
    ap.add_argument("--output", default=None, help="output file (default: <project>/camera_intrinsics_calibrated.json)")
    ap.add_argument("--option", action="append", default=[], metavar="NAME=VALUE",
                    help="a field of vmm_ba_calibrate_options (loc_NAME: of the initial localisation); may be repeated")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    a = ap.parse_args(argv)
    options = {}
    for item in a.option:
        name, sep, value = item.partition("=")
        if not sep:
            ap.error("--option takes NAME=VALUE, not %r" % item)
        options[name] = float(value) if name.endswith(("_px", "huber_a")) else int(value, 0)
    recon = _io.project_file(a.project_path, a.map, "reconstruction.json", "map", "no map to calibrate against")
    detections = _io.project_file(a.project_path, a.detections, "marker_detections.json", "detection file")
    intrinsics = _io.project_file(a.project_path, a.intrinsics, "camera_intrinsics.json", "camera model file")
    out = a.output or os.path.join(a.project_path, "camera_intrinsics_calibrated.json")
    tags, _, _ = _io.parseReconstructions(recon)
    det = _io.readDetectionResult(detections)
    rec = TagReconstructor(det, device=a.device)
    rec.setCameraModel(_io.readCameraModel(intrinsics))
    rec.setReconstructedTags(tags)
    report = rec.refineCameraModel(**options)
    _io.writeCameraModel(rec.getCameraModel(), out)
    side = os.path.join(os.path.dirname(os.path.abspath(out)), "calibration.json")
    _io.write_json(side, calibration_tree(report))
    print("Calibration %s: %d images, %d observations, rms %.4g px -> %.4g px; wrote %s and %s!"
          % (_lib.CAL_STATUS_NAMES[report["status"]], report["n_images_used"], report["n_obs_used"],
             report["initial_rms_px"], report["final_rms_px"], out, side))
    return 0


if __name__ == "__main__":
    sys.exit(main())
