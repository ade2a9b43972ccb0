"""Command-line self-calibration step: a finished reconstruction + detections + a rough camera model -> the map, the
cameras and the camera model at one joint optimum.

The reference takes camera_intrinsics.json as given (src/CameraUtilities.cpp:45-66), and the calibration step
(calibration.py) refines the model against a map held fixed -- a map that was built with the model it is meant to
correct.  This step runs the bundle adjustment over cameras, tags AND the nine numbers of the camera model on the device
(vmm_ba_solve_selfcal) and reports the covariance of the model with every pose marginalised.

    python -m visual_marker_mapping_amd.selfcalibration --project_path DIR [--map FILE] [--intrinsics FILE]
                                                        [--refine_mask N] [--output FILE]

Reads <project>/reconstruction.json (--map: tags and cameras), <project>/marker_detections.json and the starting model
<project>/camera_intrinsics.json (--intrinsics; default when the file is missing: the model stored in the map file).
Writes <project>/reconstruction_selfcalibrated.json (--output) in the format of reconstruction.json and, next to it,
camera_intrinsics_calibrated.json in the format of camera_intrinsics.json and selfcalibration.json: the report of
vmm_ba_solve_selfcal, the parameters in the order fx, fy, cx, cy, k1, k2, p1, p2, k3, their standard deviations and the
row-major 9x9 covariance ({rows, cols, coefficents}).  --refine_mask: bit i set = parameter i is refined (default 0x1FF,
all nine; 15 refines fx, fy, cx, cy and keeps the distortion).
"""
import argparse
import os
import sys

from . import _lib
from . import io as _io
from .calibration import parameters_tree
from .tag_reconstructor import TagReconstructor


def selfcalibration_tree(report):
    """The property tree of selfcalibration.json for TagReconstructor.lastSelfCalibrationReport."""
    tree = {"status": _lib.CAL_STATUS_NAMES[report["status"]]}
    tree.update((k, int(report[k])) for k in ("outer_iterations", "accepted", "inner_lm_iterations"))
    tree.update((k, float(report[k])) for k in ("initial_cost", "final_cost", "time_s"))
    return dict(tree, **parameters_tree(report))


def main(argv=None):
    ap = argparse.ArgumentParser(description="Bundle adjustment of a finished reconstruction with the camera model refined")
    ap.add_argument("--project_path", required=True, help="Path to the project (holds reconstruction.json)")
    ap.add_argument("--map", default=None, help="reconstruction file (default: <project>/reconstruction.json)")
    ap.add_argument("--intrinsics", default=None, help="starting camera model (default: <project>/camera_intrinsics.json)")
    ap.add_argument("--detections", default=None, help="detection file (default: <project>/marker_detections.json)")
    ap.add_argument("--refine_mask", type=lambda v: int(v, 0), default=0x1FF,
                    help="bit i set = parameter i of fx, fy, cx, cy, k1, k2, p1, p2, k3 is refined (default 0x1FF)")
    ap.add_argument("--output", default=None, help="output file (default: <project>/reconstruction_selfcalibrated.json)")
    ap.add_argument("--start_tag_id", type=int, default=-1, help="origin tag, held constant (default: the lowest id of the map)")
    ap.add_argument("--max_iterations", type=int, default=1500, help="iterations of every inner bundle adjustment")
    ap.add_argument("--robust", action="store_true", help="Huber loss on every corner, as the mapping step's bundle adjustments")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    a = ap.parse_args(argv)
    if not 0 <= a.refine_mask <= 0x1FF:
        ap.error("--refine_mask must lie in [0, 0x1FF]")
    recon = _io.project_file(a.project_path, a.map, "reconstruction.json", "reconstruction", "no reconstruction to refine")
    detections = _io.project_file(a.project_path, a.detections, "marker_detections.json", "detection file")
    # the default model file may be missing (then the map's model is the start); one that was named may not
    intrinsics = (_io.project_file(a.project_path, a.intrinsics, None, "camera model file") if a.intrinsics
                  else os.path.join(a.project_path, "camera_intrinsics.json"))
    out = a.output or os.path.join(a.project_path, "reconstruction_selfcalibrated.json")
    tags, cams, map_model = _io.parseReconstructions(recon)
    if not tags or not cams:
        raise RuntimeError("'%s' holds no reconstructed tags or no reconstructed cameras" % recon)
    det = _io.readDetectionResult(detections)
    rec = TagReconstructor(det, device=a.device)
    rec.setCameraModel(_io.readCameraModel(intrinsics) if os.path.isfile(intrinsics) else map_model)
    rec.setReconstructedTags(tags)
    rec.setReconstructedCameras(cams)
    rec.setOriginTagId(a.start_tag_id if a.start_tag_id != -1 else min(tags))
    rec.doBundleAdjustment(a.max_iterations, 1, a.robust, False, refineCameraModel=True, refine_mask=a.refine_mask)
    report = rec.lastSelfCalibrationReport
    if report is None:
        raise RuntimeError("nothing to adjust: no detection links a reconstructed camera to a reconstructed tag")
    rec.close()
    side = os.path.dirname(os.path.abspath(out))
    model_file = os.path.join(side, "camera_intrinsics_calibrated.json")
    report_file = os.path.join(side, "selfcalibration.json")
    _io.exportReconstructions(out, rec.getReconstructedTags(), rec.getReconstructedCameras(), rec.getCameraModel())
    _io.writeCameraModel(rec.getCameraModel(), model_file)
    _io.write_json(report_file, selfcalibration_tree(report))
    print("Self-calibration %s: %d outer iterations (%d accepted), cost %.6g -> %.6g; wrote %s, %s and %s!"
          % (_lib.CAL_STATUS_NAMES[report["status"]], report["outer_iterations"], report["accepted"],
             report["initial_cost"], report["final_cost"], out, model_file, report_file))
    return 0


if __name__ == "__main__":
    sys.exit(main())
