"""Command-line localisation of a multi-camera rig: <project>/reconstruction.json + marker_detections.json + rig.json
-> rig_localization.json, and with --calibrate rig_calibrated.json.

The reference has one CameraModel and no rig.  Here every frame of a rig of rigidly mounted cameras is localised
against the finished map in one device call (vmm_ba_rig_localize), one world->rig pose per frame.

    python -m visual_marker_mapping_amd.rig --project_path DIR [--map FILE] [--rig FILE] [--calibrate] [--output FILE]

rig.json (layout in DESIGN.md section 9) lists the cameras; each has `intrinsics` (a camera_intrinsics.json, relative
to the rig file), optionally `extrinsic` ({rotation: [w, x, y, z], translation: [x, y, z]}, rig->camera) and `images`:
the file names of its images as marker_detections.json knows them, one per frame, null where the camera has none.  The
position in the list is the frame.  When a camera has no extrinsic, all are taken from the per-camera localisation
(engine.rig_extrinsics_start; camera 0 is the rig).  rig_localization.json holds `extrinsics` and `frames`, each frame
as localization.json holds a camera.  --calibrate refines the extrinsics and the rig poses together first
(vmm_ba_rig_calibrate, every camera but 0 by default) and writes rig_calibrated.json next to the output: the rig file
with the refined extrinsics, each with its 6x6 `covariance`, and the report.
"""
import argparse
import os
import sys

import numpy as np

from . import _lib
from . import io as _io
from .tag_reconstructor import TagReconstructor


def read_rig(path):
    """rig.json -> (cameraModels, extrinsics (K, 7) or None, image file names per camera, None for a missing image)."""
    t = _io.read_json(path)
    base = os.path.dirname(os.path.abspath(path))
    models, ext, images = [], [], []
    for cam in _io._children(t, "cameras"):
        models.append(_io.readCameraModel(os.path.join(base, _io._get(cam, "intrinsics", str))))
        e = cam.get("extrinsic")
        ext.append(None if e in (None, "") else np.concatenate([_io._vector(_io._children(e, "rotation"), 4),
                                                                _io._vector(_io._children(e, "translation"), 3)]))
        images.append([None if v in (None, "", "null") else str(v) for v in _io._children(cam, "images")])
    if not models:
        raise RuntimeError("'%s' lists no camera" % path)
    if len({len(v) for v in images}) != 1:
        raise RuntimeError("the cameras of '%s' list different numbers of frames" % path)
    have = [e is not None for e in ext]
    return models, (np.array(ext) if all(have) else None), images


def write_rig(path, intrinsics_files, images, extrinsics=None):
    """Writes rig.json: the intrinsics file, image names (None: missing) and optional extrinsic (7,) of every camera."""
    cams = []
    for c, (intr, names) in enumerate(zip(intrinsics_files, images)):
        cam = {"intrinsics": intr}
        if extrinsics is not None:
            cam["extrinsic"] = _io.pose_tree(None, extrinsics[c])
        cam["images"] = ["null" if n is None else n for n in names]
        cams.append(cam)
    _io.write_json(path, {"cameras": cams})


def rig_tree(report):
    """The property tree of rig_localization.json for the report of computeRigPosesFromFrames."""
    return {"extrinsics": [_io.pose_tree(c, e) for c, e in enumerate(report["extrinsics"])],
            "frames": [_io.localized_pose_tree(f, r) for f, r in enumerate(report["frames"])]}


def calibrated_tree(rig_tree_in, report):
    """The property tree of rig_calibrated.json: the cameras of rig.json with the refined extrinsics and their 6x6
    covariance blocks, and the fields of vmm_ba_rig_calibrate_report."""
    cams = []
    for c, cam in enumerate(_io._children(rig_tree_in, "cameras")):
        e, cov = report["extrinsics"][c], report["covariance"][6 * c:6 * c + 6, 6 * c:6 * c + 6]
        cams.append({"intrinsics": cam["intrinsics"], "extrinsic": dict(_io.pose_tree(None, e), covariance=_io.matrix_tree(cov)),
                     "images": cam["images"]})
    rep = {k: (_lib.CAL_STATUS_NAMES[v] if k == "status" else v) for k, v in report.items()
           if k not in ("extrinsics", "covariance", "rigs", "frames")}
    return {"cameras": cams, "report": rep}


def main(argv=None):
    ap = argparse.ArgumentParser(description="Localises the frames of a multi-camera rig against a finished map")
    ap.add_argument("--project_path", required=True, help="Path to the project (holds marker_detections.json)")
    ap.add_argument("--map", default=None, help="the map (default: <project>/reconstruction.json)")
    ap.add_argument("--rig", default=None, help="the rig description (default: <project>/rig.json)")
    ap.add_argument("--calibrate", action="store_true", help="refine the extrinsics first; writes rig_calibrated.json too")
    ap.add_argument("--output", default=None, help="output file (default: <project>/rig_localization.json)")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    a = ap.parse_args(argv)
    recon = _io.project_file(a.project_path, a.map, "reconstruction.json", "map")
    rig = _io.project_file(a.project_path, a.rig, "rig.json", "rig description")
    detections = _io.project_file(a.project_path, None, "marker_detections.json", "detection file")
    out = a.output or os.path.join(a.project_path, "rig_localization.json")
    tags, _, _ = _io.parseReconstructions(recon)
    det = _io.readDetectionResult(detections)
    models, extrinsics, images = read_rig(rig)
    by_name = {im.filename: int(im.imageId) for im in det.images}
    by_name.update({os.path.basename(im.filename): int(im.imageId) for im in det.images})
    unknown = sorted({n for names in images for n in names if n is not None and n not in by_name})
    if unknown:
        raise RuntimeError("'%s' names images that '%s' does not hold: %s" % (rig, detections, ", ".join(unknown)))
    frames = [[None if names[f] is None else by_name[names[f]] for names in images] for f in range(len(images[0]))]
    rec = TagReconstructor(det, device=a.device)
    rec.setReconstructedTags(tags)
    if a.calibrate:
        report = rec.calibrateRig(frames, models, extrinsics)
        extrinsics = report["extrinsics"]
        calibrated = os.path.join(os.path.dirname(os.path.abspath(out)), "rig_calibrated.json")
        _io.write_json(calibrated, calibrated_tree(_io.read_json(rig), report))
        print("Calibrated the rig (%s, %d trials, rms %.3f -> %.3f px); wrote %s!"
              % (_lib.CAL_STATUS_NAMES[report["status"]], report["trials"], report["initial_rms_px"], report["final_rms_px"],
                 calibrated))
    rigs = rec.computeRigPosesFromFrames(frames, models, extrinsics)
    _io.write_json(out, rig_tree(rec.lastRigLocalizationReport))
    print("Localised %d of %d frames of a rig of %d cameras; wrote %s!" % (len(rigs), len(frames), len(models), out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
