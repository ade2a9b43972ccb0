"""Command-line map extension: a finished reconstruction.json + the detections of NEW images -> reconstruction_extended.json.

The reference has no such executable: its only way to add images to a map is to run the whole reconstruction again,
which moves every tag.  Here every tag of the map is held constant on the device (vmm_ba_set_constant_poses, Ceres'
SetParameterBlockConstant on more than one block), the new tags and the new images' cameras grow outward from the map
tags the new images see (vmm_ba_initialize), and the reference's closing bundle adjustments
(src/TagReconstructor.cpp:271-277) run with the map held: TagReconstructor.extendReconstruction.

    python -m visual_marker_mapping_amd.extension --project_path DIR [--map FILE] [--output FILE]

DIR holds camera_intrinsics.json and marker_detections.json of the new images; --map defaults to
DIR/reconstruction.json, --output to DIR/reconstruction_extended.json.  The output has the reconstruction format
(io.exportReconstructions): ALL tags of the map, their rotation, translation, width and height exactly as the map
file has them, the new tags, and the cameras of the new images.  The map's own cameras are NOT carried over: their
image ids belong to the detection file the map was built from, not to this one.
"""
import argparse
import os
import sys

from . import io as _io
from .tag_reconstructor import TagReconstructor


def main(argv=None):
    ap = argparse.ArgumentParser(description="Extends a finished map with the images of a detection file")
    ap.add_argument("--project_path", required=True,
                    help="Path to the project (camera_intrinsics.json, marker_detections.json of the new images)")
    ap.add_argument("--map", default=None, help="the finished map (default: <project>/reconstruction.json)")
    ap.add_argument("--output", default=None, help="output file (default: <project>/reconstruction_extended.json)")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    a = ap.parse_args(argv)
    recon = _io.project_file(a.project_path, a.map, "reconstruction.json", "map", "no map to extend")
    detections = _io.project_file(a.project_path, None, "marker_detections.json", None)
    intrinsics = _io.project_file(a.project_path, None, "camera_intrinsics.json", None)
    out = a.output or os.path.join(a.project_path, "reconstruction_extended.json")
    tags, _, _ = _io.parseReconstructions(recon)
    camera_model = _io.readCameraModel(intrinsics)
    rec = TagReconstructor(_io.readDetectionResult(detections), device=a.device)
    rec.setCameraModel(camera_model)
    rec.setReconstructedTags(tags)
    rec.extendReconstruction(os.cpu_count() or 4)
    new_tags = sorted(set(rec.getReconstructedTags()) - set(tags))
    _io.exportReconstructions(out, rec.getReconstructedTags(), rec.getReconstructedCameras(), camera_model)
    print("Extended the map of %d tags by %d tags and %d cameras; wrote %s!"
          % (len(tags), len(new_tags), len(rec.getReconstructedCameras()), out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
