"""Command-line map check: <project>/reconstruction.json + marker_detections.json of fresh images -> map_check.json.

Tags get knocked, re-glued and replaced.  This step answers "which tags of my map are no longer where the map says?"
without re-mapping: the fresh images are localised against the finished map (vmm_ba_localize), every map tag they see is
located from those cameras (vmm_ba_locate_tags), and each located pose is compared with the map's in units of its own
covariance (TagReconstructor.checkMap, which also says what the statistic ignores).  The reference has no such
executable.

    python -m visual_marker_mapping_amd.map_check --project_path DIR [--map FILE] [--detections FILE] [--sigma_px S]
                                                  [--chi2 T] [--min_views N] [--output FILE]

map_check.json (layout in DESIGN.md section 9) holds `rounds`, `sigma_px`, `chi2_threshold`, `tags` (per checked tag the
located pose as reconstruction.json holds one, `status`, `num_views`, `num_inlier_views`, `rms_px`, `covariance`
({rows, cols, coefficents}: sigma_px^2 (tag_cov + tag_cov_cams), row-major 6x6 in tangent order), `delta`,
`mahalanobis2`, `max_corner_displacement` in metres and `moved`), `skipped_tags` (seen in too few images) and `images`
(per image the localisation's status).  One line is printed per moved tag; the exit status is 0 whether or not
something moved.
"""
import argparse
import os
import sys

from . import _lib
from . import io as _io
from .tag_reconstructor import TagReconstructor


def map_check_tree(report):
    """The property tree of map_check.json for the report of TagReconstructor.checkMap."""
    tags = []
    for t in sorted(report["tags"]):
        r = report["tags"][t]
        tags.append(dict(_io.pose_tree(t, r["pose"]), status=_lib.LOC_STATUS_NAMES[r["status"]], num_views=int(r["n_obs"]),
                         num_inlier_views=int(r["n_inlier_obs"]), rms_px=float(r["rms_px"]),
                         covariance=_io.matrix_tree(r["covariance"]), delta=[float(v) for v in r["delta"]],
                         mahalanobis2=float(r["mahalanobis2"]),
                         max_corner_displacement=float(r["max_corner_displacement"]), moved=bool(r["moved"])))
    return {"rounds": int(report["rounds"]), "sigma_px": float(report["sigma_px"]),
            "chi2_threshold": float(report["chi2_threshold"]), "tags": tags,
            "skipped_tags": [int(t) for t in report["skipped"]],
            "images": [{"id": int(i), "status": _lib.LOC_STATUS_NAMES[report["images"][i]]} for i in sorted(report["images"])]}


def main(argv=None):
    ap = argparse.ArgumentParser(description="Checks a finished map against detections of fresh images: which tags moved?")
    ap.add_argument("--project_path", required=True, help="Path to the project (holds reconstruction.json)")
    ap.add_argument("--map", default=None, help="map file (default: <project>/reconstruction.json)")
    ap.add_argument("--detections", default=None, help="detection file (default: <project>/marker_detections.json)")
    ap.add_argument("--sigma_px", type=float, default=1.0, help="standard deviation of a detected corner in pixels")
    ap.add_argument("--chi2", type=float, default=22.458, help="threshold on the squared Mahalanobis distance (6 dof)")
    ap.add_argument("--min_views", type=int, default=2, help="localised images a tag must be seen in to be checked")
    ap.add_argument("--output", default=None, help="output file (default: <project>/map_check.json)")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    a = ap.parse_args(argv)
    recon = _io.project_file(a.project_path, a.map, "reconstruction.json", "map", None if a.map else "no map to check")
    detections = _io.project_file(a.project_path, a.detections, "marker_detections.json", "detection file")
    out = a.output or os.path.join(a.project_path, "map_check.json")
    tags, _, model = _io.parseReconstructions(recon)
    rec = TagReconstructor(_io.readDetectionResult(detections), device=a.device)
    rec.setCameraModel(model)
    rec.setReconstructedTags(tags)
    report = rec.checkMap(sigma_px=a.sigma_px, chi2_threshold=a.chi2, min_views=a.min_views)
    _io.write_json(out, map_check_tree(report))
    for t in report["moved"]:
        r = report["tags"][t]
        print("tag %d moved: mahalanobis2 %.4g, largest corner displacement %.4g m" % (t, r["mahalanobis2"],
                                                                                      r["max_corner_displacement"]))
    print("Checked %d of %d tags in %d round(s), %d moved; wrote %s!" % (len(report["tags"]), len(tags), report["rounds"],
                                                                        len(report["moved"]), out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
