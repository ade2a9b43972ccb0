"""The output files of the step modules, byte for byte: every `*_tree` function, write_uncertainty and write_rig on small
hand-made reports, written with io.write_json and compared with the text under tests/golden/trees/; and the readers
(read_rig, read_cameras, read_camera_covariances) on those files.

The golden files were written by the modules of the commit BEFORE the step modules were folded onto io.matrix_tree,
io.pose_tree, io.localized_pose_tree and calibration.parameters_tree (21a96e7), never by the code under test.  The
one-off generator is this file run against that commit's package:

    git worktree add ../before 21a96e7
    PYTHONPATH=../before python tests/test_json_trees_cpu.py

The reports below carry no `reserved` key: engine.rig_calibrate stopped returning it with the fold, and 21a96e7's
rig.calibrated_tree filtered it out, so rig_calibrated.json is the same text either way.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trees")


def _matrix(n, scale):
    """n x n, every entry different, none with a short decimal expansion."""
    return (np.arange(float(n * n)).reshape(n, n) + 1.0) * scale / 7.0


def _pose(k):
    q = np.array([0.9, 0.1 * k, -0.2, 0.3]) / np.linalg.norm([0.9, 0.1 * k, -0.2, 0.3])
    return np.concatenate([q, [0.25 * k, -1.5, 2.0 / 3.0]])


def _item(status, k):
    """One image's / frame's entry as TagReconstructor's localisation reports hold it."""
    return dict(status=status, n_obs=5 + k, n_inlier_obs=4 * (status == 0), trials=7, rms_px=0.3 / (k + 1), cost=1.25,
                pose=_pose(k), covariance=_matrix(6, 1e-6 * (k + 1)), observations=[0, 1, 2], inliers=np.array([1, 1, 0], bool))


def _model_report(**head):
    return dict(head, intrinsics=np.array([8075.5, 8083.25, 3016.0, 1996.0, -0.186, 0.37, -2.9e-4, 4.2e-4, 0.057]),
                covariance=_matrix(9, 1e-3), std=np.sqrt(np.diag(_matrix(9, 1e-3))))


RIG_IN = {"cameras": [{"intrinsics": "camera_0.json", "images": ["f0_c0.jpg", "f1_c0.jpg"]},
                      {"intrinsics": "camera_1.json", "images": ["f0_c1.jpg", "null"]}]}


def trees():
    """File name -> property tree, from whatever visual_marker_mapping_amd is importable."""
    from visual_marker_mapping_amd import calibration, localization, rig, selfcalibration, triangulation, uncertainty
    frames = [_item(0, 0), _item(3, 1)]   # one ok, one too_few_inliers
    ext = np.stack([_pose(0), _pose(2)])
    rig_report = dict(status=3, trials=100, accepted=41, passes=3, n_frames_used=1, n_obs_used=9, cams_refined=2,
                      initial_cost=12.5, final_cost=1.0 / 3.0, initial_rms_px=2.25, final_rms_px=0.4, time_s=0.125,
                      extrinsics=ext, covariance=_matrix(12, 1e-5), rigs={}, frames=frames)
    points = {5: dict(point=np.array([0.1, -0.2, 3.0]), covariance=_matrix(3, 1e-4), covariance_cameras=_matrix(3, 2e-5),
                      status=0, n_obs=4, n_inlier_obs=3, rms_px=0.7, inliers={}),
              2: dict(point=np.zeros(3), covariance=np.zeros((3, 3)), covariance_cameras=np.zeros((3, 3)),
                      status=1, n_obs=1, n_inlier_obs=0, rms_px=0.0, inliers={})}
    geometry = {4: dict(corners=_matrix(4, 0.1)[:, :3], width=0.1601, height=0.1599, width_ratio=1.000625,
                        height_ratio=0.999375, out_of_plane=2.5e-4, model_gap=1.0 / 900.0, status=0),
                1: dict(corners=np.zeros((4, 3)), width=0.0, height=0.0, width_ratio=0.0, height_ratio=0.0,
                        out_of_plane=0.0, model_gap=0.16, status=3)}
    return {
        "localization.json": localization.localization_tree([3, 11], {11: frames[1], 3: frames[0]}),
        "rig_localization.json": rig.rig_tree(dict(extrinsics=ext, frames=frames)),
        "rig_calibrated.json": rig.calibrated_tree(RIG_IN, rig_report),
        "calibration.json": calibration.calibration_tree(_model_report(
            status=0, trials=17, accepted=12, passes=3, n_images_used=2, n_obs_used=11, initial_cost=40.5, final_cost=2.0 / 3.0,
            initial_rms_px=3.5, final_rms_px=0.45, time_s=0.25)),
        "selfcalibration.json": selfcalibration.selfcalibration_tree(_model_report(
            status=2, outer_iterations=9, accepted=6, inner_lm_iterations=57, initial_cost=3.75, final_cost=1.0 / 7.0,
            time_s=1.5)),
        "triangulation.json": triangulation.triangulation_tree(points),
        "tag_geometry.json": triangulation.tag_geometry_tree(geometry),
        "reconstruction_uncertainty.json": uncertainty.uncertainty_tree(
            7, True, {7: np.zeros((6, 6)), 2: _matrix(6, 1e-7)}, {1: _matrix(6, 3e-6), 0: _matrix(6, 2e-6)}),
    }


def _write_all(directory):
    from visual_marker_mapping_amd import io, rig
    for name, tree in trees().items():
        io.write_json(os.path.join(directory, name), tree)
    rig.write_rig(os.path.join(directory, "rig.json"), ["camera_0.json", "camera_1.json"],
                  [["f0_c0.jpg", "f1_c0.jpg"], ["f0_c1.jpg", None]], np.stack([_pose(0), _pose(2)]))
    return sorted(trees()) + ["rig.json"]


def test_every_tree_is_written_as_the_golden_text(tmp_path):
    names = _write_all(str(tmp_path))
    assert sorted(names) == sorted(os.listdir(GOLDEN))
    for name in names:
        with open(os.path.join(GOLDEN, name)) as f, open(os.path.join(str(tmp_path), name)) as g:
            assert g.read() == f.read(), name


def test_write_uncertainty_writes_the_tree(tmp_path):
    from visual_marker_mapping_amd import uncertainty
    out = os.path.join(str(tmp_path), "u.json")
    uncertainty.write_uncertainty(out, 7, True, {7: np.zeros((6, 6)), 2: _matrix(6, 1e-7)},
                                  {1: _matrix(6, 3e-6), 0: _matrix(6, 2e-6)})
    with open(os.path.join(GOLDEN, "reconstruction_uncertainty.json")) as f, open(out) as g:
        assert g.read() == f.read()


def test_readers_take_the_golden_files(tmp_path):
    from visual_marker_mapping_amd import io, rig, triangulation
    # localization.json: the image that is not "ok" is skipped by both readers
    loc = os.path.join(GOLDEN, "localization.json")
    cams = triangulation.read_cameras(loc)
    assert sorted(cams) == [3] and np.concatenate([cams[3].q, cams[3].t]).tobytes() == _pose(0).tobytes()
    cov = triangulation.read_camera_covariances(loc)
    assert sorted(cov) == [3] and cov[3].tobytes() == _matrix(6, 1e-6).tobytes()
    # reconstruction_uncertainty.json has no status: every camera counts
    cov = triangulation.read_camera_covariances(os.path.join(GOLDEN, "reconstruction_uncertainty.json"))
    assert sorted(cov) == [0, 1] and cov[1].tobytes() == _matrix(6, 3e-6).tobytes()
    # without ok_only the failed image is a camera like any other (what parseReconstructions does)
    assert sorted(io.camerasFromPropertyTree(io.read_json(loc))) == [3, 11]
    # rig.json, next to the camera models it names
    model = io.readCameraModel(os.path.join(os.path.dirname(GOLDEN), "readme_camera_intrinsics.json"))
    for c in range(2):
        io.writeCameraModel(model, os.path.join(str(tmp_path), "camera_%d.json" % c))
    with open(os.path.join(GOLDEN, "rig.json")) as f, open(os.path.join(str(tmp_path), "rig.json"), "w") as g:
        g.write(f.read())
    models, ext, images = rig.read_rig(os.path.join(str(tmp_path), "rig.json"))
    assert len(models) == 2 and models[1].fx == model.fx
    assert ext.tobytes() == np.stack([_pose(0), _pose(2)]).tobytes()
    assert images == [["f0_c0.jpg", "f1_c0.jpg"], ["f0_c1.jpg", None]]


if __name__ == "__main__":
    os.makedirs(GOLDEN, exist_ok=True)
    print("\n".join(_write_all(GOLDEN)))
