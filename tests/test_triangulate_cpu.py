"""CPU-only checks of the triangulation entry points (ABI 6, additive): declared, listed, exported, laid out as the header
says, validating their arguments and answering the trivial batches before any device call (so all of this passes without
a GPU), and the host-side surface: the point detection file, the tree of triangulation.json, the packing of the tracks
and the command line's missing-file errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vmm_ba_default_triangulate_options", "vmm_ba_triangulate")


def test_triangulate_entry_points_are_declared_listed_and_exported():
    from visual_marker_mapping_amd import _lib
    header = open(os.path.join(ROOT, "include", "vmm_ba.h")).read()
    declared = set(re.findall(r"\b(vmm_ba_[a-z_]+)\s*\(", header))
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert name in declared, name
        assert hasattr(L, name), name
    assert int(re.search(r"#define VMM_BA_ABI_VERSION (\d+)", header).group(1)) == 6
    assert _lib.ABI_VERSION == 6
    assert L.vmm_ba_abi_version() == 6


def test_triangulate_structs_match_the_header_layout_and_defaults():
    from visual_marker_mapping_amd import _lib, engine
    O, R = _lib.TriangulateOptions, _lib.TriangulateResult
    # int32, int32, 3 x double, 4 x int32
    assert C.sizeof(O) == 48
    assert [getattr(O, f).offset for f, _ in O._fields_] == [0, 4, 8, 16, 24, 32, 36, 40, 44]
    # 4 x int32, 2 x double
    assert C.sizeof(R) == 32
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 4, 8, 12, 16, 24]
    header = open(os.path.join(ROOT, "include", "vmm_ba.h")).read()
    for struct, cls in (("vmm_ba_triangulate_options", O), ("vmm_ba_triangulate_result", R)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip() for decl in body.split(";") if decl.strip()
                 for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f for f, _ in cls._fields_], (struct, names)
    o = O()
    o.reserved = 99
    _lib.lib().vmm_ba_default_triangulate_options(C.byref(o))
    assert (o.refine_iterations, o.robustify, o.huber_a, o.score_cap_px, o.inlier_px, o.reclassify_passes,
            o.min_inlier_views, o.max_pair_views, o.reserved) == (30, 1, 1.0, 100.0, 8.0, 2, 2, 16, 0)
    assert engine.default_triangulate_options(max_pair_views=7).max_pair_views == 7
    assert (_lib.TRI_OK, _lib.TRI_TOO_FEW_VIEWS, _lib.TRI_NO_CANDIDATE, _lib.TRI_TOO_FEW_INLIERS,
            _lib.TRI_SINGULAR) == (0, 1, 2, 3, 4)
    assert _lib.TRI_STATUS_NAMES == ("ok", "too_few_views", "no_candidate", "too_few_inliers", "singular")
    for k, name in enumerate(("OK", "TOO_FEW_VIEWS", "NO_CANDIDATE", "TOO_FEW_INLIERS", "SINGULAR")):
        assert re.search(r"VMM_BA_TRI_%s = %d\b" % (name, k), header), name


def _good():
    return dict(intr=np.array([1000.0, 1000.0, 500.0, 400.0]), dist=np.zeros(5),
                cam_qt=np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (3, 1)), cam_cov=None, n_pts=2,
                pt_start=np.array([0, 2, 5], np.int64), obs_cam=np.array([0, 2, 0, 1, 2], np.int32), obs_uv=np.ones((5, 2)),
                xyz=np.zeros((2, 3)))


def _call(intr, dist, cam_qt, cam_cov, n_pts, pt_start, obs_cam, obs_uv, xyz, opt=None, n_cams=None, device=0):
    from visual_marker_mapping_amd import _lib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return _lib.lib().vmm_ba_triangulate(p(intr), p(dist), len(cam_qt) if n_cams is None else n_cams, p(cam_qt), p(cam_cov),
                                         n_pts, p(pt_start), p(obs_cam), p(obs_uv), opt, p(xyz), None, None, None, None, device)


def test_triangulate_refuses_bad_arguments_with_their_message_before_touching_the_device():
    from visual_marker_mapping_amd import _lib, engine
    good = _good()

    def rejected(text, **kw):
        # device 1 << 20 does not exist: a call that got as far as the device would fail with VMM_BA_ERR_HIP instead
        assert _call(**dict(good, device=1 << 20, **kw)) == _lib.ERR_ARGUMENT, kw
        assert _lib.lib().vmm_ba_last_error().decode() == "vmm_ba_triangulate: " + text, kw

    rejected("null camera model", intr=None)
    rejected("null camera model", dist=None)
    rejected("null pt_start or xyz", pt_start=None)
    rejected("null pt_start or xyz", xyz=None)
    rejected("negative size", n_pts=-1)
    rejected("negative size", n_cams=-1)
    rejected("pt_start[0] is not 0", pt_start=np.array([1, 2, 5], np.int64))
    rejected("pt_start decreases", pt_start=np.array([0, 5, 2], np.int64))
    rejected("null observations", obs_cam=None)
    rejected("null observations", obs_uv=None)
    rejected("obs_cam outside [0, n_cams)", obs_cam=np.array([0, 3, 0, 1, 2], np.int32))
    rejected("obs_cam outside [0, n_cams)", obs_cam=np.array([-1, 2, 0, 1, 2], np.int32))
    rejected("obs_cam is not strictly increasing within a point", obs_cam=np.array([0, 2, 0, 1, 1], np.int32))
    rejected("obs_cam is not strictly increasing within a point", obs_cam=np.array([2, 0, 0, 1, 2], np.int32))
    rejected("null cam_qt", cam_qt=None, n_cams=3)
    for v in (np.nan, np.inf):
        rejected("non-finite camera model", intr=np.array([1000.0, v, 500.0, 400.0]))
        rejected("non-finite camera model", dist=np.array([0.0, 0.0, v, 0.0, 0.0]))
        for col in (0, 5):
            bad = good["cam_qt"].copy()
            bad[1, col] = v
            rejected("non-finite camera pose", cam_qt=bad)
        bad = good["obs_uv"].copy()
        bad[4, 1] = v
        rejected("non-finite obs_uv", obs_uv=bad)
        bad = np.tile(np.eye(6), (3, 1, 1))
        bad[2, 5, 5] = v
        rejected("non-finite cam_cov", cam_cov=bad)
    zero_q = good["cam_qt"].copy()
    zero_q[2, :4] = 0.0
    rejected("zero camera quaternion", cam_qt=zero_q)
    bad_options = [dict(refine_iterations=-1), dict(reclassify_passes=-1), dict(min_inlier_views=0), dict(max_pair_views=1),
                   dict(max_pair_views=65)]
    for field in ("huber_a", "score_cap_px", "inlier_px"):
        bad_options += [{field: v} for v in (0.0, -1.0, np.nan, np.inf)]
    for kw in bad_options:
        o = engine.default_triangulate_options(**kw)
        rejected("bad triangulation options", opt=C.byref(o))
        # an empty batch is answered before the options are looked at
        assert _call(**dict(good, n_pts=0, opt=C.byref(o), device=1 << 20)) == _lib.OK, kw
    # the limits of max_pair_views themselves are fine (a batch that needs no device shows it)
    for v in (2, 64):
        o = engine.default_triangulate_options(max_pair_views=v)
        assert _call(**dict(good, pt_start=np.array([0, 1, 1], np.int64), opt=C.byref(o), device=1 << 20)) == _lib.OK
    # the Python wrapper refuses arrays that do not fit together, and unknown options
    g = _good()
    args = (g["intr"], g["dist"], g["cam_qt"], g["pt_start"], g["obs_cam"], g["obs_uv"])
    with pytest.raises(ValueError):
        engine.triangulate(*args[:3], [0, 2], g["obs_cam"], g["obs_uv"])
    with pytest.raises(ValueError):
        engine.triangulate(*args[:5], g["obs_uv"][:4])
    with pytest.raises(ValueError):
        engine.triangulate(*args, cam_cov=np.zeros((2, 6, 6)))
    with pytest.raises(AttributeError):
        engine.triangulate(*args, no_such_option=1)
    with pytest.raises(AttributeError):
        engine.triangulate(*args, reserved=1)
    with pytest.raises(_lib.VmmBaError) as ei:
        engine.triangulate(*args[:4], np.array([0, 2, 0, 1, 7], np.int32), g["obs_uv"], device=1 << 20)
    assert ei.value.status == _lib.ERR_ARGUMENT


def test_trivial_batches_are_answered_without_a_device():
    from visual_marker_mapping_amd import _lib, engine
    g = _good()
    assert _call(**dict(g, n_pts=0, device=1 << 20)) == _lib.OK
    xyz, cov, cov_cams, inl, res = engine.triangulate(g["intr"], g["dist"], g["cam_qt"], [0], np.zeros(0, np.int32),
                                                      np.zeros((0, 2)), device=1 << 20)
    assert xyz.shape == (0, 3) and cov.shape == (0, 3, 3) and cov_cams.shape == (0, 3, 3) and inl.shape == (0,) and res == []
    # no point has two observations: TOO_FEW_VIEWS and zeros, whatever the outputs held
    L = _lib.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    start, cam, uv = np.array([0, 1, 1, 2], np.int64), np.array([2, 0], np.int32), np.ones((2, 2))
    xyz, cov, cov_cams = np.full((3, 3), 7.0), np.full((3, 9), 7.0), np.full((3, 9), 7.0)
    inl = np.full(2, 7, np.uint8)
    res = (_lib.TriangulateResult * 3)()
    for r in res:
        r.status, r.n_inlier_obs, r.trials, r.rms_px, r.cost = 9, 9, 9, 9.0, 9.0
    cam_cov = np.tile(np.eye(6), (3, 1, 1))
    assert L.vmm_ba_triangulate(p(g["intr"]), p(g["dist"]), 3, p(g["cam_qt"]), p(cam_cov), 3, p(start), p(cam), p(uv), None,
                                p(xyz), p(cov), p(cov_cams), p(inl), C.cast(res, C.c_void_p), 1 << 20) == _lib.OK
    assert (xyz == 0).all() and (cov == 0).all() and (cov_cams == 0).all() and (inl == 0).all()
    assert [(r.status, r.n_obs, r.n_inlier_obs, r.trials, r.rms_px, r.cost) for r in res] \
        == [(_lib.TRI_TOO_FEW_VIEWS, n, 0, 0, 0.0, 0.0) for n in (1, 0, 1)]
    # the same through the wrapper, every optional output null
    assert L.vmm_ba_triangulate(p(g["intr"]), p(g["dist"]), 3, p(g["cam_qt"]), None, 3, p(start), p(cam), p(uv), None,
                                p(xyz), None, None, None, None, 1 << 20) == _lib.OK
    out = engine.triangulate(g["intr"], g["dist"], g["cam_qt"], start, cam, uv, device=1 << 20)
    assert [r["status"] for r in out[4]] == [_lib.TRI_TOO_FEW_VIEWS] * 3 and not out[3].any() and (out[0] == 0).all()
    # with a point of two observations the call does go to the device
    assert _call(**dict(g, device=1 << 20)) == _lib.ERR_HIP
    assert _lib.lib().vmm_ba_last_error().decode().startswith("vmm_ba_triangulate: hipSetDevice: ")


def test_point_detections_round_trip(tmp_path):
    from visual_marker_mapping_amd import io as vio
    tracks = {7: [(12, (101.25, 2000.0 / 3.0)), (3, (0.1, -5.5))], 2: [], 40: [(0, (1e-300, 6000.0))]}
    path = str(tmp_path / "point_detections.json")
    assert vio.writePointDetections(tracks, path)
    assert vio.readPointDetections(path) == tracks
    text = open(path).read()
    assert '"id": "7"' in text and '"image_id": "12"' in text and '"101.25"' in text   # every scalar a quoted string
    assert list(vio.readPointDetections(path)) == [7, 2, 40]
    bare = str(tmp_path / "bare.json")
    with open(bare, "w") as f:
        f.write('{"points": [{"id": 7, "observations": [{"image_id": 12, "uv": [1.5, 2]}]}]}')
    assert vio.readPointDetections(bare) == {7: [(12, (1.5, 2.0))]}
    with open(bare, "w") as f:
        f.write('{"points": [{"id": 7, "observations": [{"image_id": 12, "uv": [1.5]}]}]}')
    with pytest.raises(RuntimeError):
        vio.readPointDetections(bare)


def test_triangulation_tree_is_built_from_plain_values(tmp_path):
    from visual_marker_mapping_amd import _lib, io as vio, triangulation
    cov = np.diag([4.0, 9.0, 16.0])
    cams = np.diag([12.0, 16.0, 9.0])
    points = {5: {"point": np.array([1.0, 2.0, 3.0]), "covariance": cov, "covariance_cameras": cams, "status": _lib.TRI_OK,
                  "n_obs": 4, "n_inlier_obs": 3, "rms_px": 0.5, "inliers": {}},
              1: {"point": np.zeros(3), "covariance": np.zeros((3, 3)), "covariance_cameras": np.zeros((3, 3)),
                  "status": _lib.TRI_TOO_FEW_VIEWS, "n_obs": 1, "n_inlier_obs": 0, "rms_px": 0.0, "inliers": {}}}
    tree = triangulation.triangulation_tree(points)
    assert [p["id"] for p in tree["points"]] == [1, 5]
    p = tree["points"][1]
    assert list(p) == ["id", "position", "status", "num_observations", "num_inlier_observations", "rms_px", "sigma",
                       "covariance", "covariance_cameras"]
    assert p["position"] == [1.0, 2.0, 3.0] and p["status"] == "ok" and p["sigma"] == [4.0, 5.0, 5.0]
    assert (p["num_observations"], p["num_inlier_observations"], p["rms_px"]) == (4, 3, 0.5)
    assert p["covariance"] == {"rows": 3, "cols": 3, "coefficents": [4.0, 0, 0, 0, 9.0, 0, 0, 0, 16.0]}
    assert p["covariance_cameras"]["coefficents"][4] == 16.0
    assert tree["points"][0]["status"] == "too_few_views"
    path = str(tmp_path / "triangulation.json")
    vio.write_json(path, tree)
    back = vio.read_json(path)["points"]
    assert back[1]["position"] == ["1", "2", "3"] and back[1]["covariance"]["rows"] == "3"
    geo = triangulation.tag_geometry_tree({3: {"corners": np.arange(12.0).reshape(4, 3), "width": 0.1, "height": 0.2,
                                               "width_ratio": 1.0, "height_ratio": 2.0, "out_of_plane": 0.0,
                                               "model_gap": 0.5, "status": _lib.TRI_SINGULAR}})
    assert geo["tags"][0]["status"] == "singular" and geo["tags"][0]["corners"][3] == [9.0, 10.0, 11.0]


def test_tracks_are_sorted_unknown_images_dropped_and_duplicates_refused():
    from visual_marker_mapping_amd.tag_reconstructor import TagReconstructor
    tracks = {"a": [(9, (9.0, 90.0)), (2, (2.0, 20.0)), (5, (5.0, 50.0)), (4, (4.0, 40.0))],
              "b": [(7, (7.0, 70.0))], "c": [], "d": [(5, (1.0, 1.0)), (2, (3.0, 3.0))]}
    ids, start, cam, uv, image, dropped = TagReconstructor._pack_tracks(tracks, [2, 4, 5, 8, 9])
    assert ids == ["a", "b", "c", "d"]
    assert start.dtype == np.int64 and list(start) == [0, 4, 4, 4, 6]
    assert cam.dtype == np.int32 and list(cam) == [0, 1, 2, 4, 0, 2]
    assert image == [2, 4, 5, 9, 2, 5]
    assert uv.tolist() == [[2.0, 20.0], [4.0, 40.0], [5.0, 50.0], [9.0, 90.0], [3.0, 3.0], [1.0, 1.0]]
    assert dropped == 1
    ids, start, cam, uv, image, dropped = TagReconstructor._pack_tracks({1: [(3, (0.0, 0.0))]}, [])
    assert list(start) == [0, 0] and uv.shape == (0, 2) and dropped == 1
    with pytest.raises(ValueError) as ei:
        TagReconstructor._pack_tracks({"a": [(2, (0.0, 0.0)), (4, (1.0, 1.0)), (2, (5.0, 5.0))]}, [2, 4])
    assert "twice" in str(ei.value)


def test_triangulation_main_names_the_missing_file(tmp_path):
    from visual_marker_mapping_amd import triangulation
    proj = str(tmp_path)
    with pytest.raises(FileNotFoundError) as ei:
        triangulation.main(["--project_path", proj])
    assert "reconstruction.json" in str(ei.value) and "does not exist" in str(ei.value)
    with pytest.raises(FileNotFoundError) as ei:
        triangulation.main(["--project_path", proj, "--map", str(tmp_path / "my_map.json")])
    assert "my_map.json" in str(ei.value)
    open(os.path.join(proj, "reconstruction.json"), "w").write("{}")
    with pytest.raises(FileNotFoundError) as ei:
        triangulation.main(["--project_path", proj])
    assert "point_detections.json" in str(ei.value) and "does not exist" in str(ei.value)
    with pytest.raises(FileNotFoundError) as ei:
        triangulation.main(["--project_path", proj, "--tag_corners"])
    assert "marker_detections.json" in str(ei.value)
    open(os.path.join(proj, "point_detections.json"), "w").write("{}")
    with pytest.raises(FileNotFoundError) as ei:
        triangulation.main(["--project_path", proj, "--cameras", str(tmp_path / "loc.json")])
    assert "loc.json" in str(ei.value)
    with pytest.raises(FileNotFoundError) as ei:
        triangulation.main(["--project_path", proj, "--camera_covariances", str(tmp_path / "unc.json")])
    assert "unc.json" in str(ei.value)
