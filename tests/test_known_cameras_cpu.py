"""CPU-only checks of the known-cameras frame that triangulatePoints / locateTags and engine.triangulate /
engine.locate_tags share: both members hand down the same cameras, drop what has no pose and refuse a duplicate; both
engine functions refuse arrays that do not fit together before any device call (all of this passes without a GPU)."""
import numpy as np
import pytest

CAMERA_IDS = (12, 3, 40, 7)          # not contiguous, not sorted
PX = [[10.0, 10.0], [20.0, 10.0], [20.0, 20.0], [10.0, 20.0]]
RESULT = dict(status=0, n_obs=0, n_inlier_obs=0, trials=0, rms_px=0.0, cost=0.0)


def _reconstructor(observations):
    """Tags 5 and 8 detected as `observations` [(imageId, tagId), ...] says; no reconstructed camera of its own."""
    from visual_marker_mapping_amd.tag_reconstructor import DetectionResult, Tag, TagImg, TagObservation, TagReconstructor
    images = sorted({i for i, _ in observations})
    det = DetectionResult([TagImg(i, "img%d" % i) for i in images], [Tag(t, "x", 0.1, 0.2) for t in (5, 8)],
                          [TagObservation(i, t, PX) for i, t in observations])
    return TagReconstructor(det)


def _cameras():
    from visual_marker_mapping_amd.tag_reconstructor import Camera
    cams = {i: Camera(i, [1.0, 0.0, 0.0, 0.0], [0.1 * i, 0.0, 1.0]) for i in CAMERA_IDS}
    covs = {i: np.arange(36.0).reshape(6, 6) + i for i in CAMERA_IDS if i != 40}   # camera 40 has none
    return cams, covs


@pytest.fixture
def calls(monkeypatch):
    """The two engine calls replaced by recorders that answer with zeros of the right shapes."""
    from visual_marker_mapping_amd import tag_reconstructor as tr
    seen = {}

    def triangulate(intr, dist, cam_qt, pt_start, obs_cam, obs_uv, cam_cov=None, device=0, **options):
        seen["triangulate"] = dict(cam_qt=cam_qt, cam_cov=cam_cov, start=pt_start, obs_cam=obs_cam, obs=obs_uv)
        n = len(pt_start) - 1
        return np.zeros((n, 3)), np.zeros((n, 3, 3)), np.zeros((n, 3, 3)), np.ones(len(obs_cam), bool), [dict(RESULT)] * n

    def locate_tags(intr, dist, cam_qt, tag_wh, tag_start, obs_cam, obs_px, cam_cov=None, device=0, **options):
        seen["locate_tags"] = dict(cam_qt=cam_qt, cam_cov=cam_cov, start=tag_start, obs_cam=obs_cam, obs=obs_px, tag_wh=tag_wh)
        n = len(tag_start) - 1
        qt = np.tile([1.0, 0, 0, 0, 0, 0, 0], (n, 1))
        return qt, np.zeros((n, 6, 6)), np.zeros((n, 6, 6)), np.ones(len(obs_cam), bool), [dict(RESULT)] * n

    monkeypatch.setattr(tr._engine, "triangulate", triangulate)
    monkeypatch.setattr(tr._engine, "locate_tags", locate_tags)
    return seen


def test_both_members_hand_down_the_same_cameras(calls):
    rec = _reconstructor([(3, 5), (7, 5), (40, 8)])
    cams, covs = _cameras()
    rec.triangulatePoints({"p": [(40, (1.0, 2.0)), (3, (3.0, 4.0))]}, cameras=cams, cameraCovariances=covs)
    rec.locateTags(cameras=cams, cameraCovariances=covs)
    a, b = calls["triangulate"], calls["locate_tags"]
    assert a["cam_qt"].shape == (4, 7) and a["cam_qt"].tobytes() == b["cam_qt"].tobytes()
    assert a["cam_qt"][:, 4].tolist() == [0.1 * i for i in sorted(CAMERA_IDS)]          # image id order: 3, 7, 12, 40
    assert a["cam_cov"].shape == (4, 6, 6) and a["cam_cov"].tobytes() == b["cam_cov"].tobytes()
    assert not a["cam_cov"][3].any()                                                     # camera 40: no entry, a zero block
    for k, i in enumerate(sorted(CAMERA_IDS)[:3]):
        assert (a["cam_cov"][k] == covs[i]).all()
    # the dense indices are positions in that order
    assert a["start"].tolist() == [0, 2] and a["obs_cam"].tolist() == [0, 3] and a["obs"].tolist() == [[3.0, 4.0], [1.0, 2.0]]
    assert b["start"].tolist() == [0, 2, 3] and b["obs_cam"].tolist() == [0, 1, 3] and b["tag_wh"].tolist() == [[0.1, 0.2]] * 2
    # without covariances neither hands one down
    rec.triangulatePoints({"p": [(3, (3.0, 4.0))]}, cameras=cams)
    rec.locateTags(cameras=cams)
    assert calls["triangulate"]["cam_cov"] is None and calls["locate_tags"]["cam_cov"] is None


def test_an_observation_in_an_image_without_a_pose_is_dropped_by_both(calls):
    rec = _reconstructor([(3, 5), (99, 5), (7, 5), (99, 8)])     # image 99 has no pose
    cams, _ = _cameras()
    pts = rec.triangulatePoints({"p": [(99, (9.0, 9.0)), (7, (1.0, 2.0)), (3, (3.0, 4.0))], "q": [(99, (5.0, 5.0))]}, cameras=cams)
    assert rec.lastTriangulationDropped == 2
    assert calls["triangulate"]["start"].tolist() == [0, 2, 2] and calls["triangulate"]["obs_cam"].tolist() == [0, 1]
    assert pts["p"]["inliers"] == {3: True, 7: True} and pts["q"]["inliers"] == {}
    tags = rec.locateTags(cameras=cams)
    assert calls["locate_tags"]["start"].tolist() == [0, 2, 2] and calls["locate_tags"]["obs_cam"].tolist() == [0, 1]
    assert sorted(tags) == [5, 8]
    assert rec.lastTagLocationReport[5]["observations"] == [0, 2] and rec.lastTagLocationReport[8]["observations"] == []


def test_a_duplicate_image_in_one_item_is_refused_by_both(calls):
    cams, _ = _cameras()
    rec = _reconstructor([(3, 5), (7, 8), (3, 5)])
    with pytest.raises(ValueError) as ei:
        rec.triangulatePoints({"p": [(3, (1.0, 2.0)), (7, (1.0, 2.0)), (3, (3.0, 4.0))]}, cameras=cams)
    assert str(ei.value) == "point 'p' is observed twice in one image"
    with pytest.raises(ValueError) as ei:
        rec.locateTags(cameras=cams)
    assert str(ei.value) == "tag 5 is observed twice in one image"
    assert calls == {}


def test_the_engine_refuses_arrays_that_do_not_fit_together():
    from visual_marker_mapping_amd import engine as eng
    intr, dist = (800.0, 800.0, 320.0, 240.0), (0.0,) * 5
    cam_qt = np.tile([1.0, 0, 0, 0, 0, 0, 1.0], (3, 1))
    start, cam = np.array([0, 2]), np.array([0, 1])
    uv, px, wh = np.zeros((2, 2)), np.zeros((2, 8)), np.full((1, 2), 0.1)
    for call, obs in ((lambda **kw: eng.triangulate(intr, dist, cam_qt, kw["start"], cam, kw["obs"], cam_cov=kw["cov"]), uv),
                      (lambda **kw: eng.locate_tags(intr, dist, cam_qt, wh, kw["start"], cam, kw["obs"], cam_cov=kw["cov"]), px)):
        with pytest.raises(ValueError) as ei:
            call(start=start, obs=obs, cov=np.zeros((2, 6, 6)))
        assert str(ei.value) == "cam_cov and cam_qt differ in length"
        with pytest.raises(ValueError) as ei:
            call(start=start, obs=obs[:1], cov=None)
        assert str(ei.value) == "observation arrays differ in length"
    with pytest.raises(ValueError) as ei:
        eng.triangulate(intr, dist, cam_qt, np.array([0, 1]), cam, uv)
    assert str(ei.value) == "pt_start must have n_pts + 1 entries and end at the number of observations"
    with pytest.raises(ValueError) as ei:
        eng.triangulate(intr, dist, cam_qt, np.zeros(0, np.int64), cam[:0], uv[:0])
    assert str(ei.value) == "pt_start must have n_pts + 1 entries and end at the number of observations"
    for bad in (np.array([0, 1]), np.array([0, 1, 2])):     # does not end at n_obs; n_tags + 2 entries
        with pytest.raises(ValueError) as ei:
            eng.locate_tags(intr, dist, cam_qt, wh, bad, cam, px)
        assert str(ei.value) == "tag_start must have n_tags + 1 entries and end at the number of observations"
