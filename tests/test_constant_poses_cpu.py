"""CPU-only checks of the constant-pose entry point and of the host side of the map extension: the entry is declared,
listed and exported at ABI 6; the packings turn constantTagIds into the flag array; the pruning and the Python wrapper
behave before any device call (all of this passes without a GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_constant_poses_is_declared_listed_and_exported():
    from visual_marker_mapping_amd import _lib
    header = open(os.path.join(ROOT, "include", "vmm_ba.h")).read()
    declared = set(re.findall(r"\b(vmm_ba_[a-z_]+)\s*\(", header))
    L = _lib.lib()
    name = "vmm_ba_set_constant_poses"
    assert name in _lib.EXPORTS and name in declared and hasattr(L, name)
    assert re.search(r"int vmm_ba_set_constant_poses\(vmm_ba_handle h, const uint8_t\* cam_const, const uint8_t\* "
                     r"tag_const\);", header)
    assert "ABI 6, additive" in header
    assert int(re.search(r"#define VMM_BA_ABI_VERSION (\d+)", header).group(1)) == 6
    assert _lib.ABI_VERSION == 6 and L.vmm_ba_abi_version() == 6
    # a null handle is the one invalid argument, refused before any device call
    assert L.vmm_ba_set_constant_poses(None, None, None) == _lib.ERR_ARGUMENT
    assert b"null handle" in L.vmm_ba_last_error()


def _reconstructor():
    """3 images, tags 3, 5, 8, 9 detected; 3, 5, 8 reconstructed, image 2 not reconstructed."""
    from visual_marker_mapping_amd.tag_reconstructor import (Camera, DetectionResult, ReconstructedTag, Tag, TagImg,
                                                             TagObservation, TagReconstructor)
    px = [[10.0, 10.0], [20.0, 10.0], [20.0, 20.0], [10.0, 20.0]]
    obs = [TagObservation(i, t, px) for i, t in ((0, 3), (0, 5), (1, 5), (1, 8), (1, 9), (2, 3), (2, 8))]
    det = DetectionResult([TagImg(i, "img%d" % i) for i in range(3)], [Tag(t, "x", 0.1, 0.1) for t in (3, 5, 8, 9)], obs)
    rec = TagReconstructor(det)
    rec.setReconstructedTags({t: ReconstructedTag(t, "x", [1, 0, 0, 0], [0.1 * t, 0, 0], 0.1, 0.1) for t in (3, 5, 8)})
    rec.setReconstructedCameras({i: Camera(i, [1, 0, 0, 0], [0, 0, 1.0 + i]) for i in (0, 1)})
    return rec


def test_packings_turn_constant_tag_ids_into_the_flag_array():
    rec = _reconstructor()
    assert rec.constantTagIds == set()
    p = rec._pack(for_ba=True)
    assert p["tag_ids"] == [3, 5, 8] and p["tag_const"].dtype == np.uint8 and p["tag_const"].tolist() == [0, 0, 0]
    rec.constantTagIds = {5, 8, 9, 77}          # 9 is not reconstructed, 77 is unknown: neither is packed
    p = rec._pack(for_ba=True)
    assert p["tag_const"].tolist() == [0, 1, 1] and p["fixed"] == -1
    rec.originTagId = 3
    assert rec._pack(for_ba=False)["fixed"] == 0 and rec._pack(for_ba=False)["tag_const"].tolist() == [0, 1, 1]
    # the device-resident packing: rows of the whole detection set (tags 3, 5, 8, 9)
    rec._resident = True
    p = rec._pack_resident(for_ba=True)
    assert rec._full["tags"].tolist() == [3, 5, 8, 9] and p["tag_rows"] == [0, 1, 2]
    assert p["tag_const"].dtype == np.uint8 and p["tag_const"].tolist() == [0, 1, 1, 0]
    rec.constantTagIds = set()
    assert rec._pack_resident(for_ba=True)["tag_const"].tolist() == [0, 0, 0, 0]


def test_constants_reach_the_handle_only_when_they_change():
    from visual_marker_mapping_amd.tag_reconstructor import TagReconstructor

    class Handle:
        constant_poses = (None, None)
        calls = []

        def set_constant_poses(self, cam_const=None, tag_const=None):
            self.calls.append(None if tag_const is None else tag_const.tolist())
            self.constant_poses = (None, None if tag_const is None else tag_const.tobytes())

    h = Handle()
    flags = np.array([0, 1, 1], np.uint8)
    TagReconstructor._set_constants(h, dict(tag_const=np.zeros(3, np.uint8)))
    assert h.calls == []                                       # nothing constant, nothing sent
    TagReconstructor._set_constants(h, dict(tag_const=flags))
    TagReconstructor._set_constants(h, dict(tag_const=flags.copy()))
    assert h.calls == [[0, 1, 1]]
    TagReconstructor._set_constants(h, dict(tag_const=np.zeros(3, np.uint8)))
    assert h.calls == [[0, 1, 1], None]


def test_remove_bad_markers_keeps_constant_tags(capsys):
    rec = _reconstructor()
    rec.originTagId = 3
    rec.constantTagIds = {5}
    rec.computeReprojectionErrorPerTag = lambda: ({3: 9.0, 5: 9.0, 8: 9.0}, 9.0)
    rec.removeBadMarkers(2.0)
    assert sorted(rec.reconstructedTags) == [3, 5]
    assert "Removing bad marker with id 8" in capsys.readouterr().out


def test_set_constant_poses_checks_shapes_and_dtype_before_the_library(monkeypatch):
    from visual_marker_mapping_amd import engine

    def no_library():
        raise AssertionError("the library must not be called")

    monkeypatch.setattr(engine._lib, "lib", no_library)
    ba = engine.BundleAdjuster.__new__(engine.BundleAdjuster)
    ba._h, ba.n_cams, ba.n_tags = C.c_void_p(), 3, 2
    for kw in (dict(cam_const=np.zeros(2, np.uint8)), dict(tag_const=np.zeros(3, np.uint8)),
               dict(cam_const=np.zeros((3, 1), np.uint8)), dict(cam_const=np.zeros(3, np.uint8), tag_const=[1])):
        with pytest.raises(ValueError):
            ba.set_constant_poses(**kw)
    with pytest.raises(TypeError):
        ba.set_constant_poses(tag_const=np.array([0.0, 1.0]))
    with pytest.raises(AssertionError, match="the library must not be called"):
        ba.set_constant_poses(np.array([True, False, True]), [0, 1])       # well-formed: goes on to the library


def test_extension_main_parses_its_arguments_and_needs_a_map(tmp_path):
    from visual_marker_mapping_amd import extension
    with pytest.raises(SystemExit):
        extension.main([])                                     # --project_path is required
    with pytest.raises(FileNotFoundError) as ei:
        extension.main(["--project_path", str(tmp_path)])
    assert "reconstruction.json" in str(ei.value) and "does not exist" in str(ei.value)
    assert "no map to extend" in str(ei.value)
    other = tmp_path / "elsewhere" / "map.json"
    with pytest.raises(FileNotFoundError) as ei:
        extension.main(["--project_path", str(tmp_path), "--map", str(other), "--output", str(tmp_path / "o.json")])
    assert str(other) in str(ei.value)


def test_extend_reconstruction_needs_a_map_tag_in_the_new_images():
    rec = _reconstructor()
    from visual_marker_mapping_amd.tag_reconstructor import ReconstructedTag
    far = {t: ReconstructedTag(t, "x", [1, 0, 0, 0], [0, 0, 0], 0.1, 0.1) for t in (100, 101)}
    rec.setReconstructedTags(far)
    with pytest.raises(RuntimeError, match="No reconstructed tags in image found."):
        rec.extendReconstruction()
    assert sorted(rec.reconstructedTags) == [100, 101] and sorted(rec.reconstructedCameras) == [0, 1]


def test_extend_reconstruction_that_fails_part_way_leaves_the_object_as_it_was(monkeypatch):
    from visual_marker_mapping_amd.tag_reconstructor import Camera, ReconstructedTag, TagReconstructor
    rec = _reconstructor()
    rec.reconstructedTags[100] = ReconstructedTag(100, "x", [1, 0, 0, 0], [0, 0, 0], 0.1, 0.1)   # no image sees it
    rec.constantTagIds = {100}
    tags_before = dict(rec.reconstructedTags)
    cams_before = dict(rec.reconstructedCameras)

    def fails(self, numThreads, init_options):
        # the state the driver is in after initialize placed some poses: packed map only, constants set, new poses added
        assert sorted(self.reconstructedTags) == [3, 5, 8] and self.reconstructedCameras == {}
        assert self.constantTagIds == {3, 5, 8, 100} and self._resident
        self.reconstructedCameras[2] = Camera(2, [1, 0, 0, 0], [0, 0, 3.0])
        self.reconstructedTags[9] = ReconstructedTag(9, "x", [1, 0, 0, 0], [0.9, 0, 0], 0.1, 0.1)
        raise RuntimeError("device error")

    monkeypatch.setattr(TagReconstructor, "_extend_reconstruction", fails)
    with pytest.raises(RuntimeError, match="device error"):
        rec.extendReconstruction()
    assert sorted(rec.reconstructedTags) == sorted(tags_before) == [3, 5, 8, 100]
    assert sorted(rec.reconstructedCameras) == sorted(cams_before) == [0, 1]
    assert all(rec.reconstructedTags[t] is v for t, v in tags_before.items())
    assert all(rec.reconstructedCameras[c] is v for c, v in cams_before.items())
    assert rec.constantTagIds == {100} and not rec._resident and rec._full is None
