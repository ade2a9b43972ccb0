"""integration/visual_marker_mapping.patch -- the reference-side binding -- must apply to the reference tree as it is,
be reproducible from integration/make_patch.py, and be purely additive (the reference's own bodies stay under #else).
The checks against the reference tree (REF) skip where that tree is not present; test_patch_is_additive reads only
this repository."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
PATCH = os.path.join(ROOT, "integration", "visual_marker_mapping.patch")

needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="reference tree not present")


@needs_ref
def test_patch_applies_to_the_reference(tmp_path):
    work = tmp_path / "ref"
    shutil.copytree(REF, str(work), ignore=shutil.ignore_patterns(".git"))
    subprocess.check_call(["git", "apply", "--check", PATCH], cwd=str(work))
    subprocess.check_call(["git", "apply", PATCH], cwd=str(work))
    tr = open(str(work / "src" / "TagReconstructor.cpp")).read()
    cm = open(str(work / "src" / "CameraModel.cpp")).read()
    cmake = open(str(work / "CMakeLists.txt")).read()
    hd = open(str(work / "include" / "visual_marker_mapping" / "TagReconstructor.h")).read()
    # the five bodies of INTEGRATION.md section 2 (src/TagReconstructor.cpp:340-455,646-784, src/CameraModel.cpp:6-26)
    # go through ONE device-resident handle owned by the reconstructor (built on first use, dropped by setCameraModel)
    assert tr.count("#ifdef VISUAL_MARKER_MAPPING_WITH_VMM_BA") == 7   # include, member definition, 4 methods, setCameraModel
    assert tr.count("vmmBa().reprojectionStatistics(reconstructedTags, reconstructedCameras, originTagId,") == 3
    assert tr.count("vmmBa().doBundleAdjustment(reconstructedTags, reconstructedCameras, originTagId, maxNumIterations,") == 1
    assert "vmm_ba_adapter::doBundleAdjustment(" not in tr and "vmm_ba_adapter::reprojectionStatistics(" not in tr
    assert tr.count("struct TagReconstructor::VmmBaResident : vmm_ba_adapter::Resident<DetectionResult, CameraModel>") == 1
    assert tr.count("vmmBaResident_.reset(new VmmBaResident(detectionResults_, camModel));") == 1
    assert tr.count("    vmmBaResident_.reset();") == 1 and tr.index("camModel = cameraModel;") < tr.index("    vmmBaResident_.reset();")
    assert cm.count("vmm_ba_adapter::projectPoint(*this, point3D.x(), point3D.y(), point3D.z())") == 1
    assert "VMM_BA_ROOT}/visual_marker_mapping_amd/libvmm_ba.so" in cmake
    # the guard changes the class layout: it must reach every target that includes the header
    assert "target_compile_definitions(visual_marker_mapping_lib PUBLIC VISUAL_MARKER_MAPPING_WITH_VMM_BA)" in cmake
    # the member sits with the class's other data members (include/visual_marker_mapping/TagReconstructor.h:134-145)
    assert hd.count("#ifdef VISUAL_MARKER_MAPPING_WITH_VMM_BA") == 2 and "#include <memory>" in hd
    assert hd.index("CameraModel camModel;") < hd.index("mutable std::unique_ptr<VmmBaResident, VmmBaResidentDeleter> vmmBaResident_;")
    # every #ifdef the patch opens is closed inside the same function
    ref_tr = open(os.path.join(REF, "src", "TagReconstructor.cpp")).read()
    assert tr.count("#endif") - ref_tr.count("#endif") == 7 and tr.count("#else") - ref_tr.count("#else") == 4
    # the adapter header the patched files include offers what they call
    hdr = open(os.path.join(ROOT, "include", "vmm_ba_adapter.hpp")).read()
    for name in ("doBundleAdjustment(", "reprojectionStatistics(", "projectPoint(", "class Resident"):
        assert name in hdr


def test_patch_is_additive():
    """What can be checked without the reference tree: the patch parses, touches the four files of the binding, only
    adds lines, and the adapter header it includes offers what the added lines call."""
    text = open(PATCH).read()
    body = [l for l in text.splitlines() if not l.startswith(("---", "+++", "diff "))]
    assert not any(l.startswith("-") for l in body)
    stat = subprocess.check_output(["git", "apply", "--numstat", PATCH], cwd=ROOT, text=True).splitlines()
    files = {l.split("\t")[2]: (int(l.split("\t")[0]), int(l.split("\t")[1])) for l in stat}
    assert sorted(files) == ["CMakeLists.txt", "include/visual_marker_mapping/TagReconstructor.h",
                             "src/CameraModel.cpp", "src/TagReconstructor.cpp"], files
    assert all(added > 0 and removed == 0 for added, removed in files.values()), files
    added = "\n".join(l[1:] for l in body if l.startswith("+"))
    # 7 in TagReconstructor.cpp (as test_patch_applies_to_the_reference counts them), 2 in the header, 2 in CameraModel.cpp
    assert added.count("#ifdef VISUAL_MARKER_MAPPING_WITH_VMM_BA") == 11
    assert added.count("#endif") == added.count("#ifdef VISUAL_MARKER_MAPPING_WITH_VMM_BA")
    for call in ("vmmBa().doBundleAdjustment(", "vmmBa().reprojectionStatistics(", "vmm_ba_adapter::projectPoint(",
                 "vmm_ba_adapter::Resident<"):
        assert call in added
    hdr = open(os.path.join(ROOT, "include", "vmm_ba_adapter.hpp")).read()
    for name in ("doBundleAdjustment(", "reprojectionStatistics(", "projectPoint(", "class Resident"):
        assert name in hdr


@needs_ref
def test_patch_is_additive_and_reproducible():
    text = open(PATCH).read()
    body = [l for l in text.splitlines() if not l.startswith(("---", "+++", "diff "))]
    assert not any(l.startswith("-") for l in body)
    sys.path.insert(0, os.path.join(ROOT, "integration"))
    try:
        import make_patch
    finally:
        sys.path.pop(0)
    assert make_patch.make_patch(REF) == text
