"""CPU-only checks of the self-calibrating bundle adjustment (ABI 6, additive: vmm_ba_set_intrinsics,
vmm_ba_get_intrinsics, vmm_ba_intrinsics_system, vmm_ba_default_selfcal_options, vmm_ba_solve_selfcal): declared, listed,
exported, laid out as the header says, refusing null arguments before any device call.  The yardstick of
tests/test_gpu_selfcal.py is tests/yardstick.py, proven in tests/test_yardstick_cpu.py.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vmm_ba_set_intrinsics", "vmm_ba_get_intrinsics", "vmm_ba_intrinsics_system", "vmm_ba_default_selfcal_options",
       "vmm_ba_solve_selfcal")


# ---- the entry points -----------------------------------------------------------------------------------------------

def test_selfcal_entry_points_are_declared_listed_and_exported():
    from visual_marker_mapping_amd import _lib
    header = open(os.path.join(ROOT, "include", "vmm_ba.h")).read()
    declared = set(re.findall(r"\b(vmm_ba_[a-z_]+)\s*\(", header))
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert name in declared, name
        assert hasattr(L, name), name
    assert int(re.search(r"#define VMM_BA_ABI_VERSION (\d+)", header).group(1)) == 6
    assert _lib.ABI_VERSION == 6 and L.vmm_ba_abi_version() == 6


def test_selfcal_structs_match_the_header_layout_and_defaults():
    from visual_marker_mapping_amd import _lib
    O, R = _lib.SelfcalOptions, _lib.SelfcalReport
    assert C.sizeof(O) == 24 and [getattr(O, f).offset for f, _ in O._fields_] == [0, 4, 8, 16]      # 2 x int32, 2 x double
    assert C.sizeof(R) == 40 and [getattr(R, f).offset for f, _ in R._fields_] == [0, 4, 8, 12, 16, 24, 32]
    header = open(os.path.join(ROOT, "include", "vmm_ba.h")).read()
    for struct, cls in (("vmm_ba_selfcal_options", O), ("vmm_ba_selfcal_report", R)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f for f, _ in cls._fields_], (struct, names)
    o = O()
    _lib.lib().vmm_ba_default_selfcal_options(C.byref(o))
    assert (o.max_outer_iterations, o.refine_mask, o.parameter_tolerance, o.function_tolerance) == (30, 0x1FF, 1e-10, 1e-12)
    _lib.lib().vmm_ba_default_selfcal_options(None)   # a null pointer is ignored


def test_selfcal_entry_points_refuse_null_arguments_without_a_device():
    from visual_marker_mapping_amd import _lib
    L = _lib.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    intr, dist, cov = np.ones(4), np.zeros(5), np.zeros(81)
    rep = _lib.SelfcalReport()
    fake = C.c_void_p(8)   # never dereferenced: the pointer checks come first
    assert L.vmm_ba_set_intrinsics(None, p(intr), p(dist)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_set_intrinsics(fake, None, p(dist)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_set_intrinsics(fake, p(intr), None) == _lib.ERR_ARGUMENT
    for v in (np.nan, np.inf, -np.inf):
        for bad_intr, bad_dist in ((np.array([1.0, v, 1.0, 1.0]), dist), (intr, np.array([0.0, 0.0, v, 0.0, 0.0]))):
            assert L.vmm_ba_set_intrinsics(fake, p(bad_intr), p(bad_dist)) == _lib.ERR_ARGUMENT
            assert b"finite" in L.vmm_ba_last_error()
    assert L.vmm_ba_get_intrinsics(None, p(intr), p(dist)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_get_intrinsics(fake, None, p(dist)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_get_intrinsics(fake, p(intr), None) == _lib.ERR_ARGUMENT
    c = C.c_double(0)
    assert L.vmm_ba_intrinsics_system(None, 1, 1.0, C.byref(c), p(cov), p(cov), p(cov), p(cov)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_solve_selfcal(None, None, None, None, C.byref(rep), p(intr), p(dist), p(cov)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_solve_selfcal(fake, None, None, None, None, p(intr), p(dist), p(cov)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_solve_selfcal(fake, None, None, None, C.byref(rep), None, p(dist), p(cov)) == _lib.ERR_ARGUMENT
    assert L.vmm_ba_solve_selfcal(fake, None, None, None, C.byref(rep), p(intr), None, p(cov)) == _lib.ERR_ARGUMENT
    for kw in (dict(refine_mask=-1), dict(refine_mask=0x200), dict(max_outer_iterations=-1),
               dict(parameter_tolerance=-1.0), dict(function_tolerance=np.nan)):
        o = _lib.SelfcalOptions()
        L.vmm_ba_default_selfcal_options(C.byref(o))
        for name, v in kw.items():
            setattr(o, name, v)
        assert L.vmm_ba_solve_selfcal(fake, None, C.byref(o), None, C.byref(rep), p(intr), p(dist), p(cov)) == _lib.ERR_ARGUMENT, kw
        assert b"solve_selfcal" in L.vmm_ba_last_error()


def test_selfcalibration_main_needs_a_reconstruction(tmp_path):
    from visual_marker_mapping_amd import selfcalibration
    with pytest.raises(FileNotFoundError) as ei:
        selfcalibration.main(["--project_path", str(tmp_path)])
    assert "reconstruction.json" in str(ei.value) and "does not exist" in str(ei.value)
    (tmp_path / "reconstruction.json").write_text("{}")
    with pytest.raises(FileNotFoundError) as ei:
        selfcalibration.main(["--project_path", str(tmp_path)])
    assert "marker_detections.json" in str(ei.value) and "does not exist" in str(ei.value)
    with pytest.raises(SystemExit):
        selfcalibration.main(["--project_path", str(tmp_path), "--refine_mask", "0x200"])


def test_do_bundle_adjustment_keeps_its_defaults():
    """refineCameraModel is off unless asked for: the positional arguments of doBundleAdjustment are those it had."""
    import inspect
    from visual_marker_mapping_amd.tag_reconstructor import TagReconstructor
    sig = inspect.signature(TagReconstructor.doBundleAdjustment)
    assert list(sig.parameters)[:6] == ["self", "maxNumIterations", "ceresThreads", "robustify", "printSummary", "elimination"]
    assert sig.parameters["refineCameraModel"].default is False and sig.parameters["refine_mask"].default == 0x1FF
