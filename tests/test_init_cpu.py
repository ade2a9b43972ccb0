"""CPU-only checks of the map-initialisation entry points (ABI 6): declared, listed and exported."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vmm_ba_quad_poses", "vmm_ba_default_init_options", "vmm_ba_initialize")


def test_init_entry_points_are_declared_listed_and_exported():
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


def test_init_structs_match_the_header_layout_and_defaults():
    from visual_marker_mapping_amd import _lib
    # int32, int32, double, int32 (+ padding) and 4 x int32, 2 x double
    assert C.sizeof(_lib.InitOptions) == 24 and _lib.InitOptions.score_cap_px.offset == 8
    assert _lib.InitOptions.refine_iterations.offset == 16
    assert C.sizeof(_lib.InitReport) == 32 and _lib.InitReport.avg_reprojection_px.offset == 16
    o = _lib.InitOptions()
    _lib.lib().vmm_ba_default_init_options(C.byref(o))
    assert (o.sweeps, o.min_tag_observations, o.score_cap_px, o.refine_iterations) == (1, 2, 100.0, 30)


def test_quad_poses_validates_arguments_before_touching_the_device():
    import numpy as np
    import pytest
    from visual_marker_mapping_amd import _lib, engine
    with pytest.raises(ValueError):
        engine.quad_poses([1, 1, 0, 0], [0] * 5, np.ones((2, 2)), np.ones((3, 8)))
    qt2, rms2 = engine.quad_poses([1, 1, 0, 0], [0] * 5, np.zeros((0, 2)), np.zeros((0, 8)))   # n == 0: no device call
    assert qt2.shape == (0, 2, 7) and rms2.shape == (0, 2)
    assert _lib.lib().vmm_ba_initialize(None, None, None, None, None) == _lib.ERR_ARGUMENT
