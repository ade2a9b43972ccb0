"""vmm_ba_solve_small without a device: the declaration, the export, and every argument error, which the library must
report before its first device call (these tests run where there is no GPU at all)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(n_cams, n_tags, obs=((0, 0),)):
    """A well-formed problem of the given sizes (identity poses, the listed (camera, tag) observations)."""
    cam = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 2.0]), (n_cams, 1))
    tag = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0.0]), (n_tags, 1))
    obs = np.asarray(obs, np.int32).reshape(-1, 2)
    return dict(intr=(1000.0, 1000.0, 640.0, 480.0), dist=(0.0,) * 5, cam_qt=cam, tag_qt=tag, tag_wh=np.full((n_tags, 2), 0.1),
                fixed_tag=0, obs_cam=obs[:, 0], obs_tag=obs[:, 1], obs_px=np.full((len(obs), 8), 500.0))


def _error(problems, **kw):
    from visual_marker_mapping_amd import _lib, engine as eng
    with pytest.raises(_lib.VmmBaError) as err:
        eng.solve_small(problems, **kw)
    return err.value


def test_header_declares_and_library_exports_the_entry():
    from visual_marker_mapping_amd import _lib
    with open(os.path.join(ROOT, "include", "vmm_ba.h")) as f:
        header = f.read()
    assert re.search(r"^int\s+vmm_ba_solve_small\s*\(", header, re.M)
    assert re.search(r"^#define\s+VMM_BA_SMALL_MAX_KEPT\s+24\b", header, re.M) and _lib.SMALL_MAX_KEPT == 24
    assert "vmm_ba_solve_small" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "vmm_ba_solve_small")


def test_kept_family_above_the_limit_under_auto_names_the_problem():
    from visual_marker_mapping_amd import _lib
    e = _error([_problem(3, 2), _problem(25, 25)])
    assert e.status == _lib.ERR_ARGUMENT
    assert "problem 1" in str(e) and "25" in str(e)
    assert "problem 0" in str(_error([_problem(25, 25)]))


def test_kept_family_above_the_limit_under_a_forced_elimination():
    from visual_marker_mapping_amd import _lib, engine as eng
    e = _error([_problem(30, 25)], elimination=eng.ELIM_CAMERAS)   # keeps the 25 tags
    assert e.status == _lib.ERR_ARGUMENT and "problem 0" in str(e)


def test_observation_index_out_of_range_names_the_problem():
    from visual_marker_mapping_amd import _lib
    e = _error([_problem(3, 2), _problem(3, 2, obs=((0, 0), (3, 1)))])
    assert e.status == _lib.ERR_ARGUMENT and "problem 1" in str(e) and "observation 1" in str(e)


def test_null_problems_and_bad_elimination():
    from visual_marker_mapping_amd import _lib, engine as eng
    L = _lib.lib()
    cam, tag = np.zeros((3, 7)), np.zeros((2, 7))
    s = (_lib.Summary * 1)()
    o = eng.default_options()
    rc = L.vmm_ba_solve_small(1, None, None, None, C.byref(o), eng.ELIM_AUTO, cam.ctypes.data_as(C.c_void_p),
                              tag.ctypes.data_as(C.c_void_p), s, 0)
    assert rc == _lib.ERR_ARGUMENT and b"null" in L.vmm_ba_last_error()
    e = _error([_problem(3, 2)], elimination=7)
    assert e.status == _lib.ERR_ARGUMENT and "elimination" in str(e)


def test_empty_batch_is_ok_without_a_device():
    from visual_marker_mapping_amd import _lib, engine as eng
    assert _lib.lib().vmm_ba_solve_small(0, None, None, None, None, eng.ELIM_AUTO, None, None, None, 0) == _lib.OK
    assert eng.solve_small([]) == []
