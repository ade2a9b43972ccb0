"""CPU-only tests of the pose-covariance feature: the writer of reconstruction_uncertainty.json, joint_covariance, and
the export and argument check of vmm_ba_covariance_blocks (no device call is made for a null handle)."""
import ctypes as C
import json

import numpy as np


def _spd(seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((6, 6))
    return a @ a.T + 6.0 * np.eye(6)


def _scalars(node):
    if isinstance(node, dict):
        for v in node.values():
            yield from _scalars(v)
    elif isinstance(node, list):
        for v in node:
            yield from _scalars(v)
    else:
        yield node


def test_uncertainty_file_round_trip(tmp_path):
    from visual_marker_mapping_amd import uncertainty
    tag_cov = {230: _spd(1), 7: np.zeros((6, 6)), 1001: _spd(2)}
    cam_cov = {12: _spd(3), 3: _spd(4)}
    path = str(tmp_path / "reconstruction_uncertainty.json")
    uncertainty.write_uncertainty(path, 7, True, tag_cov, cam_cov)
    with open(path) as f:
        tree = json.load(f)
    assert all(isinstance(v, str) for v in _scalars(tree))          # every scalar is a quoted string
    assert tree["origin_tag_id"] == "7" and tree["robustify"] == "true"
    for key, cov in (("reconstructed_tags", tag_cov), ("reconstructed_cameras", cam_cov)):
        assert [int(e["id"]) for e in tree[key]] == sorted(cov)
        for e in tree[key]:
            ref = cov[int(e["id"])]
            assert sorted(e) == ["covariance", "id", "sigma"]
            assert sorted(e["covariance"]) == ["coefficents", "cols", "rows"]
            assert e["covariance"]["rows"] == "6" and e["covariance"]["cols"] == "6"
            got = np.array([float(v) for v in e["covariance"]["coefficents"]]).reshape(6, 6)
            assert got.tobytes() == np.ascontiguousarray(ref, np.float64).tobytes()   # %.17g round-trips a double
            sigma = np.array([float(v) for v in e["sigma"]])
            assert sigma.shape == (6,) and sigma.tobytes() == np.sqrt(np.diag(ref)).tobytes()
    assert not np.array([float(v) for v in tree["reconstructed_tags"][0]["sigma"]]).any()   # the origin tag


def test_joint_covariance_assembles_the_12x12():
    from visual_marker_mapping_amd import engine as eng
    caa, cbb = _spd(5), _spd(6)
    cab = np.random.default_rng(7).standard_normal((6, 6))
    J = eng.joint_covariance(caa, cab, cbb)
    assert J.shape == (12, 12)
    assert np.array_equal(J[:6, :6], caa) and np.array_equal(J[6:, 6:], cbb)
    assert np.array_equal(J[:6, 6:], cab) and np.array_equal(J[6:, :6], cab.T)
    assert np.array_equal(J, J.T)


def test_library_exports_covariance_blocks_and_refuses_a_null_handle():
    from visual_marker_mapping_amd import _lib
    assert "vmm_ba_covariance_blocks" in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, "vmm_ba_covariance_blocks")
    a = np.zeros(1, np.int32)
    cov = np.zeros(36)
    rc = L.vmm_ba_covariance_blocks(None, 0, 1.0, 1, a.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p),
                                    cov.ctypes.data_as(C.c_void_p))
    assert rc == _lib.ERR_ARGUMENT
    assert L.vmm_ba_covariance_blocks(None, 0, 1.0, 0, None, None, None) == _lib.ERR_ARGUMENT
