"""The host-side plan of a handle (visual_marker_mapping_amd/csrc/plan.cpp) driven through tests/cpp/plan_test, built
with g++ from plan.cpp alone: observation orders, the rank-k schedule, the block-sparse pair lists and the tree-ordered
factor are checked on the CPU, and the plan's decisions agree with what the GPU tests see."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "plan_test")


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-s", "plan_test"])
    return EXE


def _run(exe, args, text=None):
    r = subprocess.run([exe] + args, input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = dict(line.split() for line in r.stdout.splitlines())
    assert out["failures"] == "0"
    return {k: int(v) for k, v in out.items()}


def _scene_text(s):
    lines = ["%d %d %d" % (len(s.cam_init), len(s.tag_init), s.n_obs)]
    lines += ["%d %d" % (c, t) for c, t in zip(s.obs_cam.tolist(), s.obs_tag.tolist())]
    return "\n".join(lines) + "\n"


def _plan(exe, config, switches=(), **kw):
    from visual_marker_mapping_amd.synthetic import make_scene
    return _run(exe, ["scene"] + list(switches), _scene_text(make_scene(config, **kw)))


# the shapes of test_gpu_kernels.py::test_syrk_few_tiles_both_kernels and ::test_syrk_many_tiles
@pytest.mark.parametrize("k,n", [(3000, 1217), (330, 520), (16, 128), (48, 1000), (1000, 129), (64, 4096)])
@pytest.mark.parametrize("switches", [[], ["syrk_wide=0"], ["syrk_no_xcd=1"]])
def test_syrk_schedule_covers_every_unit_once(exe, k, n, switches):
    out = _run(exe, ["syrk", str(k), str(n)] + switches)
    if switches:
        assert out["syrk_wide"] == 0
    if (k, n) == (3000, 1217) and not switches:
        assert out["syrk_wide"] == 1 and out["syrk_wg"] <= 256


@pytest.mark.parametrize("switches", [[], ["syrk_wide=0"], ["syrk_no_xcd=1"]])
def test_headline_is_dense_with_its_syrk_schedule(exe, switches):
    """500 x 200 at full visibility: dense elimination, the rank-k schedule of its 55 tiles (k_syrk_wide by default)."""
    out = _plan(exe, 2, switches)
    assert out["sparse"] == 0 and out["n_f"] == 200 and out["syrk_tiles"] == 55
    assert out["syrk_wide"] == (0 if switches else 1)


@pytest.mark.parametrize("elim", ["cams", "tags"])
def test_quarter_visibility_is_sparse_in_natural_order(exe, elim):
    out = _plan(exe, 2, ["elim=" + elim], visibility=0.25)
    assert out["sparse"] == 1 and out["tree_nodes"] == 0


@pytest.mark.parametrize("elim", ["cams", "tags"])
def test_close_up_is_sparse(exe, elim):
    out = _plan(exe, 2, ["elim=" + elim], neighbors_min=6, neighbors_max=10)
    assert out["sparse"] == 1 and out["explicit"] == 1
    if elim == "cams":   # test_gpu_sparse.py: the tree ordering is taken
        assert out["tree_nodes"] >= 3


def test_large_close_up_is_tree_ordered(exe):
    """2000 x 1000 close-up: tree-ordered, 64 block columns and more (the six-wave factorisation kernel's range)."""
    out = _plan(exe, 4, neighbors_min=6, neighbors_max=10)
    assert out["sparse"] == 1 and out["tree_nodes"] >= 8 and out["n_blk"] >= 64


# the scenes of test_gpu_sparse.py::test_sparse_path_equals_dense_path, forced onto the block-sparse path, in every
# form of the pair list and ordering
SCENES = {
    "quarter": dict(config=5, n_cams=40, n_tags=30, visibility=0.25),
    "close_up": dict(config=1, n_cams=60, n_tags=40, neighbors_min=4, neighbors_max=7),
    "dense": dict(config=1),
    "two_groups": dict(config=1, n_cams=300, n_tags=250, visibility=0.06),
}


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("elim", ["cams", "tags"])
@pytest.mark.parametrize("form", [[], ["pairs=0"], ["pairs=1"], ["order_nd=1", "nd_leaf=8"]])
def test_forced_sparse_plans(exe, name, elim, form):
    kw = dict(SCENES[name])
    out = _plan(exe, kw.pop("config"), ["schur=2", "elim=" + elim] + form, **kw)
    assert out["sparse"] == 1
    if form == ["pairs=1"] or out["tree_nodes"]:
        assert out["explicit"] == 1
