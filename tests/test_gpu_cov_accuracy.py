"""The covariance entries (vmm_ba_covariance_blocks, vmm_ba_tag_translation_covariance, vmm_ba_intrinsics_system; the
kernels of kernels_cov.hip and the elimination half of kernels_border.hip) held to the accuracy of a float64 inverse.

Input, truth, metric and bound are those of tests/cov_cases.py (proven on the CPU in test_cov_cases_cpu.py): the handle's own
eval_blocks give H, truth is its longdouble inverse, a block's deviation is max_ij |got - truth| / sqrt(truth_aa,ii
truth_bb,jj), and the bound of a case is 8 x the larger deviation of two float64 CPU references over all of its blocks
(A: numpy's inverse, B: the device's scheme restated in numpy).  Blocks of constant, origin and residual-free poses must be
exactly zero.  The references set the bound, never the code under test; every test prints deviation, bound and ratio
(tools/covariance_accuracy.py records them, DESIGN.md section 4.14 holds the measured ones).
"""
import numpy as np
import pytest

import cov_cases as cc
import eval_cases as ec

pytestmark = pytest.mark.gpu

ALL_PAIRS_SCENES = ("24x12", "24x12_robust", "24x12_weak", "24x12_sparse_view", "20x10")
BIG_SCENES = (("44x10", "tags"), ("10x44", "cams"), ("ragged_tags", "cams"), ("ragged_tags", "tags"), ("ragged_cams", "cams"),
              ("ragged_cams", "tags"))
TRANSLATION_SCENES = ("24x12", "44x10", "10x44")
ELIMS = ("cams", "tags")


@pytest.fixture(scope="module")
def eng():
    from visual_marker_mapping_amd import engine
    return engine


def open_handle(eng, sc, elim, k=None):
    """A handle of scene sc at its poses, mask and constants set; k: another camera model than the scene's."""
    intr, dist = (sc.intr, sc.dist) if k is None else (k[:4], k[4:])
    ba = eng.BundleAdjuster(intr, dist, sc.cam_qt, sc.tag_qt, sc.tag_wh, sc.fixed_tag, sc.obs_cam, sc.obs_tag, sc.obs_px,
                            elimination=eng.ELIM_CAMERAS if elim == "cams" else eng.ELIM_TAGS)
    if sc.mask is not None:
        ba.set_observation_mask(sc.mask)
    if sc.cam_const is not None:
        ba.set_constant_poses(sc.cam_const, sc.tag_const)
    return ba


def record(case, request, dev, n_blocks):
    return dict(scene=case.scene.name, elimination=case.elim, request=request, blocks=n_blocks, order=case.order,
                reference_deviation=dict(case.refs), bound=case.bound, deviation=dev, ratio_to_bound=dev / case.bound)


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- 1. all pairs -----------------------------------------------------------------------------------------------------

def run_all_pairs(eng, name, elim):
    """(failures, records, (case, pairs, cov)) of one covariance_blocks call with every ordered pair of poses."""
    sc = cc.scene(name)
    n_c, n = len(sc.cam_qt), len(sc.cam_qt) + len(sc.tag_qt)
    pairs = cc.all_pairs(n)
    with open_handle(eng, sc, elim) as ba:
        case = cc.device_case(ba, sc, elim)
        cov = ba.covariance_blocks(pairs, robustify=sc.robust)
    label = "%s elim %s all pairs" % (name, elim)
    bad, worst = case.check(pairs, cov, label)
    at = {(int(a), int(b)): k for k, (a, b) in enumerate(pairs)}
    kept = (lambda p: p >= n_c) if elim == "cams" else (lambda p: p < n_c)
    gap = 0.0
    for a in range(n):
        m = cov[at[(a, a)]]
        if not _same_bits(m, m.T):
            bad.append("%s: the marginal of pose %d is not symmetric in its bits" % (label, a))
        for b in range(a + 1, n):
            ab, ba_ = cov[at[(a, b)]], cov[at[(b, a)]]
            if kept(a) and kept(b):
                # k_cov_pair, neither endpoint eliminated: G[6 i + j] sums x_i y_j over the rows in one fixed order (thread
                # r mod 256, then the LDS tree), the swapped pair sums y_j x_i in the same order, no transform, sign +1
                if not _same_bits(ba_, ab.T):
                    bad.append("%s: Cov(%d, %d) has not the bits of Cov(%d, %d)^T (both kept)" % (label, b, a, a, b))
            elif case.free(a) and case.free(b):
                i, j = case.pos[a], case.pos[b]
                d = cc.entry_deviation(ba_.T, ab.astype(cc.LD), case.diag[i:i + 6], case.diag[j:j + 6])
                gap = max(gap, d)
                if not d <= case.bound:
                    bad.append("%s: Cov(%d, %d) and Cov(%d, %d)^T are %.3e apart, bound %.3e" % (label, b, a, a, b, d, case.bound))
    print("%s: transposes with an eliminated endpoint at most %.3e apart (bound %.3e, ratio %.3f)"
          % (label, gap, case.bound, gap / case.bound))
    recs = [record(case, "all pairs", worst, len(pairs)), record(case, "all pairs: transpose gap", gap, len(pairs))]
    return bad, recs, (case, pairs, cov)


@pytest.mark.parametrize("elim", ELIMS)
@pytest.mark.parametrize("name", ALL_PAIRS_SCENES)
def test_all_pairs(eng, name, elim):
    bad, _, _ = run_all_pairs(eng, name, elim)
    assert not bad, "\n".join(bad[:20])


# ---- 2. request edges -------------------------------------------------------------------------------------------------

def run_request_edges(eng, elim):
    sc = cc.scene("24x12")
    n_c, n_t = len(sc.cam_qt), len(sc.tag_qt)
    every = cc.all_pairs(n_c + n_t)
    bad, recs = [], []
    with open_handle(eng, sc, elim) as ba:
        case = cc.device_case(ba, sc, elim)
        base = ba.covariance_blocks(every)
        at = {(int(a), int(b)): k for k, (a, b) in enumerate(every)}
        for label, pairs, expected in cc.edge_requests(elim, n_c, n_t):
            # the chunks_at vector named in cov_cases.edge_requests is the one the request produces
            assert cc.chunks_at(n_c, n_t, elim, pairs)[0] == expected, label
            cov = ba.covariance_blocks(pairs)
            full = "24x12 elim %s %s, chunks_at %s" % (elim, label, expected)
            b, worst = case.check(pairs, cov, full)
            bad += b
            for (a, c), got in zip(pairs.tolist(), cov):
                if not _same_bits(got, base[at[(a, c)]]):
                    bad.append("%s: block (%d, %d) has other bits than in the all-pairs call" % (full, a, c))
            recs.append(record(case, "%s, chunks_at %s" % (label, expected), worst, len(pairs)))
    return bad, recs


@pytest.mark.parametrize("elim", ELIMS)
def test_request_edges(eng, elim):
    bad, _ = run_request_edges(eng, elim)
    assert not bad, "\n".join(bad[:20])


# ---- 3. reduced systems of more than 256 rows -------------------------------------------------------------------------

def run_big(eng, name, elim):
    sc = cc.scene(name)
    n_c, n_t = len(sc.cam_qt), len(sc.tag_qt)
    n = n_c + n_t
    extra = []
    if name.startswith("ragged"):
        many = 0 if sc.few == "tags" else n_c      # first pose index of the family of 130
        few = n_c if sc.few == "tags" else 0
        idle, const_many, const_few = many + 129, many + 2, few + ec.RAGGED_COUNTS.index(64)
        extra = [(idle, many + 7), (few + 5, idle), (const_many, few + 1), (const_few, many + 9), (const_few, const_many)]
    pairs = cc.marginals_and_cross(n, 60, extra=extra)
    with open_handle(eng, sc, elim) as ba:
        case = cc.device_case(ba, sc, elim)
        cov = ba.covariance_blocks(pairs, robustify=sc.robust)
    bad, worst = case.check(pairs, cov, "%s elim %s marginals and %d cross pairs" % (name, elim, len(pairs) - n))
    if extra:
        for p in (idle, const_many, const_few):
            assert not case.free(p)
        for (a, b), got in zip(pairs.tolist(), cov):
            if not (case.free(a) and case.free(b)) and got.any():
                bad.append("%s elim %s: block (%d, %d) of a constant or residual-free pose is not zero" % (name, elim, a, b))
    return bad, [record(case, "marginals and %d cross pairs" % (len(pairs) - n), worst, len(pairs))]


@pytest.mark.parametrize("name,elim", BIG_SCENES)
def test_more_than_256_rows(eng, name, elim):
    bad, _ = run_big(eng, name, elim)
    assert not bad, "\n".join(bad[:20])


# ---- 4. tag_translation_covariance ------------------------------------------------------------------------------------

def run_translation(eng, name, elim):
    """The separate k_trsm_diag / k_trsm_update / k_cov_gram path: every tag's 3 x 3 translation block against the leading
    3 x 3 of the truth's marginal, normalised by the truth's translation diagonal."""
    sc = cc.scene(name)
    n_c, n_t = len(sc.cam_qt), len(sc.tag_qt)
    with open_handle(eng, sc, elim) as ba:
        case = cc.device_case(ba, sc, elim)
        cov = ba.tag_translation_covariance(robustify=sc.robust)
    bad, worst = [], 0.0
    for t in range(n_t):
        dev = case.block_deviation(n_c + t, n_c + t, cov[t], rows=3)
        if dev is None:
            if cov[t].any():
                bad.append("%s elim %s: the block of tag %d (origin) is not zero" % (name, elim, t))
            continue
        worst = max(worst, dev)
        if not dev <= case.bound:
            bad.append("%s elim %s tag %d: deviation %.3e above the bound %.3e" % (name, elim, t, dev, case.bound))
    print("%s elim %s tag_translation_covariance: %d blocks, deviation %.3e  bound %.3e  ratio %.3f"
          % (name, elim, n_t, worst, case.bound, worst / case.bound))
    return bad, [record(case, "tag_translation_covariance", worst, n_t)]


@pytest.mark.parametrize("elim", ELIMS)
@pytest.mark.parametrize("name", TRANSLATION_SCENES)
def test_tag_translation_covariance(eng, name, elim):
    bad, _ = run_translation(eng, name, elim)
    assert not bad, "\n".join(bad[:20])


# ---- 5. intrinsics_system ---------------------------------------------------------------------------------------------

def run_model(eng, O, name, elim):
    """intrinsics_system on a ragged scene (poses with 1, 63, 64, 65, 128 and 129 observations through border_body) at
    k = truth + 0.01 PERTURB: C, g_k and the cost in test_gpu_selfcal.py's metric and bounds, inv(S_k) and the step
    inv(S_k) r_k in cov_cases.ModelCase's metrics and bounds."""
    from yardstick import BOUND_C, BOUND_COST, BOUND_G, same_bytes
    sc = cc.scene(name)
    bad, recs = [], []
    first = cc.model_case(O, name, cc.MODEL_VARIANTS[0][0])
    with open_handle(eng, sc, elim, first.k) as ba:
        for variant, robust, masked in cc.MODEL_VARIANTS:
            case = cc.model_case(O, name, variant)
            label = "%s elim %s %s" % (name, elim, variant)
            ba.set_observation_mask(case.mask)
            got = ba.intrinsics_system(robustify=robust)
            again = ba.intrinsics_system(robustify=robust)
            o = case.oracle
            for arr, bound in (("C", BOUND_C), ("g_k", BOUND_G)):
                mag = o["mag_" + arr[0]]
                live = mag > 0
                dev = float((np.abs(got[arr] - o[arr])[live] / mag[live]).max())
                print("%s %-3s deviation %.3e  bound %.3e  ratio %.3f" % (label, arr, dev, bound, dev / bound))
                if not (dev <= bound and not got[arr][~live].any()):
                    bad.append("%s %s: deviation %.3e above %.3e, or a non-zero entry of magnitude 0" % (label, arr, dev, bound))
            dev = abs(got["cost"] - o["cost"]) / o["cost"]
            print("%s cost deviation %.3e  bound %.3e  ratio %.3f" % (label, dev, BOUND_COST, dev / BOUND_COST))
            if not dev <= BOUND_COST:
                bad.append("%s cost: %.3e above %.3e" % (label, dev, BOUND_COST))
            d_cov, d_step = case.deviation(got["S_k"], got["r_k"])
            for what, d, bound in (("inv(S_k)", d_cov, case.bound_cov), ("step", d_step, case.bound_step)):
                print("%s %-8s deviation %.3e  bound %.3e  ratio %.3f  (references %s)"
                      % (label, what, d, bound, d / bound, {k: "%.2e %.2e" % v for k, v in case.refs.items()}))
                if not d <= bound:
                    bad.append("%s %s: deviation %.3e above the bound %.3e" % (label, what, d, bound))
                recs.append(dict(scene=name, elimination=elim, request="intrinsics_system %s: %s" % (variant, what),
                                 reference_deviation={k: v[what == "step"] for k, v in case.refs.items()}, bound=bound,
                                 deviation=d, ratio_to_bound=d / bound))
            if not np.array_equal(got["S_k"], got["S_k"].T):
                bad.append("%s: S_k is not symmetric in its bits" % label)
            if not same_bytes(got, again):
                bad.append("%s: the second call gives other bits" % label)
    return bad, recs


@pytest.mark.parametrize("elim", ELIMS)
@pytest.mark.parametrize("name", ["ragged_tags", "ragged_cams"])
def test_intrinsics_system(eng, oracle, name, elim):
    bad, _ = run_model(eng, oracle, name, elim)
    assert not bad, "\n".join(bad)


# ---- 6. a block-sparse, tree-ordered handle ---------------------------------------------------------------------------

@pytest.mark.parametrize("elim", ELIMS)
def test_block_sparse_tree_ordered_handle_gives_the_bits_of_the_dense_one(eng, monkeypatch, elim):
    sc = cc.scene("24x12_sparse_view")
    pairs = cc.all_pairs(len(sc.cam_qt) + len(sc.tag_qt))
    monkeypatch.setenv("VMM_BA_SCHUR", "dense")
    with open_handle(eng, sc, elim) as ba:
        dense = ba.covariance_blocks(pairs)
        dense_t = ba.tag_translation_covariance()
    monkeypatch.setenv("VMM_BA_SCHUR", "sparse")
    monkeypatch.setenv("VMM_BA_ORDER", "nd")
    with open_handle(eng, sc, elim) as ba:
        assert ba.solve(eng.default_options(robustify=0, max_num_iterations=0))["block_sparse"] == 1
        ba.set_state(sc.cam_qt, sc.tag_qt)
        sparse = ba.covariance_blocks(pairs)
        sparse_t = ba.tag_translation_covariance()
    assert dense.any()
    differ = [tuple(p) for p, a, b in zip(pairs.tolist(), dense, sparse) if not _same_bits(a, b)]
    print("24x12_sparse_view elim %s: %d blocks, %d differ in bits between the dense and the block-sparse handle"
          % (elim, len(pairs), len(differ)))
    assert not differ, differ[:10]
    assert _same_bits(dense_t, sparse_t)
