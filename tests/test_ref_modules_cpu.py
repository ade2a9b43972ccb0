"""ref_geometry.py and ref_algebra.py against their definitions, in longdouble on seeded inputs: the identities a rotation, a
quaternion product, Plus and its inverse must meet, the documented difference of the two distortion models, the small
algebra against a longdouble solve, the summation orders against exact integer sums."""
import numpy as np
import pytest

import ref_algebra as ra
import ref_geometry as rg

LD = np.longdouble
EPS = float(np.finfo(LD).eps)
N = 48


def _quats(rng, n=N):
    return rng.normal(size=(n, 4)).astype(LD) * rng.uniform(0.2, 5.0, (n, 1))      # any length: every user normalises


def _spd(rng, n):
    A = rng.standard_normal((n, 2 * n))
    return A @ A.T


def test_rotation_is_orthonormal_and_follows_the_product():
    rng = np.random.default_rng(1)
    a, b = _quats(rng), _quats(rng)
    Ra, Rb = rg.rotation(a), rg.rotation(b)
    assert Ra.dtype == LD and Ra.shape == (N, 3, 3)
    assert np.abs(Ra @ np.swapaxes(Ra, 1, 2) - np.eye(3)).max() <= 16 * EPS
    assert np.abs(np.linalg.det(Ra.astype(np.float64)) - 1).max() <= 1e-12
    assert np.abs(rg.rotation(rg.qmul(a, b)) - Ra @ Rb).max() <= 32 * EPS
    # one quaternion with a tail gives one matrix; the yardstick's norm is the same rotation to float64 rounding
    assert np.array_equal(rg.rotation(np.r_[a[3], 1, 2, 3]), Ra[3])
    q = a[5].astype(np.float64)
    assert np.abs(rg.rotation(q, np.float64, norm="linalg") - rg.rotation(q, np.float64)).max() <= 8 * 2.0 ** -53


def test_quat_from_R_inverts_rotation_on_all_four_branches():
    rng = np.random.default_rng(2)
    q = rg.unit(_quats(rng, 400))
    got, branch = rg.quat_from_R(rg.rotation(q))
    assert set(branch.tolist()) == {0, 1, 2, 3}
    sign = np.sign((got * q).sum(axis=1, keepdims=True))
    assert np.abs(got * sign - q).max() <= 64 * EPS
    assert np.abs((got * got).sum(axis=1) - 1).max() <= 8 * EPS


def test_pose_minus_inverts_pose_plus():
    rng = np.random.default_rng(3)
    poses = np.concatenate([rg.unit(_quats(rng)), rng.normal(size=(N, 3)).astype(LD)], axis=1)
    steps = rng.normal(0, 0.3, (N, 6)).astype(LD)
    steps[0, 3:] = 0                       # a pure translation leaves the quaternion's bits
    moved = rg.pose_plus(poses, steps)
    assert moved.dtype == LD and np.array_equal(moved[0, :4], poses[0, :4])
    for p, d, m in zip(poses, steps, moved):
        assert np.array_equal(rg.pose_plus(p, d), m)            # one pose or a batch: the same bits
        assert np.abs(rg.pose_minus(m, p) - d).max() <= 64 * EPS
        assert np.abs(rg.pose_minus(np.r_[-3 * m[:4], m[4:]], p) - d).max() <= 64 * EPS      # a quaternion's length and sign do not count
    # Plus is the left product by a rotation of 2 |d| about d
    R = rg.rotation(moved) @ np.swapaxes(rg.rotation(poses), 1, 2)
    angle = np.arccos(np.clip((np.trace(R, axis1=1, axis2=2) - 1) / 2, -1, 1))
    assert np.abs(angle - 2 * np.sqrt((steps[:, 3:] ** 2).sum(axis=1))).max() <= 1e-9


def test_skew_is_the_cross_product():
    rng = np.random.default_rng(4)
    v, u = rng.normal(size=(N, 3)).astype(LD), rng.normal(size=(N, 3)).astype(LD)
    S = rg.skew(v)
    assert S.dtype == LD and np.array_equal(S, -np.swapaxes(S, 1, 2))
    assert np.array_equal(np.einsum("nij,nj->ni", S, u), np.cross(v, u))
    assert np.array_equal(rg.skew(v[7]), S[7])


def test_corners_run_LL_LR_UR_UL_and_reach_the_camera_frame():
    rng = np.random.default_rng(5)
    wh = rng.uniform(0.05, 0.3, (N, 2))
    local = rg.local_corners(wh)
    assert np.array_equal(np.sign(local[0, :, :2]), [[-1, -1], [1, -1], [1, 1], [-1, 1]]) and not local[..., 2].any()
    assert np.array_equal(2 * np.abs(local[:, :, :2]), np.broadcast_to(wh.astype(LD)[:, None], (N, 4, 2)))
    tag = np.concatenate([_quats(rng), rng.normal(size=(N, 3))], axis=1)
    cam = np.concatenate([_quats(rng), rng.normal(size=(N, 3))], axis=1)
    pw = rg.world_corners(tag, wh)
    assert np.abs(pw - (np.einsum("nij,nkj->nki", rg.rotation(tag), local) + tag[:, None, 4:])).max() <= 8 * EPS
    pc, Rc, a, b = rg.camera_points(cam, tag, wh, parts=True)
    assert np.array_equal(pc, rg.camera_points(cam, tag, wh)) and np.array_equal(a + tag[:, None, 4:].astype(LD), pw)
    assert np.array_equal(b + cam[:, None, 4:].astype(LD), pc) and np.array_equal(Rc, rg.rotation(cam))


def test_the_aliased_distortion_differs_by_the_documented_term():
    rng = np.random.default_rng(6)
    x, y = rng.uniform(-0.6, 0.6, N).astype(LD), rng.uniform(-0.4, 0.4, N).astype(LD)
    dist = np.array([-0.19, 0.37, -3e-4, 4e-4, 0.057], LD)
    xd, yd, r2, rad = rg.distort(x, y, dist)
    xa, ya, _, _ = rg.distort(x, y, dist, aliased=True)
    assert np.array_equal(xa, xd) and np.array_equal(r2, x * x + y * y)
    assert np.abs(rad - (1 + dist[0] * r2 + dist[1] * r2 ** 2 + dist[4] * r2 ** 3)).max() <= 8 * EPS
    term = 2 * dist[3] * (xd - x) * y
    assert np.abs(term).max() > 1e-8 and np.abs((ya - yd) - term).max() <= 8 * EPS * np.abs(yd).max()
    assert np.array_equal(rg.distort(x, y, np.zeros(5, LD))[:2], (x, y))
    intr = np.array([800.0, 810.0, 320.0, 240.0], LD)
    assert np.array_equal(rg.pixel(intr, xd, yd), np.stack([800 * xd + 320, 810 * yd + 240], axis=-1))


def test_the_rig_chain_is_the_composed_pose_and_its_columns():
    rng = np.random.default_rng(7)
    ext, rig = np.r_[_quats(rng, 1)[0], 0.2, -0.1, 0.05], np.r_[_quats(rng, 1)[0], 1.0, 2.0, 3.0]
    cam, Rc, v = rg.compose_rig(ext, rig)
    assert np.abs(rg.rotation(cam) - rg.rotation(ext) @ rg.rotation(rig)).max() <= 32 * EPS
    assert np.abs(cam[4:] - (rg.rotation(ext) @ rig[4:] + ext[4:])).max() <= 8 * EPS and np.array_equal(v, Rc @ rig[4:].astype(LD))
    # a rig step and an extrinsic step move the camera as the two column turns say, to first order
    f = lambda q: np.r_[rg.rotation(q) @ np.array([0.3, -0.2, 1.5], LD) + q[4:]]      # a point in the camera frame
    Jc = np.stack([(f(rg.pose_plus(cam, h)) - f(rg.pose_plus(cam, -h))) / 2e-6 for h in 1e-6 * np.eye(6, dtype=LD)], axis=-1)
    J_rig = np.stack([(f(rg.compose_rig(ext, rg.pose_plus(rig, h))[0]) - f(rg.compose_rig(ext, rg.pose_plus(rig, -h))[0])) / 2e-6
                      for h in 1e-6 * np.eye(6, dtype=LD)], axis=-1)
    J_ext = np.stack([(f(rg.compose_rig(rg.pose_plus(ext, h), rig)[0]) - f(rg.compose_rig(rg.pose_plus(ext, -h), rig)[0])) / 2e-6
                      for h in 1e-6 * np.eye(6, dtype=LD)], axis=-1)
    assert np.abs(rg.turn_to_rig(Jc, Rc) - J_rig).max() <= 1e-9 and np.abs(rg.extrinsic_columns(Jc, v) - J_ext).max() <= 1e-9


def test_seeded_helpers_draw_what_they_say():
    q = rg.small_quat(np.random.default_rng(8), 0.1)
    assert abs(np.linalg.norm(q) - 1) <= 1e-15 and q[0] > 0.9
    assert rg.start([3, 0, 2]).tolist() == [0, 3, 3, 5] and rg.start([3, 0, 2]).dtype == np.int64
    cam, tag = np.array([[0.0, 1.0, 0, 0, 0, 0, 3.0]]), np.array([[1.0, 0, 0, 0, 0.1, 0, 0]])
    intr, dist = [800.0, 800.0, 320.0, 240.0], [-0.1, 0.02, 1e-3, -1e-3, 0.0]
    clean, noisy = rg.pixels(np.random.default_rng(9), intr, dist, cam, tag, [[0.1, 0.1]], 0.5)
    assert clean.dtype == np.float64 and clean.shape == (1, 8) and 0 < np.abs(noisy - clean).max() < 3
    assert np.array_equal(clean, rg.project(intr, dist, cam, tag, [[0.1, 0.1]]).reshape(1, 8).astype(np.float64))


@pytest.mark.parametrize("n", [3, 6, 9])
def test_small_algebra_agrees_with_a_longdouble_solve(n):
    rng = np.random.default_rng(10 + n)
    A, S, g = _spd(rng, n), _spd(rng, n), rng.standard_normal(n)
    tol = 8 * n * np.linalg.cond(A) * 2.0 ** -53          # a few ulp of the condition
    A_ld = A.astype(LD)
    inv = np.linalg.inv(A).astype(LD)
    for _ in range(3):
        inv = inv + inv @ (np.eye(n, dtype=LD) - A_ld @ inv)
    L = ra.cholesky(A)
    assert np.array_equal(L, np.tril(L)) and np.abs(L @ L.T - A).max() <= 8 * n * 2.0 ** -53 * np.abs(A).max()
    M = ra.lower_inverse(L)
    assert np.abs(M @ L - np.eye(n)).max() <= tol
    assert np.array_equal(ra.lower_gram(M), ra.spd_inverse(A))
    C = ra.spd_inverse(A)
    assert np.array_equal(C, C.T) and np.abs(C - inv).max() <= tol * np.abs(inv).max()
    B = rng.standard_normal((n, 4))
    assert np.abs(L @ ra.forward(L, B) - B).max() <= tol * np.abs(B).max() and np.abs(L.T @ ra.backward(L, g) - g).max() <= tol * np.abs(g).max()
    for lam in (0.0, 1e-3):
        D = ra.damped(A, lam)
        assert np.array_equal(D - np.diag(np.diag(D)), A - np.diag(np.diag(A))) and np.allclose(np.diag(D), (1 + lam) * np.diag(A), rtol=1e-15)
        want = -(np.linalg.inv(D).astype(LD) @ g)
        want = want - np.linalg.inv(D).astype(LD) @ (D.astype(LD) @ want + g)
        assert np.abs(ra.damped_solve(A, g, lam) - want).max() <= tol * np.abs(want).max()
    W = ra.sandwich(C, S)
    assert np.array_equal(W, W.T) and np.abs(W - inv @ S.astype(LD) @ inv).max() <= tol * np.abs(W).max()


def test_summation_orders_are_exact_on_integers():
    rng = np.random.default_rng(20)
    for m in (1, 3, 4, 5, 63, 64, 65, 257):
        x = rng.integers(-1000, 1000, (m, 3)).astype(np.float64)
        assert np.array_equal(ra.ordered_sum(x), x.sum(axis=0)) and np.array_equal(ra.chains4(x), x.sum(axis=0))
        t = rng.integers(-1000, 1000, (m, 4, 2)).astype(np.float64)
        assert np.array_equal(ra.wave_total(t), t.sum(axis=(0, 1)))
    v = rng.integers(-1000, 1000, 256).astype(np.float64)
    assert ra.tree256(v) == v.sum() and ra.chains4(np.zeros((0, 2))).tolist() == [0, 0]
    # the orders are the documented ones: a term that only one order absorbs
    x = np.array([1.0, 2.0 ** -53, 0.0, 0.0, 0.0, 2.0 ** -53, 0.0, 0.0])
    assert ra.ordered_sum(x) == 1.0 and ra.chains4(x[:, None])[0] == 1.0 + 2.0 ** -52
