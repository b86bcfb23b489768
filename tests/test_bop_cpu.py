"""tests/bop_ref.py, the numpy restatement of include/ffb6d_bop.h that the BOP kernels are held against, pins itself: properties
the three errors must have, a second formulation, a VSD case counted by hand; and the host arithmetic of ffb6d_amd.bop
(symmetry_transforms, recall, average_recall).  No GPU."""
import numpy as np
import pytest

import bop_ref
from ffb6d_amd import bop


@pytest.fixture(scope="module")
def case():
    return bop_ref.mssd_case()


def with_sym(T, R, t):
    out = T.copy()
    out[:, :3], out[:, 3] = T[:, :3] @ R, T[:, :3] @ t + T[:, 3]
    return out


def test_identical_poses_give_zero_for_all_three_errors(case):
    r = case["rows"]
    s2, p2 = bop_ref.mssd_mspd2(case["models"], case["syms"], r["class_of"], r["frame_of"], r["gt_T"], r["gt_T"], case["K"])
    assert not s2.any() and not p2.any()
    v = bop_ref.vsd_case(48, 64)
    depth = bop_ref.render_alone(v["meshes"], v["gt_T"], v["class_of"], v["frame_of"], v["K"], 48, 64)
    counts, err = bop_ref.vsd(np.zeros((2, 48, 64), np.float32), depth, depth, v["class_of"], v["frame_of"], v["K"], v["diameters"],
                              v["delta"], bop_ref.TAUS10)
    drawn = counts[:, 0] > 0
    assert drawn.sum() >= 4 and not err[drawn].any() and (counts[drawn, 0] == counts[drawn, 1]).all() and not counts[:, 2:].any()


def test_a_pose_moved_by_a_symmetry_is_free_with_the_set_and_not_without(case):
    rng = np.random.RandomState(2)
    for c, k in ((2, 101), (3, 1), (4, 7)):
        R, t = case["syms"][c][k]
        gt = np.zeros((3, 4))
        gt[:, :3], gt[:, 3] = bop_ref.rot(rng.randn(3), 0.7), [0.03, -0.02, 0.8]
        # the estimate is the plain pose, the ground truth is recorded as the symmetric copy's inverse image: est = gt o sym
        est = with_sym(gt, R, t)
        s2, p2 = bop_ref.mssd_mspd2_row(case["models"][c], case["syms"][c], est, gt, case["K"][0])
        n2, q2 = bop_ref.mssd_mspd2_row(case["models"][c], [], est, gt, case["K"][0])
        assert s2 < 1e-28 and p2 < 1e-18, (c, s2, p2)                # exact up to the rounding of the composed transform
        assert n2 > 1e-6 and q2 > 1.0, (c, n2, q2)


def test_the_matmul_formulation_agrees_to_1e_12(case):
    r = case["rows"]
    for q in range(len(r["class_of"])):
        c, b = r["class_of"][q], r["frame_of"][q]
        s2, p2 = bop_ref.mssd_mspd2_row(case["models"][c], case["syms"][c], r["est_T"][q], r["gt_T"][q], case["K"][b])
        ms, mp = bop_ref.mssd_mspd2_matmul(case["models"][c], case["syms"][c], r["est_T"][q], r["gt_T"][q], case["K"][b])
        if q == 4:      # an exact symmetric copy: both errors are the rounding of the composed transform, 0 up to cancellation
            assert np.sqrt(s2) < 1e-15 and ms < 1e-15 and np.sqrt(p2) < 1e-11 and mp < 1e-11, (s2, ms, p2, mp)
            continue
        assert np.sqrt(s2) > 1e-3 and np.sqrt(p2) > 1.0
        np.testing.assert_allclose(np.sqrt(s2), ms, rtol=1e-12, atol=0)
        np.testing.assert_allclose(np.sqrt(p2), mp, rtol=1e-12, atol=0)


def test_bad_rows_of_the_restatement(case):
    b = case["bad"]
    s2, p2 = bop_ref.mssd_mspd2(case["models"], case["syms"], b["class_of"], b["frame_of"], b["est_T"], b["gt_T"], case["K"])
    assert np.isnan(s2[[0, 1, 2, 3, 4, 5, 6, 9]]).all() and np.isnan(p2[[0, 1, 2, 3, 4, 5, 6, 9]]).all()
    assert np.isfinite(s2[7]) and p2[7] == np.inf                               # a point behind the camera
    assert np.isfinite(s2[8]) and np.isfinite(p2[8])


def test_vsd_of_a_hand_built_4x5_case():
    # K with fx = fy = 1 and the principal point at pixel (0, 0): only pixel (0, 0) has dist == z exactly, so every depth below is
    # put through ray_dist and the thresholds are chosen on the distances
    K = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    f32 = np.float32
    gt, est, test = np.zeros((4, 5), f32), np.zeros((4, 5), f32), np.zeros((4, 5), f32)
    # row 0: gt and est both drawn, no measurement (dt == 0): visible in both, inter
    gt[0, :3], est[0, :3] = 1.0, [1.0, 1.05, 1.5]                              # errors 0, ~0.05 d, ~0.5 d  (diameter 1 at pixel (0,0))
    # row 1: occluded beyond delta (test far in front of both): invisible in both
    gt[1, :2], est[1, :2], test[1, :2] = 1.0, 1.0, 0.5
    # row 2: pixel (2,0) measured; gt exactly delta behind the test surface is visible; pixel (2,1) just beyond is not, and the
    # estimate there, nearer than the test surface, is visible alone
    gt[2, 0], est[2, 0] = 1.0, 1.0
    gt[2, 1], est[2, 1] = 1.0, 0.7
    # row 3: gt only (est misses), test absent: union without inter; est only elsewhere
    gt[3, 0] = 1.0
    est[3, 4] = 2.0
    dg, de = bop_ref.ray_dist(gt, K), bop_ref.ray_dist(est, K)
    # the test depth at (2,0): the depth whose distance is exactly dg - delta is found by construction: take delta := dg - dt
    test[2, 0] = 0.9
    test[2, 1] = 0.9
    dt = bop_ref.ray_dist(test, K)
    delta = f32(dg[2, 0] - dt[2, 0])                                             # exactly at delta: visible
    assert dg[2, 1] - dt[2, 1] > delta                                           # farther from the axis: the same depths differ by more
    counts, err = bop_ref.vsd_row(test, est, gt, K, 1.0, delta, [0.04, 0.3])
    # union: (0,0) (0,1) (0,2) (2,0) (2,1: est alone) (3,0) (3,4) = 7; inter: (0,0) (0,1) (0,2) (2,0) = 4
    assert counts[0] == 7 and counts[1] == 4, counts
    e = np.abs(dg - de)
    want = [int(sum(e[p] >= f32(tau) for p in ((0, 0), (0, 1), (0, 2), (2, 0)))) for tau in (0.04, 0.3)]
    assert want == [2, 1] and list(counts[2:]) == want, (counts, want)
    assert np.array_equal(err, [(2 + 3) / 7.0, (1 + 3) / 7.0])
    # one ulp less tolerance hides the pixel at delta
    counts2, _ = bop_ref.vsd_row(test, est, gt, K, 1.0, np.nextafter(delta, f32(0)), [0.04, 0.3])
    assert counts2[0] == 6 and counts2[1] == 3, counts2
    # nothing visible at all: 1.0
    counts3, err3 = bop_ref.vsd_row(test, np.zeros((4, 5), f32), np.zeros((4, 5), f32), K, 1.0, delta, [0.04, 0.3])
    assert not counts3.any() and np.array_equal(err3, [1.0, 1.0])


def test_symmetry_transforms_counts_and_orthonormality():
    flip = np.diag([-1.0, -1.0, 1.0, 1.0])
    quarter = np.eye(4)
    quarter[:3, :3] = bop_ref.rot([0, 0, 1], np.pi / 2)
    assert len(bop.symmetry_transforms()) == 1
    assert len(bop.symmetry_transforms(discrete=[flip, np.eye(4)])) == 2          # an exact copy of the identity is removed
    assert len(bop.symmetry_transforms(continuous=[((0, 0, 1), (0, 0, 0))])) == 315
    assert len(bop.symmetry_transforms(continuous=[((0, 0, 2), (0.1, 0, 0))], max_disc_step=0.1)) == 32
    both = bop.symmetry_transforms(discrete=[flip, quarter], continuous=[((1, 0, 0), (0, 0.02, 0.01))], max_disc_step=0.5)
    assert len(both) == 3 * 7
    for sym in (both, bop.symmetry_transforms(continuous=[((1, 2, 3), (0.1, 0.2, 0.3))], max_disc_step=0.3)):
        R0, t0 = sym[0]
        assert np.array_equal(R0, np.eye(3)) and not t0.any()
        assert sum(np.array_equal(R, np.eye(3)) and not t.any() for R, t in sym) == 1
        for R, t in sym:
            np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-14)
            assert abs(np.linalg.det(R) - 1) < 1e-14
    # a continuous transform leaves its axis line in place: offset + s * axis maps onto itself
    for R, t in bop.symmetry_transforms(continuous=[((1, 2, 3), (0.1, 0.2, 0.3))], max_disc_step=0.3):
        p = np.array([0.1, 0.2, 0.3]) + 0.7 * np.array([1.0, 2.0, 3.0])
        np.testing.assert_allclose(R @ p + t, p, atol=1e-14)


def test_recall_and_average_recall_on_hand_made_errors():
    assert bop.recall([], [0.1]) == 0.0
    assert bop.recall([0.05, 0.2, np.inf, np.nan], [0.1, 0.3]) == 3 / 8
    assert bop.recall([0.1], [0.1]) == 0.0                                       # strictly below
    assert bop.recall([1.0, 1.0], [[2.0, 0.5], [0.5, 0.5]]) == 1 / 4            # per-estimate thresholds
    assert bop.recall([[0.0, 1.0]], [0.5]) == 1 / 2                              # several error values per estimate
    # three estimates: perfect; VSD 0.22 at every tau, MSSD 0.12 d, MSPD 22 px at W = 1280 (as 11 px at 640); missing
    vsd = np.array([[0.0] * 10, [0.22] * 10, [np.inf] * 10])
    ar = bop.average_recall(vsd, [0.0, 0.012, np.inf], [0.0, 22.0, np.inf], [0.2, 0.1, 0.3], width=1280)
    assert ar["n"] == 3
    np.testing.assert_allclose(ar["ar_vsd"], (10 + 6) / 30, rtol=1e-15)         # 0.22 < 0.25 .. 0.5
    np.testing.assert_allclose(ar["ar_mssd"], (10 + 8) / 30, rtol=1e-15)        # 0.12 d < 0.15 d .. 0.5 d
    np.testing.assert_allclose(ar["ar_mspd"], (10 + 8) / 30, rtol=1e-15)        # 22 px < 30 .. 100 px
    np.testing.assert_allclose(ar["ar"], (ar["ar_vsd"] + ar["ar_mssd"] + ar["ar_mspd"]) / 3, rtol=1e-15)
    assert bop.average_recall(np.zeros((0, 10)), [], [], [])["ar"] == 0.0
