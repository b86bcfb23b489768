"""The numpy restatement of include/ffb6d_orb.h (tests/orb_ref.py) against closed forms, and the host logic of the texture-aware
keypoints (ffb6d_amd/objinfo.py: quotas, view poses).  OpenCV is not in the build image, so cv2.ORB's own keypoints cannot be
recorded: the expected values below were worked out from the rule as the header states it (isolated one-pixel dots have closed-form
scores and responses), and the view poses come from running the reference's PoseUtils (tests/golden/make_golden_views.py)."""
import os

import numpy as np
import pytest

import orb_ref
from ffb6d_amd import objinfo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "view_poses.npz")


def detect_gray(g, L=1, t=20, edge=4, quota=(16,)):
    return orb_ref.detect(orb_ref.as_rgb(g)[None], L, t, edge, quota)


def test_gray_of_a_gray_pixel_is_the_pixel_and_the_weights_round():
    g = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(orb_ref.gray(orb_ref.as_rgb(g)), g)
    rgb = np.array([[[255]], [[0]], [[0]]], np.uint8)
    assert orb_ref.gray(rgb)[0, 0] == (4899 * 255 + 8192) >> 14 == 76
    assert orb_ref.gray(rgb[[1, 0, 2]])[0, 0] == 150 and orb_ref.gray(rgb[[2, 1, 0]])[0, 0] == 29


def test_isolated_dots_have_their_closed_form_scores_responses_and_order():
    g = orb_ref.dots_image()
    s = orb_ref.fast_scores(g)
    assert [int(s[y, x]) for x, y, _ in orb_ref.DOTS] == [170, 90, 220, 30, 21, 20, 170]
    count, kps, resp = detect_gray(g)
    assert count[0] == 6                                       # (54,38): its score of 20 is not above t
    assert kps[0, :6, :2].tolist() == [[50, 14], [10, 10], [12, 40], [30, 12], [20, 30], [40, 34]]
    assert (kps[0, :6, 2] == 0).all() and np.array_equal(kps[0, :6, 3:], kps[0, :6, :2])      # level 0: (X, Y) = (x, y)
    assert resp[0, :6].tolist() == [7083901440000, 2525675040000, 2525675040000, 198404640000, 2449440000, 588110544]
    assert (kps[0, 6:] == -1).all() and not resp[0, 6:].any()
    # a dot of height h on a flat image: Ix and Iy are h * (1, 2, 1) on two sides of it, a = b = 12 h^2, c = 0: resp = 3024 h^4
    assert resp[0, :6].tolist() == [3024 * h ** 4 for h in (220, 170, 170, 90, 30, 21)]


def test_the_summed_area_form_of_the_response_equals_the_7x7_sums():
    g = orb_ref.gray(orb_ref.noise_rgb(24, 31, 3))
    m = orb_ref.harris_map(g)
    assert all(int(m[y, x]) == orb_ref.harris(g, x, y) for y in range(4, 20) for x in range(4, 27))
    step = np.full((24, 31), 10, np.uint8)
    step[:, 15:] = 90                                           # a straight edge: a = 7 * 2 * 320^2, b = c = 0, resp = -a^2
    assert orb_ref.harris_map(step)[12, 15] == orb_ref.harris(step, 15, 12) == -(14 * 320 ** 2) ** 2


def test_ties_and_flat_images_give_no_keypoints():
    rect = np.full((48, 64), 30, np.uint8)
    rect[15:30, 20:45] = 200
    board = (((np.arange(48)[:, None] // 8 + np.arange(64)[None] // 8) % 2) * 200 + 20).astype(np.uint8)
    for g in (rect, board, np.full((48, 64), 77, np.uint8)):
        count, kps, resp = detect_gray(g)
        assert count[0] == 0 and (kps == -1).all() and not resp.any()
    assert orb_ref.fast_scores(rect).max() > 20                # the corners do score: strict NMS removes the tied pairs


def test_level_sizes_quotas_and_the_level_0_pixel():
    assert orb_ref.level_sizes(480, 640, 8) == [(480, 640), (400, 533), (333, 444), (278, 370), (231, 309), (193, 257), (161, 214), (134, 179)]
    assert orb_ref.level_sizes(37, 53, 8) == [(37, 53), (31, 44), (26, 37), (21, 31), (18, 26), (15, 21), (12, 18), (10, 15)]
    for n in (37, 53, 480, 640):
        for l in range(8):
            assert orb_ref.level_size(n, l) == int(np.floor(n / 1.2 ** l + 0.5))
    q = objinfo.orb_quotas(500, 8)
    assert q.tolist() == [109, 90, 75, 63, 52, 44, 36, 31] and q.sum() == 500 and q.dtype == np.int32
    assert np.array_equal(q, orb_ref.quotas(500, 8))
    assert objinfo.orb_quotas(500, 1).tolist() == [500] and objinfo.orb_quotas(7, 3).sum() == 7
    for bad in ((0, 8), (500, 0), (500, 9)):
        with pytest.raises(ValueError):
            objinfo.orb_quotas(*bad)


def test_resize_keeps_a_constant_and_the_order_of_a_ramp():
    for size in ((48, 64), (37, 53)):
        (h, w), (h1, w1) = orb_ref.level_sizes(*size, 2)
        assert (orb_ref.resize(np.full((h, w), 93, np.uint8), h1, w1) == 93).all()
        ramp = np.broadcast_to((np.arange(w) * 255 // (w - 1)).astype(np.uint8), (h, w))
        out = orb_ref.resize(ramp, h1, w1)
        assert out.shape == (h1, w1) and (np.diff(out.astype(int), axis=1) >= 0).all() and (out == out[0]).all()
        assert out[0, 0] <= 3 and out[0, -1] >= 252
    pyr = orb_ref.pyramid(np.zeros((37, 53), np.uint8), 8)
    assert [p.shape for p in pyr] == orb_ref.level_sizes(37, 53, 8)


def test_keypoints_of_upper_levels_map_into_the_frame():
    rgb = orb_ref.noise_rgb(48, 64, 1)[None]
    count, kps, resp = orb_ref.detect(rgb, 3, 20, 4, (16, 8, 4))
    k = kps[0, :count[0]]
    assert count[0] == 28 and (np.diff(k[:, 2]) >= 0).all() and set(k[:, 2]) == {0, 1, 2}      # by level ...
    for l in range(3):
        r = resp[0, :count[0]][k[:, 2] == l]
        assert (np.diff(r) <= 0).all()                                                          # ... then by response
    sizes = orb_ref.level_sizes(48, 64, 3)
    for x, y, l, X, Y in k:
        assert X == (2 * x + 1) * 64 // (2 * sizes[l][1]) and Y == (2 * y + 1) * 48 // (2 * sizes[l][0])
        assert 0 <= X < 64 and 0 <= Y < 48 and abs(X + 0.5 - (x + 0.5) * 1.2 ** l) < 1.5


def test_view_poses_equal_the_reference():
    gold = np.load(GOLDEN)
    for c, (r, n1, n2) in enumerate(zip(gold["radius"], gold["n1"], gold["n2"])):
        want = gold[f"poses{c}"]
        got = objinfo.view_poses(float(r), int(n1), int(n2))
        assert got.shape == (1, n1 * n2, 3, 4) and got.dtype == np.float64
        assert np.abs(got[0] - want[:, :3]).max() <= 1e-12, c
        assert np.array_equal(want[:, 3], np.broadcast_to([0, 0, 0, 1.0], want[:, 3].shape))
    both = objinfo.view_poses(gold["radius"][:2], 3, 3)
    assert np.abs(both[1] - gold["poses1"][:, :3]).max() <= 1e-12
    assert np.array_equal(both[0, :, :, :3], both[1, :, :, :3])                # the rotations do not depend on the radius


def test_view_poses_are_rigid_and_look_at_the_origin():
    poses = objinfo.view_poses([0.035, 0.11, 0.3], 3, 3)
    R, t = poses[..., :3], poses[..., 3]
    assert np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max() < 1e-14 and np.abs(np.linalg.det(R) - 1).max() < 1e-14
    K = np.array(objinfo.DEFAULT_K)
    uv = t @ K.T
    assert np.abs(uv[..., :2] / uv[..., 2:] - [320, 240]).max() < 1e-9         # the origin projects to (cx, cy)
    assert np.allclose(t[..., 2], (np.array([0.035, 0.11, 0.3]) / 0.035 * 0.18)[:, None], rtol=1e-15, atol=0)
    assert len({tuple(np.round(r.reshape(-1), 9)) for r in R[0]}) == 9         # nine different views


def test_lift_returns_the_points_of_a_fronto_parallel_plane():
    H, W, Q = 24, 32, 6
    K = np.array([[40.0, 0, 16], [0, 40, 12], [0, 0, 1]])
    T = np.array([[[0.0, 1, 0, 0.02], [-1, 0, 0, -0.01], [0, 0, 1, 0.1]]])     # a quarter turn about z, the plane z_obj = 0.4
    depth = np.full((1, H, W), 0.5, np.float32)
    kps = np.full((1, Q, 5), -1, np.int32)
    kps[0, :5, 3:] = [[16, 12], [0, 0], [31, 23], [20, 4], [7, 19]]
    depth[0, 4, 20] = 0                                        # a hole under row 3
    depth[0, 19, 7] = np.inf
    count, visible = np.array([5], np.int32), np.array([600], np.int32)
    pts, ok = orb_ref.lift(kps, count, depth, visible, T, K)
    assert ok[0].tolist() == [1, 1, 1, 0, 0, 0] and not pts[0, 3:].any()
    for r in range(3):
        X, Y = kps[0, r, 3:]
        cam = np.array([(X - 16) * 0.5 / 40, (Y - 12) * 0.5 / 40, 0.5])
        want = (cam - T[0, :, 3]) @ T[0, :, :3]
        assert np.abs(pts[0, r] - want).max() < 1e-7 and abs(pts[0, r, 2] - 0.4) < 1e-7
    cp, begin, n_found = orb_ref.compact(pts, ok, 1, 1)
    assert n_found.tolist() == [3] and begin.tolist() == [0, 3] and np.array_equal(cp[:3], pts[0, :3]) and not cp[3:].any()
    assert not orb_ref.lift(kps, count, depth, np.array([499], np.int32), T, K)[1].any()       # below min_pixels = 500
    depth[0, 12, 16] = np.nan
    assert orb_ref.lift(kps, count, depth, visible, T, K)[1][0].tolist() == [0, 1, 1, 0, 0, 0]  # the order is kept


def test_from_meshes_and_orb_detect_refuse_what_the_host_can_judge():
    with pytest.raises(ValueError):
        objinfo.ObjectInfo.from_meshes([None], keypoints="sift")
    with pytest.raises(TypeError):
        objinfo.orb_detect(np.zeros((1, 3, 48, 64), np.uint8))
    with pytest.raises(ValueError):
        objinfo._detector(500, 8, 20, 3)
    with pytest.raises(ValueError):
        objinfo._detector(500, 8, 256, 31)
