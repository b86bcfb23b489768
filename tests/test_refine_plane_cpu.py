"""The numpy restatement of the point-to-plane metric (tests/icp_plane_ref.py) on its own, without a GPU and without the
emulator: it refines, and faster than the point metric; it leaves alone what a plane and a sphere do not determine; and the cases
the emulator and device tests hold the kernels against have no truncation decision on a rounding edge and no float32 / float64
tie, so those tests excuse nothing."""
import numpy as np
import pytest

import icp_plane_ref as pref
import icp_ref
from ffb6d_amd import synth

# chosen like REFINE_SEEDS of tests/test_refine_gpu.py, by running the restatement on the CPU (surface model 100 + seed with 2048
# points and 16-neighbour normals, view 200 + seed, synth.eval_pose_pair(seed, "near"), max_dist 0.02): ADD in mm before / point
# metric after 10 iterations / plane metric after 5 --
#   0: 12.3 / 3.68 / 0.70   1: 18.5 / 2.92 / 0.74   3: 20.2 / 2.23 / 0.60   5: 27.1 / 6.90 / 3.15   6: 21.5 / 2.89 / 0.56   9: 19.2 / 2.12 / 0.21
# (seeds 4, 10, 11 and 15 start within 15 mm and the point metric ends below the plane metric's 0.6 - 1.8 mm noise floor there)
REFINE_SEEDS = (0, 1, 3, 5, 6, 9)
# the device test's batches (tests/test_refine_plane_gpu.py): models of 1024 - 4096 points
VIEW_SEEDS, VIEW_SIZES = (0, 1, 3, 5), (1024, 2048, 4096, 1536)
INST_SEEDS = (0, 1, 3)
MIN_EIG = 1e-6


def clear_of_the_edge(eig, min_eig=MIN_EIG):
    r = pref.eig_ratios(eig)
    return not np.any((r >= min_eig / 10) & (r <= 10 * min_eig))


@pytest.fixture(scope="module")
def refine_runs():
    out = []
    for s in REFINE_SEEDS:
        m, n = pref.model_with_normals(100 + s, 2048)
        pred, gt = (x.astype(np.float64) for x in synth.eval_pose_pair(s, "near"))
        scene = icp_ref.partial_view(m, gt, 200 + s)
        point = icp_ref.icp(scene, m, pred, 10, 0.02)
        plane = pref.icp_plane(scene, m, n, pred, 5, 0.02, min_eig=MIN_EIG)
        out.append(dict(before=icp_ref.add(m, pred, gt), point=icp_ref.add(m, point["T"], gt), plane=icp_ref.add(m, plane["T"], gt), run=plane))
    return out


def test_plane_after_5_beats_point_after_10(refine_runs):
    before, point, plane = (np.array([r[k] for r in refine_runs]) for k in ("before", "point", "plane"))
    print("ADD mm before", 1e3 * before, "point x10", 1e3 * point, "plane x5", 1e3 * plane)
    assert (plane * 5 <= before).all()                                            # every case is one the restatement refines 5 x
    assert plane.mean() < point.mean()
    assert all(r["run"]["iters"] == 5 and clear_of_the_edge(r["run"]["eig"]) for r in refine_runs)
    assert all(r["run"]["rms_plane"] < r["run"]["rms"] for r in refine_runs)      # a projection of the same residuals


def test_a_planar_model_keeps_its_in_plane_pose():
    """A 32 x 32 grid with its exact normal: rotation about the normal and the two in-plane shifts are eigenvalues (numerically)
    zero and are truncated; two iterations remove the out-of-plane residual and move nothing in the plane."""
    pts, normals = pref.planar_grid(32)
    T0, gt = pref.off_pose(4, deg=3.0, shift=0.004)
    rng = np.random.RandomState(1)
    scene = (pts[rng.randint(0, len(pts), 400)].astype(np.float64) + [0.0005, -0.0003, 0.0]) @ gt[:, :3].T + gt[:, 3]
    scene = scene.astype(np.float32)
    one = pref.icp_plane(scene, pts, normals, T0, 1, 0.05, min_eig=MIN_EIG)
    lam, used = one["eig"][0]
    assert used.sum() == 3 and np.all(np.abs(lam[~used]) <= 1e-12 * lam.max())
    two = pref.icp_plane(scene, pts, normals, T0, 2, 0.05, min_eig=MIN_EIG)
    q = icp_ref.to_model_frame(scene, two["T"], np.float64)
    assert np.abs(q[:, 2]).max() <= 1e-6                                          # (float32 scene points: 1e-7 at a depth of 0.8 m)
    c, _ = pref.class_constants(pts)
    assert np.abs(pref.in_plane_motion(T0, two["T"], c)).max() <= 1e-6
    assert clear_of_the_edge(two["eig"])


def test_a_sphere_keeps_its_rotation_and_finds_its_centre():
    pts, normals = pref.sphere_cloud(2, 1024)
    T0, gt = pref.off_pose(6, deg=10.0, shift=0.006)
    scene = icp_ref.partial_view(pts, gt, 9, noise=0.0, clutter=0.0)
    # A SAMPLED sphere: a scene point lies up to half the sample spacing (5.5 mm at 1024 points, radius 50 mm) beside its model
    # point, so u x n is (offset / radius) |u|, not zero, and the rotational eigenvalues are ~ (0.05)^2 / 2 ~ 1e-3 of the
    # translational ones.  A user with such an object asks for min_eig between the two groups; 0.05 is a decade from either.
    run = pref.icp_plane(scene, pts, normals, T0, 6, 0.02, min_eig=0.05)
    assert run["iters"] == 6
    for lam, used in run["eig"]:
        assert used.sum() == 3 and np.all(lam[:3] <= 0.005 * lam.max()) and np.all(lam[3:] >= 0.5 * lam.max())
    Rm = run["T"][:, :3] @ T0[:, :3].T
    moved = np.degrees(np.arccos(np.clip((np.trace(Rm) - 1) / 2, -1, 1)))
    assert moved <= 0.1                                                           # the rotation, 10 degrees off, is left where it is
    # the centre: from 6 mm to within a tenth of the sample spacing
    assert np.linalg.norm(run["T"][:, 3] - gt[:, 3]) <= 5.5e-4 < 0.005 < np.linalg.norm(T0[:, 3] - gt[:, 3])


def test_the_parity_cases_sit_on_no_edge():
    """What the device test excuses by `first_divergence` is decided here: none of its cases has a float32 / float64 tie, and none
    has an eigenvalue ratio within a decade of min_eig."""
    case, models, normals = pref.view_case(VIEW_SEEDS, VIEW_SIZES)
    for p in range(len(VIEW_SEEDS)):
        cls = int(case["class_of"][p])
        scene = icp_ref.problem_scene(case["pcld"], case["mask"], int(case["frame_of"][p]), cls)
        assert 500 <= len(scene) <= 900
        for max_dist, tol, iters in ((0.01, 0.0, 5), (0.02, 1e-5, 12)):
            assert pref.first_divergence(scene, models[cls], normals[cls], case["T0"][p], iters, max_dist, tol) is None
            assert clear_of_the_edge(pref.icp_plane(scene, models[cls], normals[cls], case["T0"][p], iters, max_dist, tol)["eig"])
    case, models, normals = pref.instance_view_case(INST_SEEDS)
    args = (case["pcld"], case["mask"], case["inst"], case["T0"], case["frame_of"], case["class_of"], case["inst_of"], models, normals)
    for mode in ("map", "nearest"):
        assert pref.first_divergence_instances(*args, 5, 0.02, mode) == [None] * 6
        assert all(clear_of_the_edge(e) for e in pref.icp_refine_plane_instances(*args, 5, 0.02, mode)[1]["eig"])


def test_given_normals_and_the_sign_rule():
    n = pref.given_normals([[0, 0, 2], [3, 4, 0], [0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 0], [1e-30, 0, 0]])
    assert np.array_equal(n[:3], np.float32([[0, 0, 1], [0.6, 0.8, 0], [0, 0, 0]])) and not n[3:5].any() and n[5, 0] == 1
    assert np.array_equal(pref.oriented(np.array([0.5, -0.5, 0.1])), [0.5, -0.5, 0.1])      # a tie: the lowest axis decides
    assert np.array_equal(pref.oriented(np.array([-0.5, 0.5, 0.1])), [0.5, -0.5, -0.1])
    assert np.array_equal(pref.oriented(np.array([0.1, -0.9, 0.2])), [-0.1, 0.9, -0.2])
    line = np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]])
    assert not pref.estimate_normals(line)[0].any() and not pref.estimate_normals(line[:2])[0].any()
