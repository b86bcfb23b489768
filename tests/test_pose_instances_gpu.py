"""The multi-instance pose solver on the device (ffb6d_amd/pose.py: mean_shift_multi, MeanShiftTorch.fit_multi_clus, solve_instances;
include/ffb6d_pose.h states the rule) against
  * outputs of the reference's MeanShiftTorch.fit_multi_clus (tests/golden/ms_multi.npz),
  * the single fit, as bits (cluster 1), at set sizes either side of every form threshold,
  * the numpy restatement (tests/pose_instances_ref.py) on the kernels' own converged points,
  * solve_poses (one instance per class: the same bits), true poses of frames with several instances of a class, and
    bop.BOPSceneEval, which takes the solver's output as it is.
Tolerances: CTR_TOL and POSE_TOL of tests/test_pose_gpu.py.  The golden cases have no converged pair near the bandwidth and compare
clusters of pairwise different sizes only (asserted by their generator), so labels and ball sizes are compared exactly."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import pose_instances_ref as ref
import test_pose_instances_cpu as cpu_side
from conftest import GOLDEN
from ffb6d_amd import _lib, pose, synth

pytestmark = pytest.mark.gpu

CTR_TOL = 5e-4
POSE_TOL = 5e-3
gen = cpu_side.gen

spec = importlib.util.spec_from_file_location("make_golden_pose", os.path.join(GOLDEN, "make_golden_pose.py"))
single_gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(single_gen)


def pack(clouds, stride, device):
    sets = torch.zeros((len(clouds), stride, 4), device=device)
    for g, c in enumerate(clouds):
        if len(c):
            sets[g, :len(c), :3] = torch.from_numpy(np.ascontiguousarray(c, np.float32)).to(device)
    return sets, torch.tensor([len(c) for c in clouds], dtype=torch.int32, device=device)


def multi_with_points(sets, counts, bw, K, min_inside=1, max_iter=300):
    """mean_shift_multi + the converged point of every vote (the test hook of include/ffb6d_pose.h)"""
    conv = torch.zeros_like(sets)
    lib = _lib.load()
    lib.ffb6d_pose_set_converged_out(conv.data_ptr())
    try:
        out = pose.mean_shift_multi(sets, counts, bw, K, min_inside, max_iter)
        torch.cuda.synchronize()
    finally:
        lib.ffb6d_pose_set_converged_out(None)
    return out, conv


def equal_results(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "ms_multi.npz"))


@pytest.mark.parametrize("i", range(len(gen.CASES)))
def test_fit_multi_clus_matches_the_reference(device, gold, i):
    seed, sizes, outliers, bw = gen.CASES[i]
    votes = torch.from_numpy(gen.mixture(seed, sizes, outliers)).to(device)
    centres, labels, n_in = pose.MeanShiftTorch(bandwidth=bw).fit_multi_clus(votes)
    assert isinstance(centres, list) and isinstance(n_in, list) and labels.dtype == torch.int32 and tuple(labels.shape) == (len(votes),)
    assert all(isinstance(n, int) for n in n_in) and all(tuple(c.shape) == (3,) for c in centres)
    cpu_side.check_against_reference(gold, i, torch.stack(centres).cpu().numpy(), labels.cpu().numpy(), n_in)
    # a cap: the first clusters of the same sequence, later points labelled 0
    c2, l2, n2 = pose.MeanShiftTorch(bandwidth=bw).fit_multi_clus(votes, max_clusters=2)
    assert n2 == n_in[:2] and all(torch.equal(a, b) for a, b in zip(c2, centres)) and torch.equal(l2, torch.where(labels <= 2, labels, 0))


THRESHOLD_SIZES = (0, 1, 40, 511, 512, 513, 2048, 2049, 4096, 4200)      # kSpreadMin, kCapLight, kCap, the chip-wide rounds


@pytest.fixture(scope="module")
def threshold_sets(device):
    """two-blob vote sets (the ones tests/test_pose_gpu.py fits) of every threshold size behind one stride"""
    clouds = [single_gen.ms_votes(900 + g, n) if n else np.zeros((0, 3), np.float32) for g, n in enumerate(THRESHOLD_SIZES)]
    return clouds, pack(clouds, max(THRESHOLD_SIZES), device)


def test_cluster_one_is_the_single_fit_as_bits(device, threshold_sets):
    clouds, (sets, counts) = threshold_sets
    (centers, cluster, n_in, n_clus, rounds), conv = multi_with_points(sets, counts, 0.04, 3)
    s_centers, s_labels, s_n_in, s_rounds = pose.mean_shift(sets, counts, 0.04)
    assert torch.equal(centers[:, 0], s_centers) and torch.equal(n_in[:, 0], s_n_in) and torch.equal(rounds, s_rounds)
    assert torch.equal(cluster == 1, s_labels)
    assert n_clus.tolist()[:2] == [0, 1] and all(n >= 2 for n in n_clus.tolist()[2:])      # two blobs (and stragglers)
    # the peel itself, on the converged points of each form: one-workgroup fit (light / large), chip-wide rounds then the fit
    for g in (2, 5, 7, 9):
        M = THRESHOLD_SIZES[g]
        C = conv[g, :M, :3].cpu().numpy()
        w_centres, w_cluster, w_n_in = ref.peel(C, 0.04, 3, 1)
        k = len(w_n_in)
        assert int(n_clus[g]) == k and n_in[g, :k].tolist() == w_n_in and not n_in[g, k:].any() and not centers[g, k:].any(), g
        assert np.array_equal(cluster[g, :M].cpu().numpy(), w_cluster) and not cluster[g, M:].any(), g
        assert np.array_equal(centers[g, :k].cpu().numpy().view(np.uint32), w_centres.view(np.uint32)), g


def test_round_by_round_sets_peel_too(device, threshold_sets):
    """big_form = 0: the sets of more than 4096 points stay with the round-by-round kernels and are peeled by one workgroup on
    the converged points; cluster 1 is that path's single fit, the peel equals the restatement, and the result agrees with the
    chip-wide form to rounding (include/ffb6d_pose.h, ffb6d_pose_set_big_form)"""
    clouds, _ = threshold_sets
    lattice = np.stack(np.meshgrid(*[np.arange(17, dtype=np.float32) * 0.2] * 3, indexing="ij"), -1).reshape(-1, 3)      # 4913 points that never meet
    mixed = [clouds[9], clouds[2], lattice, ref.blobs(8, (2500, 1200, 600))]
    sets, counts = pack(mixed, 4913, device)
    lib = _lib.load()
    base = pose.mean_shift_multi(sets, counts, 0.04, 4)
    try:
        lib.ffb6d_pose_set_big_form(0)
        (centers, cluster, n_in, n_clus, rounds), conv = multi_with_points(sets, counts, 0.04, 4)
        s_centers, s_labels, s_n_in, s_rounds = pose.mean_shift(sets, counts, 0.04)
    finally:
        lib.ffb6d_pose_set_big_form(1)
    assert torch.equal(centers[:, 0], s_centers) and torch.equal(n_in[:, 0], s_n_in) and torch.equal(cluster == 1, s_labels)
    assert torch.equal(rounds, s_rounds)
    for g, c in enumerate(mixed):
        M = len(c)
        w_centres, w_cluster, w_n_in = ref.peel(conv[g, :M, :3].cpu().numpy(), 0.04, 4, 1)
        assert n_in[g].tolist() == (w_n_in + [0] * 4)[:4] and int(n_clus[g]) == len(w_n_in), g
        assert np.array_equal(cluster[g, :M].cpu().numpy(), w_cluster) and not cluster[g, M:].any(), g
        assert np.array_equal(centers[g, :len(w_n_in)].cpu().numpy().view(np.uint32), w_centres.view(np.uint32)), g
    assert n_in[2].tolist() == [1, 1, 1, 1] and cluster[2, :5].tolist() == [1, 2, 3, 4, 0]      # the lattice: ties, lowest index first
    assert n_in[3].tolist() == base[2][3].tolist() == [2500, 1200, 600, 0]
    assert all(abs(a - b) <= max(1, int(0.005 * 4200)) for a, b in zip(n_in[0].tolist(), base[2][0].tolist()))      # LABEL_FLIP of test_pose_gpu.py
    assert (centers[3, :3] - base[0][3, :3]).abs().max() <= CTR_TOL and torch.equal(cluster[3], base[1][3])
    assert torch.equal(cluster[2], base[1][2]) and torch.equal(centers[2], base[0][2])          # never merges: the same kernels in both


BATCH = ((40, (20, 13, 7)), (513, (300, 213)), (1, (1,)), (2000, (900, 600, 300, 150, 50)), (64, (64,)), (700, (400, 200, 100)), (0, ()))


@pytest.mark.parametrize("K", [1, 4])
def test_batch_equals_single_sets(device, K):
    """sets of different sizes and cluster counts in one call equal their own single-set calls bit for bit"""
    clouds = [ref.blobs(40 + g, sizes) if n else np.zeros((0, 3), np.float32) for g, (n, sizes) in enumerate(BATCH)]
    assert [len(c) for c in clouds] == [n for n, _ in BATCH]
    sets, counts = pack(clouds, 2000, device)
    sets[:, :, :3] += torch.where(torch.arange(2000, device=device)[None, :, None] >= counts[:, None, None], 7.0, 0.0)      # padding differs
    batch = pose.mean_shift_multi(sets, counts, 0.04, K)
    for g, c in enumerate(clouds):
        s1, c1 = pack([c], max(len(c), 1), device)
        alone = pose.mean_shift_multi(s1, c1, 0.04, K)
        M = len(c)
        assert torch.equal(alone[0][0], batch[0][g]) and torch.equal(alone[1][0, :M], batch[1][g, :M]) and not batch[1][g, M:].any(), g
        assert torch.equal(alone[2][0], batch[2][g]) and int(alone[3][0]) == int(batch[3][g]) == min(K, len(BATCH[g][1])), g
        assert int(alone[4][0]) == int(batch[4][g])
        assert batch[2][g].tolist() == (list(BATCH[g][1]) + [0] * K)[:K], (g, batch[2][g].tolist())


def test_forms_give_the_same_bits(device):
    """the loop of tests/test_pose_gpu.py::test_mean_shift_forms_give_the_same_bits on the multi entry"""
    lib = _lib.load()
    sizes = (511, 512, 513, 1700, 2048, 2049, 3000, 4096, 40, 0, 900, 640)
    clouds = []
    for g, n in enumerate(sizes):
        v = ref.blobs(700 + g, (n - n // 2 - n // 5, n // 2, n // 5), spread=0.02) if n else np.zeros((0, 3), np.float32)
        if g in (10, 11):                                      # every vote of these sets twice: round 0 finds duplicates
            v[n // 2:] = v[:n - n // 2]
        clouds.append(v)
    sets, counts = pack(clouds, 4096, device)
    got = {}
    try:
        for form, spread in ((1, 2), (1, 1), (1, 0), (0, 2), (0, 0)):
            lib.ffb6d_pose_set_fit_form(form)
            lib.ffb6d_pose_set_fit_spread(spread)
            got[form, spread] = [t.clone() for t in pose.mean_shift_multi(sets, counts, 0.04, 4)]
            for limit in (0, 1, 2):                            # round limits inside the spread rounds: thousands of distinct points peel
                got[form, spread] += [t.clone() for t in pose.mean_shift_multi(sets, counts, 0.04, 4, 1, limit)]
    finally:
        lib.ffb6d_pose_set_fit_form(1)
        lib.ffb6d_pose_set_fit_spread(1)
    base = got[0, 0]
    assert int(base[4][3]) > 3 and int(base[4][10]) > 3 and all(n >= 3 for n in base[3].tolist()[:9])      # real fits, three blobs each
    for key, res in got.items():
        for a, b in zip(base, res):
            assert torch.equal(a, b), key


def test_caps_and_min_inside(device, gold):
    seed, sizes, outliers, bw = gen.CASES[3]                    # [601, 130, 62, 3, 2, 2, 1, ...]: 16 clusters
    want = [int(n) for n in gold["c3_n_in"]]
    votes = gen.mixture(seed, sizes, outliers)
    sets, counts = pack([votes, votes[:0], gen.mixture(*gen.CASES[1][:3])], len(votes), device)
    full = pose.mean_shift_multi(sets, counts, bw, 40)
    assert full[3].tolist() == [len(want), 0, 3] and full[2][0, :len(want)].tolist() == want
    assert not full[2][0, len(want):].any() and not full[0][0, len(want):].any() and not full[2][2, 3:].any() and not full[0][2, 3:].any()
    assert not full[0][1].any() and not full[2][1].any() and not full[1][1].any()
    assert int(full[1][0].max()) == len(want) and int((full[1][0] == 0).sum()) == 0
    for K in (1, 2, 5):                                         # more clusters than K: the prefix
        capped = pose.mean_shift_multi(sets, counts, bw, K)
        assert capped[3].tolist() == [K, 0, min(K, 3)]
        assert torch.equal(capped[0], full[0][:, :K]) and torch.equal(capped[2], full[2][:, :K])
        assert torch.equal(capped[1], torch.where(full[1] <= K, full[1], 0))
    for min_inside in (2, 3, 4, 63, 700):                       # cuts exactly the smaller balls
        keep = sum(n >= min_inside for n in want)
        cut = pose.mean_shift_multi(sets, counts, bw, 40, min_inside)
        assert cut[3].tolist() == [keep, 0, 3 if min_inside <= 100 else 0], min_inside
        assert torch.equal(cut[2][0, :keep], full[2][0, :keep]) and not cut[2][0, keep:].any() and not cut[0][0, keep:].any()
        assert torch.equal(cut[1][0], torch.where(full[1][0] <= keep, full[1][0], 0))


# ---- the solver ------------------------------------------------------------------------------------------------------------
def stacked(cases, device):
    up = lambda key: torch.from_numpy(np.stack([c[key] for c in cases])).to(device)      # noqa: E731
    return up("pcld"), up("mask"), up("ctr_of"), up("kp_of")


@pytest.mark.parametrize("classes", [None, [1, 2, 3, 4]], ids=["present", "listed"])
def test_one_instance_per_class_gives_the_poses_of_solve_poses_as_bits(device, classes):
    cases = [synth.make_pose_case(700 + k, n_pts=1500, n_obj=3, n_cls=5, mesh_seed=7) for k in range(3)]
    cases[1]["mask"][:] = 0                                              # nothing to solve in frame 1
    cases[2]["mask"][cases[2]["mask"] == 2] = 0                          # class 2 absent in frame 2
    frames = stacked(cases, device)
    mesh_kps, mesh_ctr = cases[0]["mesh_kps"], cases[0]["mesh_ctr"]
    want = pose.solve_poses(*frames, mesh_kps, mesh_ctr, use_ctr_clus_flter=True, refine_mask=False, classes=classes)
    got = pose.solve_instances(*frames, mesh_kps, mesh_ctr, 1, min_inside=1, classes=classes)
    assert got["est_RT"].dtype == torch.float64 and got["est_score"].dtype == torch.float32 and got["kps"].dtype == torch.float32
    assert all(got[k].dtype == torch.int32 for k in ("est_class", "est_frame", "est_instance", "n_inside")) and all(v.is_cuda for v in got.values())
    rows = {(int(f), int(c)): e for e, (f, c) in enumerate(zip(got["est_frame"].tolist(), got["est_class"].tolist()))}
    n = 0
    for b, (ids, poses, kps) in enumerate(want):
        for c, T, k in zip(ids, poses, kps):
            if int((cases[b]["mask"] == c).sum()) == 0:                  # solve_poses: the identity; here: no row
                assert (b, int(c)) not in rows
                continue
            e = rows[(b, int(c))]
            n += 1
            assert np.array_equal(got["est_RT"][e].cpu().numpy(), T) and np.array_equal(got["kps"][e].cpu().numpy(), k), (b, c)
    assert n == len(rows) == int(got["est_RT"].shape[0]) and n >= 5 and got["est_instance"].tolist() == [1] * n
    order = list(zip(got["est_frame"].tolist(), got["est_class"].tolist()))
    assert order == sorted(order)


@pytest.fixture(scope="module")
def multi_frames():
    return ref.make_multi_instance_frames(31)                            # 2 and 3 instances of class 1, one of class 2; 0.4 m apart


def test_frames_with_several_instances_of_a_class(device, multi_frames):
    f = multi_frames
    frames = [torch.from_numpy(f[k]).to(device) for k in ("pcld", "mask", "ctr_of", "kp_of")]
    stats = {}
    got = pose.solve_instances(*frames, f["mesh_kps"], f["mesh_ctr"], max_instances=4, min_fraction=0.05, stats=stats)
    keys = list(zip(got["est_frame"].tolist(), got["est_class"].tolist(), got["est_instance"].tolist()))
    assert keys == [(0, 1, 1), (0, 1, 2), (0, 2, 1), (1, 1, 1), (1, 1, 2), (1, 1, 3), (1, 2, 1)], keys      # the true counts, in order
    T = got["est_RT"].cpu().numpy()
    taken = set()
    for b, placed in enumerate(f["poses"]):
        for c, RT in placed:
            errs = [(float(np.abs(T[e] - RT).max()), e) for e, k in enumerate(keys) if k[:2] == (b, c)]
            err, e = min(errs)
            print("frame", b, "class", c, "pose err", err)
            assert err <= POSE_TOL and e not in taken, (b, c, err)
            taken.add(e)
    assert len(taken) == len(keys)
    score, n_in = got["est_score"].cpu().numpy(), got["n_inside"].cpu().numpy()
    assert ((score > 0) & (score <= 1)).all() and (n_in >= 1).all()
    for b in (0, 1):
        for c in (1, 2):
            sel = [e for e, k in enumerate(keys) if k[:2] == (b, c)]
            total = int((f["mask"][b] == c).sum())
            assert score[sel].sum() <= 1.0 and np.array_equal(score[sel], n_in[sel].astype(np.float32) / np.float32(total))
            assert all(n_in[sel][i] >= n_in[sel][i + 1] for i in range(len(sel) - 1))
    assert all(n >= true for n, true in zip(stats["n_clusters"].tolist(), (2, 1, 3, 1)))      # (outlier votes form further clusters: min_fraction drops them)
    # the capability is the difference: one pose per (frame, class) from solve_poses
    one = pose.solve_poses(*frames, f["mesh_kps"], f["mesh_ctr"], use_ctr_clus_flter=True, refine_mask=False)
    assert [ids.tolist() for ids, _, _ in one] == [[1, 2], [1, 2]] and all(p.shape == (2, 3, 4) for _, p, _ in one)
    # and the restatement's dataflow gives the same rows
    want = ref.solve_instances(f["pcld"], f["mask"], f["ctr_of"], f["kp_of"], f["mesh_kps"], f["mesh_ctr"], 4, 1, 0.05)
    assert [(r["frame"], r["cls"], r["instance"]) for r in want] == keys
    assert all(abs(r["n_inside"] - int(n)) <= max(1, int(0.005 * r["n_inside"])) for r, n in zip(want, n_in))      # LABEL_FLIP of test_pose_gpu.py
    kps = got["kps"].cpu().numpy()
    for e, r in enumerate(want):
        assert np.abs(kps[e] - r["kps"]).max() <= CTR_TOL and np.abs(T[e] - r["RT"]).max() <= POSE_TOL, e


def test_the_solvers_output_goes_into_the_scene_evaluator(device):
    from ffb6d_amd import bop, evaluate, render
    import render_ref
    H, W = 96, 128
    K = np.stack([render_ref.SMALL_K * np.array([[2.0], [2.0], [1.0]])] * 2)      # one per frame (a single [3,3] K means a single frame to bop)
    meshes = [None, synth.sphere_mesh(2, 0.1, seed=3), synth.sphere_mesh(1, 0.07, seed=5)]
    rng = np.random.RandomState(5)
    P = lambda t: render_ref.pose(t, synth.random_rotation(rng))         # noqa: E731
    placed = [[(1, P([-0.2, 0.0, 0.6])), (1, P([0.2, 0.02, 0.62])), (2, P([0.0, -0.12, 0.5]))],
              [(1, P([-0.3, 0.03, 0.66])), (1, P([0.02, 0.0, 0.6])), (1, P([0.33, -0.02, 0.64])), (2, P([0.15, 0.13, 0.5]))]]
    f = ref.make_multi_instance_frames(9, placed=placed, local=lambda c, r: meshes[c]["xyz"][r.randint(len(meshes[c]["xyz"]))])
    gt_RT = np.stack([RT for fr in placed for _, RT in fr])
    gt_class = np.array([c for fr in placed for c, _ in fr], np.int32)
    gt_frame = np.array([b for b, fr in enumerate(placed) for _ in fr], np.int32)
    prepared = render.PreparedMeshes(meshes, device)
    depth = render.render(prepared, gt_RT, gt_frame, gt_class, K, 2, H, W, outputs=("depth",))["depth"]
    assert int((depth > 0).sum()) > 500
    frames = [torch.from_numpy(f[k]).to(device) for k in ("pcld", "mask", "ctr_of", "kp_of")]
    got = pose.solve_instances(*frames, f["mesh_kps"], f["mesh_ctr"], max_instances=4, min_fraction=0.05)
    assert int(got["est_RT"].shape[0]) == 7
    models = evaluate.ModelPoints([np.zeros((0, 3), np.float32) if m is None else m["xyz"] for m in meshes], device)
    diameters = np.array([1.0, 0.2, 0.14], np.float32)
    ev = bop.BOPSceneEval(models, prepared, bop.SymmetrySets([None, None, None], device), diameters)
    m = ev.add_batch(depth, K, got["est_RT"], got["est_class"], got["est_frame"], got["est_score"], gt_RT, gt_class, gt_frame)
    valid = m["valid"].cpu().numpy()
    assert valid.all(), m["visib_fract"]                                 # every instance is visible
    assert (m["gt_est"]["mssd"][:, 0, -1] >= 0).all(), m["gt_est"]["mssd"][:, 0, -1]      # ... and matched at the loosest MSSD threshold
    assert (m["est_gt"]["mssd"][:, 0, -1] >= 0).all()                    # by an estimate each: no estimate is left over
    out = ev.cal_ar()
    assert out["n_targets"] == 7 and out["ar_mssd"] > 0.5


def test_sensor_to_pose_takes_max_instances(device, multi_frames):
    from ffb6d_amd import pipeline
    f = multi_frames
    frames = tuple(torch.from_numpy(f[k]).to(device) for k in ("pcld", "mask", "ctr_of", "kp_of"))
    net = torch.nn.Linear(1, 1).to(device)
    make = lambda **kw: pipeline.SensorToPose(net, np.eye(3), 2048, f["mesh_kps"], f["mesh_ctr"], r_lst=np.float32([0.1, 0.1]), pose_inputs=lambda i, o: frames, **kw)      # noqa: E731
    want = pose.solve_instances(*frames, f["mesh_kps"], f["mesh_ctr"], 4)
    got = make(max_instances=4).solve(None, None)
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    plain = make().solve(None, None)
    assert isinstance(plain, list) and len(plain) == 2 and plain[0][1].shape == (2, 3, 4)
    with pytest.raises(ValueError):
        make(max_instances=2, refine=dict())


def test_bad_arguments_raise(device):
    sets, counts = pack([ref.blobs(1, (20, 10))], 30, device)
    for K in (0, 256):
        with pytest.raises(_lib.FFB6DNativeError, match="max_clusters"):
            pose.mean_shift_multi(sets, counts, 0.04, K)
    with pytest.raises(_lib.FFB6DNativeError, match="min_inside"):
        pose.mean_shift_multi(sets, counts, 0.04, 2, min_inside=0)
    with pytest.raises(_lib.FFB6DNativeError, match="workspace"):
        pose.mean_shift_multi(sets, counts, 0.04, 2, workspace=torch.zeros(64, dtype=torch.uint8, device=device))
    with pytest.raises(ValueError):
        pose.MeanShiftTorch(0.04).fit_multi_clus(torch.zeros((0, 3), device=device))
    with pytest.raises(TypeError):
        pose.solve_instances(sets, counts, sets, sets, np.zeros((2, 1, 3)), np.zeros((2, 3)), 2, refine=None)
    assert pose.mean_shift_multi(sets, counts, 0.04, 255)[2][0, :3].tolist() == [20, 10, 0]


def test_cpu_tensors_are_rejected():
    sets, counts = torch.zeros(1, 30, 4), torch.tensor([30], dtype=torch.int32)
    with pytest.raises(_lib.FFB6DNativeError):
        pose.mean_shift_multi(sets, counts, 0.04, 2)
    with pytest.raises(_lib.FFB6DNativeError):
        pose.MeanShiftTorch(0.04).fit_multi_clus(torch.zeros(10, 3))
    with pytest.raises(_lib.FFB6DNativeError):
        pose.solve_instances(torch.zeros(1, 30, 3), torch.zeros(1, 30, dtype=torch.int64), torch.zeros(1, 1, 30, 3), torch.zeros(1, 8, 30, 3),
                             np.zeros((2, 8, 3)), np.zeros((2, 3)), 2)
