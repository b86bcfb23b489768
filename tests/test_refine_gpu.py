"""ICP refinement on the device (ffb6d_amd/refine.py, csrc/icp.hip) against the numpy restatement of tests/icp_ref.py: the
correspondences as bits, the two forms of the search as bits, the loop within the bar of the double Kabsch, and what the
feature is for -- a smaller ADD -- scored with evaluate.add_adds."""
import numpy as np
import pytest
import torch

import icp_ref
from ffb6d_amd import evaluate, pipeline, pose, refine, synth

pytestmark = pytest.mark.gpu

INF = float("inf")
# seeds chosen by running the restatement on the CPU (surface model 100 + seed with 2048 points, view 200 + seed,
# synth.eval_pose_pair(seed, "near")): none of them has a float32 / float64 rounding tie within 20 iterations at max_dist 0.01
# (seeds 2 and 11 have one, in iterations 11 and 6), and with max_dist 0.02 the restatement reduces the ADD of every REFINE seed by
# more than 35 x in 30 iterations (0: 37.9, 1: 51.8, 3: 126, 5: 110, 6: 122, 9: 106; seeds 4 and 10 reach only 19.6 and 19.5)
PARITY_SEEDS = (0, 1, 3, 4, 6, 7, 9, 10)
REFINE_SEEDS = (0, 1, 3, 5, 6, 9)


def _canon(x):
    x = np.array(x, np.float32)
    x[np.isnan(x)] = np.nan
    return x.view(np.uint32)


def _dev(device, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays]


def view_batch(seeds, n_model=2048, per_frame=2, N=4096):
    """Partial views of surface models, `per_frame` objects to a frame: class 1 + k = surface_model(100 + seed_k), class 0 is the
    background and the last class has no model points.  -> dict of numpy arrays + the model list."""
    models = [None] + [icp_ref.surface_model(100 + s, n_model) for s in seeds] + [None]
    B = (len(seeds) + per_frame - 1) // per_frame
    rng = np.random.RandomState(7)
    pcld = (rng.rand(B, N, 3) * [2.0, 1.2, 1.0] + [-1.0, -0.6, 0.6]).astype(np.float32)
    mask = np.zeros((B, N), np.int64)
    T0, gts, frame_of, class_of = [], [], [], []
    for k, s in enumerate(seeds):
        b, cls = k // per_frame, 1 + k
        pred, gt = synth.eval_pose_pair(s, "near")
        scene = icp_ref.partial_view(models[cls], gt, 200 + s)
        free = np.flatnonzero(mask[b] == 0)
        at = np.sort(rng.choice(free, len(scene), replace=False))
        pcld[b, at], mask[b, at] = scene[rng.permutation(len(scene))], cls
        T0.append(pred.astype(np.float64))
        gts.append(gt.astype(np.float64))
        frame_of.append(b)
        class_of.append(cls)
    return dict(pcld=pcld, mask=mask, T0=np.stack(T0), gt=np.stack(gts), frame_of=np.array(frame_of, np.int32),
                class_of=np.array(class_of, np.int32)), icp_ref.models_of(models)


def ragged_case(mask_dtype):
    """Classes of 700 / 2048 / 0 / 18 (a grid with two duplicated points) / 65 / 1 points; frame 0 holds classes 1 and 2, frame 1 the
    others and points labelled with the empty class; problems 5 and 7 have an empty scene set, problem 4 an empty class.  The scene
    points are model points under the problem's own pose + 2 mm of noise."""
    rng = np.random.RandomState(3)
    g = np.arange(4) / 64.0
    grid = np.array([[x, y, 0.0] for x in g for y in g] + [[g[0], g[3], 0.0], [g[2], g[2], 0.0]], np.float32)      # rows 16, 17 = rows 3, 10
    models = icp_ref.models_of([None, icp_ref.surface_model(1, 700), icp_ref.surface_model(2, 2048), None, grid,
                                icp_ref.surface_model(5, 65), icp_ref.surface_model(6, 1)])
    B, N = 2, 1536
    pcld = (rng.rand(B, N, 3) * [2.0, 1.2, 1.0] + [-1.0, -0.6, 0.6]).astype(np.float32)
    mask = np.zeros((B, N), np.int64)
    problems = [(0, 1), (0, 2), (1, 4), (1, 5), (1, 3), (0, 5), (1, 6), (1, 2)]
    T = np.zeros((len(problems), 3, 4))
    for p, (b, cls) in enumerate(problems):
        pred, gt = synth.eval_pose_pair(40 + p, "near")
        T[p] = pred
        if p in (5, 7) or cls == 3:
            continue
        n = {1: 300, 2: 500, 4: 0, 5: 130, 6: 2}[cls]                          # (one model point fixes no rotation: 2 pairs < min_pairs)
        m = models[cls]
        scene = (m[rng.randint(0, len(m), n)].astype(np.float64) @ pred[:, :3].T + pred[:, 3] + 0.002 * rng.randn(n, 3)).astype(np.float32)
        at = np.sort(rng.choice(np.flatnonzero(mask[b] == 0), n, replace=False))
        pcld[b, at], mask[b, at] = scene, cls
    # the grid under a pose whose arithmetic is exact: a point half way between rows 0 and 4, one on the duplicated rows 3 / 16,
    # one on rows 10 / 17, one far away
    T[2, :, :3], T[2, :, 3] = np.eye(3), [0.0, 0.0, 1.0]
    at = np.flatnonzero(mask[1] == 0)[:4]
    pcld[1, at] = [[1 / 128.0, 0.0, 1.0], [g[0], g[3], 1.0], [g[2], g[2], 1.0], [0.5, 0.5, 1.0]]
    mask[1, at] = 4
    at = np.flatnonzero(mask[1] == 0)[:50]
    mask[1, at] = 3                                                               # points of the class without a model
    keep = (rng.rand(B, N) < 0.7).astype(np.uint8)
    return dict(pcld=pcld, mask=mask.astype(mask_dtype), T=T, frame_of=np.array([b for b, _ in problems], np.int32),
                class_of=np.array([c for _, c in problems], np.int32), keep=keep), models


@pytest.fixture(scope="module")
def views(device):
    case, models = view_batch(PARITY_SEEDS)
    return case, models, refine.PreparedModels(evaluate.ModelPoints(models, device=device))


@pytest.fixture(autouse=True)
def default_form():
    yield
    refine.set_form(0)


# ---- 1. correspondences ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [-1, 0, 1])
@pytest.mark.parametrize("mask_dtype,with_keep", [(np.int64, False), (np.int32, False), (np.int64, True)])
def test_correspondences_equal_the_restatement_as_bits(device, mask_dtype, with_keep, form):
    case, models = ragged_case(mask_dtype)
    prepared = refine.PreparedModels(evaluate.ModelPoints(models, device=device))
    keep = case["keep"] if with_keep else None
    refine.set_form(form)
    pcld, mask = _dev(device, case["pcld"], case["mask"])
    for max_dist in (INF, 0.004):
        idx, d2, counts = refine.correspondences(pcld, mask, case["T"], case["frame_of"], case["class_of"], prepared, max_dist=max_dist,
                                                 keep=_dev(device, keep)[0] if with_keep else None)
        widx, wd2, wcounts = icp_ref.correspondences(case["pcld"], case["mask"], case["T"], case["frame_of"], case["class_of"], models,
                                                     max_dist, keep=keep)
        assert np.array_equal(counts.cpu().numpy(), wcounts)
        assert np.array_equal(idx.cpu().numpy(), widx)
        assert np.array_equal(_canon(d2.cpu().numpy()), _canon(wd2))
        assert wcounts[4] > 0 and wcounts[5] == 0 and (widx[4] == -1).all()      # the empty class has scene points; the empty scene set
        if not with_keep:
            assert list(widx[2, :4]) == ([0, 3, 10, 15] if max_dist == INF else [-1, 3, 10, -1])      # ties go to the lowest index


# ---- 2. the two forms ------------------------------------------------------------------------------------------------
def test_scan_and_pruned_forms_agree_as_bits(device, views):
    case, models, prepared = views
    pcld, mask = _dev(device, case["pcld"], case["mask"])
    got = {}
    for form in (0, 1):
        refine.set_form(form)
        idx, d2, _ = refine.correspondences(pcld, mask, case["T0"], case["frame_of"], case["class_of"], prepared, max_dist=0.01)
        T, st = refine.icp_refine(pcld, mask, case["T0"], case["frame_of"], case["class_of"], prepared, max_iter=10, max_dist=0.01)
        got[form] = [x.cpu().numpy() for x in (idx, d2, T, st["n_pairs"], st["rms"], st["iters"])]
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert (got[0][0] >= 0).sum() > 1000


def test_pruned_form_evaluates_a_fraction_of_the_pairs(device, views):
    case, models, prepared = views
    pcld, mask = _dev(device, case["pcld"], case["mask"])
    from ffb6d_amd import _lib
    lib = _lib.load()
    ctr = torch.zeros(1, dtype=torch.int64, device=device)
    pairs = {}
    try:
        for form in (0, 1):
            refine.set_form(form)
            ctr.zero_()
            _lib.check(lib.ffb6d_icp_set_pair_counter(ctr.data_ptr()), "ffb6d_icp_set_pair_counter")
            refine.correspondences(pcld, mask, case["T0"], case["frame_of"], case["class_of"], prepared, max_dist=0.01)
            pairs[form] = int(ctr.item())
    finally:
        lib.ffb6d_icp_set_pair_counter(None)
    n_scene = int((case["mask"] > 0).sum())
    assert pairs[0] == n_scene * 2048                                             # the scan form tests every model point
    print(f"pruned / scan pairs: {pairs[1]} / {pairs[0]} = {pairs[1] / pairs[0]:.4f}")
    assert 0 < pairs[1] < pairs[0]


# ---- 3. the loop -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 5, 20])
def test_loop_matches_the_restatement(device, views, iters):
    """Bar: max |T_dev - T_ref| <= 2e-5 (the bar of the double Kabsch, tests/test_pose_gpu.py:16-17), n_pairs equal, rms within
    1e-6 relative.  A case is excused only if the float32 and the float64 restatement themselves diverge (a rounding tie); the
    committed seeds have no such tie on the CPU (checked with icp_ref.first_divergence for all eight).  The largest difference on
    the MI355X has not been recorded yet (the test prints it per case); on the SIMT emulator's small cases it stays below 1e-12."""
    case, models, prepared = views
    pcld, mask = _dev(device, case["pcld"], case["mask"])
    T, st = refine.icp_refine(pcld, mask, case["T0"], case["frame_of"], case["class_of"], prepared, max_iter=iters, max_dist=0.01)
    wT, wst = icp_ref.icp_refine(case["pcld"], case["mask"], case["T0"], case["frame_of"], case["class_of"], models, iters, 0.01)
    T, n_pairs, rms, made = T.cpu().numpy(), st["n_pairs"].cpu().numpy(), st["rms"].cpu().numpy(), st["iters"].cpu().numpy()
    err = np.abs(T - wT).reshape(len(T), -1).max(axis=1)
    print(f"iters={iters}: max |T_dev - T_ref| per case {err}")
    excused = 0
    for p in range(len(T)):
        ok = err[p] <= 2e-5 and n_pairs[p] == wst["n_pairs"][p] and abs(rms[p] - wst["rms"][p]) <= 1e-6 * wst["rms"][p]
        if not ok:
            s = icp_ref.problem_scene(case["pcld"], case["mask"], int(case["frame_of"][p]), int(case["class_of"][p]))
            tie = icp_ref.first_divergence(s, models[case["class_of"][p]], case["T0"][p], iters, 0.01)
            assert tie is not None, (p, err[p], n_pairs[p], wst["n_pairs"][p], rms[p], wst["rms"][p])
            excused += 1
    assert excused <= len(T) // 10
    assert np.array_equal(made, wst["iters"]) and (made == iters).all()


# ---- 4. it refines ---------------------------------------------------------------------------------------------------
def test_refinement_reduces_add(device):
    case, models = view_batch(REFINE_SEEDS)
    mp = evaluate.ModelPoints(models, device=device)
    prepared = refine.PreparedModels(mp)
    pcld, mask = _dev(device, case["pcld"], case["mask"])
    T, _ = refine.icp_refine(pcld, mask, case["T0"], case["frame_of"], case["class_of"], prepared, max_iter=30, max_dist=0.02)
    wT, _ = icp_ref.icp_refine(case["pcld"], case["mask"], case["T0"], case["frame_of"], case["class_of"], models, 30, 0.02)
    score = lambda poses: evaluate.add_adds(poses, case["gt"], case["class_of"], mp)[0].cpu().numpy()       # noqa: E731
    before, after, ref_after = score(case["T0"]), score(T.cpu().numpy()), score(wT)
    print("ADD before", before, "after", after, "restatement", ref_after)
    assert (ref_after * 10 <= before).all()                                       # the cases are ones the restatement itself refines
    assert (after <= before).all() and (after <= 1.05 * ref_after).all()


# ---- 5. early stop, degenerate input -----------------------------------------------------------------------------------
def test_early_stop_matches_the_restatement(device, views):
    case, models, prepared = views
    pcld, mask = _dev(device, case["pcld"], case["mask"])
    T, st = refine.icp_refine(pcld, mask, case["T0"], case["frame_of"], case["class_of"], prepared, max_iter=30, max_dist=0.02, tol=1e-5)
    wT, wst = icp_ref.icp_refine(case["pcld"], case["mask"], case["T0"], case["frame_of"], case["class_of"], models, 30, 0.02, tol=1e-5)
    made = st["iters"].cpu().numpy()
    assert (wst["iters"] < 30).any()
    assert np.array_equal(made, wst["iters"]) and np.array_equal(st["n_pairs"].cpu().numpy(), wst["n_pairs"])
    assert np.abs(T.cpu().numpy() - wT).max() <= 2e-5


@pytest.mark.parametrize("form", [0, 1])
def test_degenerate_problems_return_their_input_pose(device, form):
    case, models = ragged_case(np.int64)
    prepared = refine.PreparedModels(evaluate.ModelPoints(models, device=device))
    refine.set_form(form)
    pcld = case["pcld"].copy()
    scene1 = np.flatnonzero(case["mask"][0] == 1)
    pcld[0, scene1[:25]] = np.nan                                                 # NaN scene points of problem 0
    pcld[0, scene1[25], 0] = np.inf
    dpcld, mask = _dev(device, pcld, case["mask"])
    for max_dist in (0.005, INF):
        if max_dist == INF:
            pcld[0, scene1[25], 0] = 0.3                                          # (an infinite point within an infinite gate: not a case)
            dpcld = _dev(device, pcld)[0]
        T, st = refine.icp_refine(dpcld, mask, case["T"], case["frame_of"], case["class_of"], prepared, max_iter=6, max_dist=max_dist)
        wT, wst = icp_ref.icp_refine(pcld, case["mask"], case["T"], case["frame_of"], case["class_of"], models, 6, max_dist)
        T, n_pairs, made = T.cpu().numpy(), st["n_pairs"].cpu().numpy(), st["iters"].cpu().numpy()
        assert np.isfinite(T).all()
        assert np.array_equal(n_pairs, wst["n_pairs"]) and np.array_equal(made, wst["iters"])
        assert n_pairs[0] >= 50 and made[0] == 6                                  # the NaN points are gated out, the others pair up
        for p in (4, 5, 7):                                                       # empty class; empty scene sets
            assert made[p] == 0 and n_pairs[p] == 0 and np.array_equal(T[p].view(np.uint64), case["T"][p].view(np.uint64))
        if max_dist == 0.005:                                                     # the grid: 2 kept pairs < min_pairs
            assert made[2] == 0 and n_pairs[2] == 2 and np.array_equal(T[2].view(np.uint64), case["T"][2].view(np.uint64))
        assert made[6] == 0 and n_pairs[6] <= 2
        for p in (0, 1, 3):                                                       # (the grid is all ties: its bits are pinned by test 1)
            assert np.abs(T[p] - wT[p]).max() <= 2e-5, (p, max_dist)
    # device ids that are no index: problems without pairs, nothing is read out of bounds
    bad_f, bad_c = _dev(device, np.array([0, 9, -1, 0], np.int32), np.array([1, 1, 2, 99], np.int32))
    T, st = refine.icp_refine(dpcld, mask, case["T"][:4], bad_f, bad_c, prepared, max_iter=3, max_dist=0.01)
    assert list(st["iters"].cpu().numpy()) == [3, 0, 0, 0]
    assert np.array_equal(T.cpu().numpy()[1:].view(np.uint64), case["T"][1:4].view(np.uint64))
    with pytest.raises(ValueError):
        refine.icp_refine(dpcld, mask, case["T"][:1], [0], [99], prepared)


# ---- 6. the pipeline ---------------------------------------------------------------------------------------------------
def _pose_batch(device, B=2, N=2048, n_cls=6):
    cases = [synth.make_pose_case(50 + b, n_pts=N, n_obj=3, n_cls=n_cls, mesh_seed=4) for b in range(B)]
    stack = lambda k: torch.from_numpy(np.stack([c[k] for c in cases])).to(device)       # noqa: E731
    rng = np.random.RandomState(9)
    balls = []
    for _ in range(n_cls):
        v = rng.randn(1500, 3)
        balls.append((v / np.linalg.norm(v, axis=1, keepdims=True) * 0.07 * rng.rand(1500, 1) ** (1 / 3)).astype(np.float32))
    prepared = refine.PreparedModels(evaluate.ModelPoints([None] + balls[1:], device=device))
    return cases, (stack("pcld"), stack("mask"), stack("ctr_of"), stack("kp_of")), prepared


def _same(a, b):
    assert len(a) == len(b)
    for (ia, pa, ka), (ib, pb, kb) in zip(a, b):
        assert np.array_equal(ia, ib) and np.array_equal(pa.view(np.uint64), pb.view(np.uint64)) and np.array_equal(ka, kb)


def test_solve_poses_with_refine_equals_the_two_separate_calls(device):
    cases, fixed, prepared = _pose_batch(device)
    kw = dict(r_lst=cases[0]["r_lst"])
    plain = pose.solve_poses(*fixed, cases[0]["mesh_kps"], cases[0]["mesh_ctr"], **kw)
    _same(plain, pose.solve_poses(*fixed, cases[0]["mesh_kps"], cases[0]["mesh_ctr"], refine=None, **kw))
    stats = {}
    fused = pose.solve_poses(*fixed, cases[0]["mesh_kps"], cases[0]["mesh_ctr"], stats=stats,
                             refine=dict(models=prepared, max_iter=8, max_dist=0.03), **kw)
    frame_of = np.concatenate([np.full(len(ids), b, np.int32) for b, (ids, _, _) in enumerate(plain)])
    class_of = np.concatenate([ids for ids, _, _ in plain]).astype(np.int32)
    T, st = refine.icp_refine(fixed[0], fixed[1], np.concatenate([p for _, p, _ in plain]), frame_of, class_of, prepared, max_iter=8,
                              max_dist=0.03)
    T = T.cpu().numpy()
    at = 0
    for (ids, poses, kps), (pids, _, pkps) in zip(fused, plain):
        assert np.array_equal(ids, pids) and np.array_equal(kps, pkps)            # the keypoints stay as fitted
        assert np.array_equal(poses.view(np.uint64), T[at:at + len(ids)].view(np.uint64))
        at += len(ids)
    assert at == len(T) > 0 and (stats["refine"]["iters"].cpu().numpy() == 8).all()
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(fused, plain))      # the refinement moved something


def test_pipeline_with_refine_serial_equals_overlapped(device):
    from test_forward_gpu import build
    from test_pipeline_gpu import _sensor
    B, N, H, W, n_cls = 2, 2048, 240, 320, 6
    net = build(n_cls, N, device)
    net.two_streams = True
    cases, fixed, prepared = _pose_batch(device, B, N, n_cls)
    batches = [_sensor(c, B, N, H, W, device) for c in (2, 3, 4)]
    mk = lambda r: pipeline.SensorToPose(net, synth.LINEMOD_K, N, cases[0]["mesh_kps"], cases[0]["mesh_ctr"], r_lst=cases[0]["r_lst"],       # noqa: E731
                                         seed=11, pose_inputs=lambda inp, out: fixed, refine=r)
    pipe = mk(dict(models=prepared, max_iter=8, max_dist=0.03))
    pipe.run(batches[:1], overlap=False)
    serial = pipe.run(batches, overlap=False)
    over = pipe.run(batches, overlap=True)
    torch.cuda.synchronize()
    want = pose.solve_poses(*fixed, cases[0]["mesh_kps"], cases[0]["mesh_ctr"], r_lst=cases[0]["r_lst"],
                            refine=dict(models=prepared, max_iter=8, max_dist=0.03))
    for s, o in zip(serial, over):
        _same(s, o)
        _same(s, want)
    plain = mk(None).run(batches[:1], overlap=False)
    _same(plain[0], pose.solve_poses(*fixed, cases[0]["mesh_kps"], cases[0]["mesh_ctr"], r_lst=cases[0]["r_lst"]))


# ---- 7. no synchronisation ---------------------------------------------------------------------------------------------
def test_icp_refine_does_not_wait_for_the_stream(device, views):
    case, models, prepared = views
    pcld, mask, T0, frame_of, class_of = _dev(device, case["pcld"], case["mask"], case["T0"], case["frame_of"], case["class_of"])
    refine.icp_refine(pcld, mask, T0, frame_of, class_of, prepared, max_iter=10, max_dist=0.01)      # (allocations cached)
    a = torch.randn(8192, 8192, device=device)
    torch.cuda.synchronize()
    for _ in range(40):
        a @ a                                                                     # some hundred milliseconds of queued work
    T, st = refine.icp_refine(pcld, mask, T0, frame_of, class_of, prepared, max_iter=10, max_dist=0.01)
    idx, _, _ = refine.correspondences(pcld, mask, T0, frame_of, class_of, prepared, max_dist=0.01)
    assert not torch.cuda.current_stream().query()                                # the calls returned with the stream still busy
    torch.cuda.synchronize()
    assert (st["iters"].cpu().numpy() == 10).all()
