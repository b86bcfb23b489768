"""Instance-aware ICP on the device (refine.correspondences_instances / icp_refine_instances, pose.solve_instances_refined,
pipeline.SensorToPose(instance_refine=)) against the numpy restatement of tests/icp_inst_ref.py: the single step as bits in both
modes, all forms of the search, both mask widths, with and without keep; the loop within the bar of the class form's test; the
anchors to the class calls as bits; the solver and the pipeline; and what the feature is for."""
import numpy as np
import pytest
import torch

import icp_inst_ref as iref
from ffb6d_amd import _lib, evaluate, pipeline, pose, refine, synth

pytestmark = pytest.mark.gpu

INF = float("inf")
# Seeds of iref.instance_views, chosen by running the restatement ALONE on the CPU (1024-point models, N = 4096):
#   LOOP_SEEDS  neither mode has a float32 / float64 rounding tie within 20 iterations at max_dist 0.01
#   HELP_SEEDS  with max_dist 0.02 and 30 iterations the restatement lowers the ADD of both instances in both modes, keeps at least as
#               many pairs per instance in nearest mode as in map mode, and its refined map gives more of the instance-0 points to
#               the instance they were drawn from than to the other
LOOP_SEEDS = (0, 1, 3)
HELP_SEEDS = (0, 1, 3)


def _canon(x):
    x = np.array(x, np.float32)
    x[np.isnan(x)] = np.nan
    return x.view(np.uint32)


def _dev(device, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays]


def _args(case, T="T"):
    return case["pcld"], case["mask"], case["inst"], case[T], case["frame_of"], case["class_of"], case["inst_of"]


@pytest.fixture(autouse=True)
def default_form():
    yield
    refine.set_form(0)


@pytest.fixture(scope="module")
def tiny(device):
    """the tiny ragged case at both sizes and mask widths, its models prepared once"""
    out = {}
    for N, dt in ((192, np.int64), (300, np.int32)):
        case, models = iref.instances_case(N, dt)
        out[N] = case, models, refine.PreparedModels(evaluate.ModelPoints(models, device=device))
    return out


@pytest.fixture(scope="module")
def views(device):
    case, models = iref.instance_views(LOOP_SEEDS)
    return case, models, refine.PreparedModels(evaluate.ModelPoints(models, device=device))


# ---- 1, 2. the single step as bits; the forms agree ----------------------------------------------------------------------
@pytest.mark.parametrize("N", [192, 300])
@pytest.mark.parametrize("mode", ["map", "nearest"])
def test_single_step_equals_the_restatement_as_bits(device, tiny, N, mode):
    case, models, prepared = tiny[N]
    pcld, mask, inst, keep = _dev(device, case["pcld"], case["mask"], case["inst"], case["keep"])
    ids = _dev(device, case["frame_of"], case["class_of"], case["inst_of"])      # device ids: a frame that is no index is not refused
    got = {}
    for max_dist, kp in ((INF, None), (0.006, None), (0.006, case["keep"])):
        want = iref.correspondences_instances(*_args(case), models, max_dist, mode, kp)
        for form in (-1, 0, 1):
            refine.set_form(form)
            idx, d2, counts, owner = (x.cpu().numpy() for x in refine.correspondences_instances(
                pcld, mask, inst, case["T"], *ids, prepared, mode=mode, max_dist=max_dist, keep=keep if kp is not None else None))
            assert np.array_equal(counts, want[2]) and np.array_equal(idx, want[0]), (form, max_dist)
            assert np.array_equal(_canon(d2), _canon(want[1])) and np.array_equal(owner, want[3]), (form, max_dist)
            got[form] = (idx, _canon(d2), owner)
        for form in (-1, 1):                                                      # scan, pruned, automatic: the same bits
            assert all(np.array_equal(a, b) for a, b in zip(got[form], got[0]))
    widx, _, wcounts, wowner = iref.correspondences_instances(*_args(case), models, INF, mode)
    if mode == "map":
        assert list(wcounts) == [64, 65, 7, 30, 25, 40, 65, 0, 5, 0, 0, 0, 8] and (wowner[0, :3] == -1).all()
    else:
        assert list(wcounts) == [151, 151, 151, 61, 61, 45, 151, 151, 151, 61, 61, 0, 10]
        assert set(np.unique(wowner[0, :151])) == {-1, 0, 1, 2} and np.array_equal(wowner[0], wowner[2])


def test_an_exact_tie_between_siblings_goes_to_the_lower_row(device, tiny):
    case, models, prepared = tiny[192]
    pcld, mask = _dev(device, case["pcld"], case["mask"])
    T = np.stack([case["T"][0], case["T"][0], case["T"][2]])
    for form in (0, 1):
        refine.set_form(form)
        idx, d2, _, owner = (x.cpu().numpy() for x in refine.correspondences_instances(
            pcld, mask, None, T, case["frame_of"][:3], case["class_of"][:3], case["inst_of"][:3], prepared, mode="nearest"))
        assert np.array_equal(_canon(d2[0]), _canon(d2[1]))
        assert (owner[:, :151] != 1).all() and (owner[0, :151] == 0).sum() > 60 and (idx[1] == -1).all()
        widx, _, _, wowner = iref.correspondences_instances(case["pcld"], case["mask"], None, T, case["frame_of"][:3], case["class_of"][:3],
                                                               case["inst_of"][:3], models, INF, "nearest")
        assert np.array_equal(idx, widx) and np.array_equal(owner, wowner)


# ---- 3. the loop -----------------------------------------------------------------------------------------------------
def _judge(T, st, wT, wst, tie):
    """The bar of tests/test_refine_gpu.py::test_loop_matches_the_restatement: max |T_dev - T_ref| <= 2e-5, n_pairs equal, rms within
    1e-6 relative; a problem is excused only if the float32 and the float64 restatement themselves diverge (a rounding tie), in
    nearest mode anywhere in its group.  -> the excused problems"""
    err = np.abs(T - wT).reshape(len(T), -1).max(axis=1)
    print("max |T_dev - T_ref| per problem", err)
    excused = []
    for p in range(len(T)):
        ok = err[p] <= 2e-5 and st["n_pairs"][p] == wst["n_pairs"][p] and abs(st["rms"][p] - wst["rms"][p]) <= 1e-6 * wst["rms"][p]
        if not ok:
            assert tie()[p] is not None, (p, err[p], st["n_pairs"][p], wst["n_pairs"][p], st["rms"][p], wst["rms"][p])
            excused.append(p)
    assert len(excused) <= len(T) // 10
    return excused


@pytest.mark.parametrize("iters", [1, 5, 20])
@pytest.mark.parametrize("mode", ["map", "nearest"])
def test_loop_matches_the_restatement(device, views, mode, iters):
    case, models, prepared = views
    pcld, mask, inst = _dev(device, case["pcld"], case["mask"], case["inst"])
    T, st = refine.icp_refine_instances(pcld, mask, inst, case["T0"], case["frame_of"], case["class_of"], case["inst_of"], prepared, mode=mode,
                                        max_iter=iters, max_dist=0.01)
    wT, wst = iref.icp_refine_instances(*_args(case, "T0"), models, iters, 0.01, mode)
    T, st = T.cpu().numpy(), {k: v.cpu().numpy() for k, v in st.items()}
    excused = _judge(T, st, wT, wst, lambda: iref.first_divergence_instances(*_args(case, "T0"), models, iters, 0.01, mode))
    assert np.array_equal(st["iters"], wst["iters"]) and (st["iters"] == iters).all()
    if not excused:                                                               # the maps agree wherever the loops have not diverged
        assert (wst["writers"] <= 1).all() and np.array_equal(st["inst"], wst["inst"])
    assert (wst["inst"] > 0).sum() > 500 and (wst["inst"][case["mask"] == 0] == 0).all()


@pytest.mark.parametrize("mode", ["map", "nearest"])
def test_loop_on_the_tiny_case(device, tiny, mode):
    """every kind of problem at once, with and without keep, in the scan and the pruned form: the bar of the loop test, the forms as bits"""
    case, models, prepared = tiny[300]
    pcld, mask, inst, keep = _dev(device, case["pcld"], case["mask"], case["inst"], case["keep"])
    ids = _dev(device, case["frame_of"], case["class_of"], case["inst_of"])
    for kp in (None, case["keep"]):
        got = {}
        wT, wst = iref.icp_refine_instances(*_args(case), models, 6, 0.012, mode, keep=kp)
        for form in (0, 1):
            refine.set_form(form)
            T, st = refine.icp_refine_instances(pcld, mask, inst, case["T"], *ids, prepared, mode=mode, max_iter=6, max_dist=0.012,
                                                keep=keep if kp is not None else None)
            got[form] = T.cpu().numpy(), {k: v.cpu().numpy() for k, v in st.items()}
        T, st = got[0]
        decided = wst["writers"] <= 1                                             # (rows 0-2 and 6-8 are separate groups of one pair: a point both keep carries either id)
        assert np.array_equal(T.view(np.uint64), got[1][0].view(np.uint64)) and np.array_equal(st["inst"][decided], got[1][1]["inst"][decided])
        assert all(np.array_equal(st[k].view(np.uint8), got[1][1][k].view(np.uint8)) for k in ("n_pairs", "rms", "iters"))
        err = np.abs(T - wT).reshape(len(T), -1).max(axis=1)
        tie = None
        for p in range(len(T)):
            if not (err[p] <= 2e-5 and st["n_pairs"][p] == wst["n_pairs"][p] and abs(st["rms"][p] - wst["rms"][p]) <= 1e-6 * wst["rms"][p]
                    and st["iters"][p] == wst["iters"][p]):
                tie = tie or iref.first_divergence_instances(*_args(case), models, 6, 0.012, mode, keep=kp)
                assert tie[p] is not None, (p, err[p], st["n_pairs"][p], wst["n_pairs"][p])
        if tie is None:
            assert np.array_equal(st["inst"][decided], wst["inst"][decided]) and (wst["inst"] > 0).sum() > 80


# ---- 4. early stop ---------------------------------------------------------------------------------------------------------
def test_a_stopped_sibling_goes_on_competing(device, views):
    """tol > 0 in nearest mode: the first instance of every class starts at the pose the restatement converges to, so it stops in its
    first iterations while its sibling goes on; iters per problem as the restatement's."""
    case, models, prepared = views
    settled, _ = iref.icp_refine_instances(*_args(case, "T0"), models, 30, 0.02, "nearest")
    T0 = case["T0"].copy()
    T0[0::2] = settled[0::2]
    pcld, mask = _dev(device, case["pcld"], case["mask"])
    T, st = refine.icp_refine_instances(pcld, mask, None, T0, case["frame_of"], case["class_of"], case["inst_of"], prepared, mode="nearest",
                                        max_iter=12, max_dist=0.02, tol=1e-4)
    wT, wst = iref.icp_refine_instances(case["pcld"], case["mask"], None, T0, case["frame_of"], case["class_of"], case["inst_of"], models, 12,
                                           0.02, "nearest", tol=1e-4)
    made = st["iters"].cpu().numpy()
    print("iters", made, "restatement", wst["iters"])
    assert (wst["iters"][0::2] < wst["iters"][1::2]).all() and (wst["iters"][0::2] < 12).all()      # the case is what it says
    assert np.array_equal(made, wst["iters"]) and np.array_equal(st["n_pairs"].cpu().numpy(), wst["n_pairs"])
    assert np.abs(T.cpu().numpy() - wT).max() <= 2e-5
    assert np.array_equal(st["inst"].cpu().numpy(), wst["inst"])


# ---- 5. anchors to the class calls -------------------------------------------------------------------------------------------
def test_anchors_to_icp_refine_as_bits(device, views, tiny):
    case, models, prepared = views
    pcld, mask, inst = _dev(device, case["pcld"], case["mask"], case["inst"])
    alone = np.arange(0, len(case["frame_of"]), 2)                               # one instance of every class: singleton groups
    f, c, T0 = case["frame_of"][alone], case["class_of"][alone], case["T0"][alone]
    for kw in (dict(max_iter=10, max_dist=0.01), dict(max_iter=30, max_dist=0.02, tol=1e-5)):
        T, st = refine.icp_refine(pcld, mask, T0, f, c, prepared, **kw)
        ones = (mask > 0).to(torch.uint8)
        runs = [refine.icp_refine_instances(pcld, mask, ones, T0, f, c, np.ones(len(alone), np.int32), prepared, mode="map", **kw),
                refine.icp_refine_instances(pcld, mask, inst, T0, f, c, case["inst_of"][alone], prepared, mode="nearest", **kw),
                refine.icp_refine_instances(pcld, mask, None, T0, f, c, case["inst_of"][alone], prepared, mode="nearest", **kw)]
        for gT, gst in runs:
            assert torch.equal(gT, T) and all(torch.equal(gst[k], st[k]) for k in st)
        assert torch.equal(runs[1][1]["inst"], runs[2][1]["inst"]) and int((runs[0][1]["inst"] > 0).sum()) > 500
    # nearest mode never reads the map: groups of several, any map or none
    a = refine.icp_refine_instances(pcld, mask, inst, case["T0"], case["frame_of"], case["class_of"], case["inst_of"], prepared, mode="nearest", max_iter=5)
    b = refine.icp_refine_instances(pcld, mask, None, case["T0"], case["frame_of"], case["class_of"], case["inst_of"], prepared, mode="nearest", max_iter=5)
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


# ---- 6. degenerate problems ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("mode", ["map", "nearest"])
def test_degenerate_problems_return_their_input_pose(device, tiny, mode, form):
    case, models, prepared = tiny[192]
    refine.set_form(form)
    pcld, mask, inst = _dev(device, case["pcld"], case["mask"], case["inst"])
    T, st = refine.icp_refine_instances(pcld, mask, inst, case["T"], *_dev(device, case["frame_of"], case["class_of"], case["inst_of"]), prepared,
                                        mode=mode, max_iter=6, max_dist=0.012)
    T, n_pairs, made, out = T.cpu().numpy(), st["n_pairs"].cpu().numpy(), st["iters"].cpu().numpy(), st["inst"].cpu().numpy()
    assert np.isfinite(T).all() and made[0] == 6 and made[3] == 6                 # the NaN points are gated out, the others pair up
    # map: an instance no point carries, ids 0 and 256; both: a frame that is no index, a class without a model
    for p in (7, 9, 10, 11, 12) if mode == "map" else (11, 12):
        assert made[p] == 0 and n_pairs[p] == 0 and np.array_equal(T[p].view(np.uint64), case["T"][p].view(np.uint64)), p
    assert (out[case["mask"] == 3] == 0).all() and (out[case["mask"] == 0] == 0).all()
    assert (out[0, np.isnan(case["pcld"][0]).any(axis=1)] == 0).all()
    if mode == "map":
        assert set(np.unique(out)) <= {0, 1, 2, 3, 255} and ((out == 0) | (out == case["inst"])).all()
    host = case["T"][:3], case["frame_of"][:3], case["class_of"][:3], case["inst_of"][:3]
    with pytest.raises(ValueError):
        refine.icp_refine_instances(pcld, mask, None, *host, prepared, mode="map")
    with pytest.raises(ValueError):
        refine.icp_refine_instances(pcld, mask, inst, *host, prepared, mode="votes")
    with pytest.raises(ValueError):                                               # host-visible ids are checked, as in icp_refine
        refine.icp_refine_instances(pcld, mask, inst, case["T"], case["frame_of"], case["class_of"], case["inst_of"], prepared)


# ---- 7. the solver -------------------------------------------------------------------------------------------------------------
def _multi(device):
    import pose_instances_ref as ref
    f = ref.make_multi_instance_frames(31)
    frames = tuple(torch.from_numpy(f[k]).to(device) for k in ("pcld", "mask", "ctr_of", "kp_of"))
    rng = np.random.RandomState(9)
    balls = []
    for _ in range(f["mesh_kps"].shape[0]):
        v = rng.randn(1200, 3)
        balls.append((v / np.linalg.norm(v, axis=1, keepdims=True) * 0.07 * rng.rand(1200, 1) ** (1 / 3)).astype(np.float32))
    prepared = refine.PreparedModels(evaluate.ModelPoints([None] + balls[1:], device=device))
    return f, frames, prepared


def test_solver_without_refine_and_with_it(device):
    f, frames, prepared = _multi(device)
    plain = pose.solve_instances(*frames, f["mesh_kps"], f["mesh_ctr"], 4, min_fraction=0.05)
    same = pose.solve_instances_refined(*frames, f["mesh_kps"], f["mesh_ctr"], 4, refine=None, min_fraction=0.05)
    assert all(torch.equal(same[k], plain[k]) for k in plain) and torch.equal(same["est_RT_fit"], plain["est_RT"])
    assert set(same) == set(plain) | {"est_RT_fit", "icp_pairs", "icp_rms", "icp_iters", "inst"}
    assert same["inst"].dtype == torch.uint8 and same["inst"].shape == frames[1].shape and int(same["inst"].max()) >= 3
    for mode in ("nearest", "map"):
        opts = dict(models=prepared, mode=mode, max_iter=8, max_dist=0.03)
        got = pose.solve_instances_refined(*frames, f["mesh_kps"], f["mesh_ctr"], 4, refine=opts, min_fraction=0.05)
        T, st = refine.icp_refine_instances(frames[0], frames[1], same["inst"], plain["est_RT"], plain["est_frame"], plain["est_class"],
                                            plain["est_instance"], prepared, mode=mode, max_iter=8, max_dist=0.03)
        assert torch.equal(got["est_RT"], T) and torch.equal(got["est_RT_fit"], plain["est_RT"]) and torch.equal(got["inst"], st["inst"])
        assert torch.equal(got["icp_pairs"], st["n_pairs"]) and torch.equal(got["icp_rms"], st["rms"]) and torch.equal(got["icp_iters"], st["iters"])
        assert all(torch.equal(got[k], plain[k]) for k in plain if k != "est_RT")                  # est_score stays the vote share
        assert not torch.equal(got["est_RT"], plain["est_RT"]) and (got["icp_iters"] > 0).all()
        if mode == "nearest":                                                     # the default mode
            d = pose.solve_instances_refined(*frames, f["mesh_kps"], f["mesh_ctr"], 4, min_fraction=0.05,
                                             refine=dict(models=prepared, max_iter=8, max_dist=0.03))
            assert torch.equal(d["est_RT"], got["est_RT"])


@pytest.mark.parametrize("classes", [None, [1, 2, 3, 4]], ids=["present", "listed"])
def test_one_instance_per_class_equals_solve_poses_as_bits(device, classes):
    """the fixtures of tests/test_pose_instances_gpu.py's K = 1 equality"""
    cases = [synth.make_pose_case(700 + k, n_pts=1500, n_obj=3, n_cls=5, mesh_seed=7) for k in range(3)]
    cases[1]["mask"][:] = 0
    cases[2]["mask"][cases[2]["mask"] == 2] = 0
    frames = tuple(torch.from_numpy(np.stack([c[key] for c in cases])).to(device) for key in ("pcld", "mask", "ctr_of", "kp_of"))
    mesh_kps, mesh_ctr, r_lst = cases[0]["mesh_kps"], cases[0]["mesh_ctr"], cases[0]["r_lst"]
    rng = np.random.RandomState(4)
    clouds = [None] + [(0.05 * rng.randn(600, 3)).astype(np.float32) for _ in range(4)]
    prepared = refine.PreparedModels(evaluate.ModelPoints(clouds, device=device))
    icp = dict(models=prepared, max_iter=6, max_dist=0.03)

    def compare(want, got):
        rows = {(int(fr), int(c)): e for e, (fr, c) in enumerate(zip(got["est_frame"].tolist(), got["est_class"].tolist()))}
        n = 0
        for b, (ids, poses, kps) in enumerate(want):
            for c, T, k in zip(ids, poses, kps):
                if (b, int(c)) not in rows:
                    assert np.array_equal(T, np.identity(4)[:3])                  # solve_poses: the identity; here: no row
                    continue
                e, n = rows[(b, int(c))], n + 1
                assert np.array_equal(got["est_RT"][e].cpu().numpy().view(np.uint64), T.view(np.uint64)), (b, c)
                assert np.array_equal(got["kps"][e].cpu().numpy(), k), (b, c)
        assert n == len(rows) >= 5

    want = pose.solve_poses(*frames, mesh_kps, mesh_ctr, use_ctr_clus_flter=True, refine_mask=False, classes=classes, refine=icp)
    got = pose.solve_instances_refined(*frames, mesh_kps, mesh_ctr, 1, min_inside=1, classes=classes, refine=dict(icp, mode="nearest"))
    compare(want, got)
    assert int(got["icp_iters"].max()) == 6
    want = pose.solve_poses(*frames, mesh_kps, mesh_ctr, r_lst=r_lst, use_ctr_clus_flter=True, refine_mask=True, classes=classes)
    got = pose.solve_instances_refined(*frames, mesh_kps, mesh_ctr, 1, min_inside=1, classes=classes, refine_mask=True, r_lst=r_lst)
    compare(want, got)
    with pytest.raises(ValueError):
        pose.solve_instances_refined(*frames, mesh_kps, mesh_ctr, 1, refine_mask=True)


# ---- 8. it helps ---------------------------------------------------------------------------------------------------------------
def test_refinement_helps_on_touching_instances(device):
    """Two instances of a class 1.5 model radii apart, 40 % of each instance's points with instance 0 in the map (HELP_SEEDS: the
    restatement alone meets the three conditions below on the CPU)."""
    case, models = iref.instance_views(HELP_SEEDS)
    mp = evaluate.ModelPoints(models, device=device)
    prepared = refine.PreparedModels(mp)
    pcld, mask, inst = _dev(device, case["pcld"], case["mask"], case["inst"])
    score = lambda poses: evaluate.add_adds(poses, case["gt"], case["class_of"], mp)[0].cpu().numpy()       # noqa: E731
    before, pairs = score(case["T0"]), {}
    for mode in ("map", "nearest"):
        T, st = refine.icp_refine_instances(pcld, mask, inst, case["T0"], case["frame_of"], case["class_of"], case["inst_of"], prepared, mode=mode,
                                            max_iter=30, max_dist=0.02)
        after, pairs[mode] = score(T.cpu().numpy()), st["n_pairs"].cpu().numpy()
        print(mode, "ADD before", before, "after", after, "pairs", pairs[mode])
        assert (after <= before).all()
    assert (pairs["nearest"] >= pairs["map"]).all()
    out = st["inst"].cpu().numpy()
    free = (case["truth"] > 0) & (case["inst"] == 0)
    for b, cls in zip(case["frame_of"][::2], case["class_of"][::2]):
        sel = free[b] & (case["mask"][b] == cls)
        right, wrong = int((out[b][sel] == case["truth"][b][sel]).sum()), int(((out[b][sel] > 0) & (out[b][sel] != case["truth"][b][sel])).sum())
        print("class", cls, "instance-0 points given to their instance", right, "to the other", wrong, "of", int(sel.sum()))
        assert right >= wrong and right > 0


# ---- 9. the pipeline -----------------------------------------------------------------------------------------------------------
def test_pipeline_with_instance_refine(device):
    from test_forward_gpu import build
    from test_pipeline_gpu import _sensor
    f, frames, prepared = _multi(device)
    B, N = frames[1].shape
    H, W, n_cls = 240, 320, 6
    net = build(n_cls, N, device)
    net.two_streams = True
    batches = [_sensor(c, B, N, H, W, device) for c in (2, 3, 4)]
    opts = dict(models=prepared, mode="nearest", max_iter=8, max_dist=0.03)
    mk = lambda **kw: pipeline.SensorToPose(net, synth.LINEMOD_K, N, f["mesh_kps"], f["mesh_ctr"], seed=11, pose_inputs=lambda inp, out: frames, **kw)       # noqa: E731
    pipe = mk(max_instances=4, instance_refine=opts)
    pipe.run(batches[:1], overlap=False)
    serial = pipe.run(batches, overlap=False)
    over = pipe.run(batches, overlap=True)
    torch.cuda.synchronize()
    want = pose.solve_instances_refined(*frames, f["mesh_kps"], f["mesh_ctr"], 4, refine=opts)
    for s, o in zip(serial, over):
        assert set(s) == set(o) == set(want)
        assert all(torch.equal(s[k], o[k]) and torch.equal(s[k], want[k]) for k in want)
    assert int(want["est_RT"].shape[0]) >= 7 and (want["icp_iters"] > 0).any()
    with pytest.raises(ValueError):
        mk(instance_refine=opts)
    with pytest.raises(ValueError):
        mk(max_instances=2, refine=dict())


# ---- 10. no synchronisation ----------------------------------------------------------------------------------------------------
def test_icp_refine_instances_does_not_wait_for_the_stream(device, views):
    case, models, prepared = views
    pcld, mask, inst, T0, frame_of, class_of, inst_of = _dev(device, *_args(case, "T0"))
    for mode in ("map", "nearest"):
        refine.icp_refine_instances(pcld, mask, inst, T0, frame_of, class_of, inst_of, prepared, mode=mode, max_iter=10, max_dist=0.01)      # (allocations cached)
    a = torch.randn(8192, 8192, device=device)
    torch.cuda.synchronize()
    for _ in range(40):
        a @ a                                                                     # some hundred milliseconds of queued work
    runs = [refine.icp_refine_instances(pcld, mask, inst, T0, frame_of, class_of, inst_of, prepared, mode=mode, max_iter=10, max_dist=0.01)
            for mode in ("map", "nearest")]
    refine.correspondences_instances(pcld, mask, inst, T0, frame_of, class_of, inst_of, prepared, mode="nearest", max_dist=0.01)
    assert not torch.cuda.current_stream().query()                                # the calls returned with the stream still busy
    torch.cuda.synchronize()
    assert all((st["iters"].cpu().numpy() == 10).all() for _, st in runs)


# ---- 11. workspace and argument errors -------------------------------------------------------------------------------------------
def test_workspace_and_argument_errors(device, tiny):
    case, models, prepared = tiny[192]
    lib = _lib.load()
    pcld, mask, inst, T0, frame_of, class_of, inst_of = _dev(device, *_args(case))
    P, (B, N) = len(case["frame_of"]), case["mask"].shape
    wbytes = lib.ffb6d_icp_inst_workspace_bytes(P, N, 1)
    assert wbytes > lib.ffb6d_icp_workspace_bytes(P, N) and lib.ffb6d_icp_inst_workspace_bytes(P, N, 2) == 0
    ws = torch.zeros(wbytes, dtype=torch.uint8, device=device)
    T = torch.full((P, 3, 4), 7.0, dtype=torch.float64, device=device)
    out = torch.full((B, N), 7, dtype=torch.uint8, device=device)

    def call(P=P, mode=0, inst=inst, wbytes=wbytes):
        return lib.ffb6d_icp_refine_inst_f32(prepared.buf.data_ptr(), prepared.n_cls, prepared.total, pcld.data_ptr(), mask.data_ptr(), 64, None,
                                             inst.data_ptr() if inst is not None else None, frame_of.data_ptr(), class_of.data_ptr(),
                                             inst_of.data_ptr(), T0.data_ptr(), P, B, N, N, 0.01, 3, 0.0, 3, mode, T.data_ptr(), None, None,
                                             None, out.data_ptr(), ws.data_ptr(), wbytes, None)
    for kw, text in ((dict(mode=2), "mode must be 0 (map) or 1 (nearest)"), (dict(inst=None), "needs the instance map"), (dict(P=65536), "at most 65535")):
        assert call(**kw) == -1 and text in _lib.last_error(), kw
    assert call(wbytes=wbytes - 1) == -3 and "workspace" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((T == 7.0).all()) and bool((out == 7).all())                      # nothing was launched
    assert call(mode=1, inst=None) == 0
    torch.cuda.synchronize()
    assert bool((T != 7.0).all()) and int(out.max()) <= 255 and bool((out != 7).all())
