"""Pose evaluation on the MI355X (ffb6d_amd/evaluate.py over csrc/pose_eval.hip): ADD / ADD-S against the reference's own
results (tests/golden/eval_small.npz, make_golden_eval.py) and a float64 restatement, batch independence and determinism,
the exact self-consistency of the two distances, edge cases and argument errors, eval_metric against the reference's
per-class lists, and TorchEval scoring solve_poses / SensorToPose output."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from ffb6d_amd import _lib, evaluate, pose, synth
from test_eval_cpu import ref_add_adds

pytestmark = pytest.mark.gpu

spec = importlib.util.spec_from_file_location("make_golden_eval", os.path.join(GOLDEN, "make_golden_eval.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "eval_small.npz"))


def close(got, want):
    return abs(float(got) - float(want)) <= 1e-6 + 1e-6 * abs(float(want))


def test_cal_add_and_adds_match_the_reference(device, golden):
    for i in range(gen.n_add_cases()):
        p3ds, pred, gt = (torch.from_numpy(a).to(device) for a in gen.add_inputs(i))
        add = evaluate.cal_add_cuda(pred, gt, p3ds)
        adds = evaluate.cal_adds_cuda(pred, gt, p3ds)
        assert add.dim() == 0 and adds.dim() == 0
        assert close(add.item(), golden[f"add{i}"]), (i, add.item(), golden[f"add{i}"])
        assert close(adds.item(), golden[f"adds{i}"]), (i, adds.item(), golden[f"adds{i}"])


def _batch(sizes, rows, seed=0):
    models = [synth.model_cloud(1000 + seed + c, n) for c, n in enumerate(sizes)]
    pairs = [synth.eval_pose_pair(2000 + seed + k, kind) for k, (_, kind) in enumerate(rows)]
    return models, [c for c, _ in rows], np.stack([p for p, _ in pairs]), np.stack([g for _, g in pairs])


def test_add_adds_matches_float64_beyond_one_lds_tile(device):
    sizes = (1, 255, 256, 257, 1025, 2620, 4500, 9000)
    rows = [(c, kind) for c in range(len(sizes)) for kind in ("near", "far")]
    models, cls, pred, gt = _batch(sizes, rows)
    mp = evaluate.ModelPoints(models, device=device)
    add, adds = (t.cpu().numpy() for t in evaluate.add_adds(pred, gt, cls, mp))
    for q, c in enumerate(cls):
        want_add, want_adds = ref_add_adds(models[c], pred[q], gt[q])
        assert close(add[q], want_add), (q, sizes[c], add[q], want_add)
        assert close(adds[q], want_adds), (q, sizes[c], adds[q], want_adds)


def test_rows_do_not_depend_on_the_batch_and_runs_repeat(device):
    sizes = (63, 2000, 2620, 300, 5000)
    rows = [(c % len(sizes), ("near", "far", "zero")[k % 3]) for k, c in enumerate((0, 1, 2, 3, 4, 2, 1, 2, 4, 0, 2, 3))]
    models, cls, pred, gt = _batch(sizes, rows, seed=7)
    mp = evaluate.ModelPoints(models, device=device)
    add, adds = evaluate.add_adds(pred, gt, cls, mp)
    add2, adds2 = evaluate.add_adds(pred, gt, cls, mp)
    assert torch.equal(add, add2) and torch.equal(adds, adds2)
    for q in range(len(cls)):
        a1, s1 = evaluate.add_adds(pred[q:q + 1], gt[q:q + 1], cls[q:q + 1], mp)
        assert torch.equal(a1[0], add[q]) and torch.equal(s1[0], adds[q]), q
    # a row at the end of a different batch
    a3, s3 = evaluate.add_adds(np.concatenate([pred[5:], pred[:1]]), np.concatenate([gt[5:], gt[:1]]), cls[5:] + cls[:1], mp)
    assert torch.equal(a3[-1], add[0]) and torch.equal(s3[-1], adds[0])


def test_adds_never_exceeds_add_and_identical_poses_give_zero(device):
    sizes = (1, 17, 640, 2620)
    rows = [(c, kind) for c in range(len(sizes)) for kind in ("near", "far", "zero", "same")]
    models, cls, pred, gt = _batch(sizes, rows, seed=3)
    add, adds = (t.cpu().numpy() for t in evaluate.add_adds(pred, gt, cls, evaluate.ModelPoints(models, device=device)))
    assert np.all(adds <= add)
    same = [q for q, (_, kind) in enumerate(rows) if kind == "same"]
    assert np.all(add[same] == 0) and np.all(adds[same] == 0)


def test_symmetric_model_and_zero_prediction(device):
    p3ds, pred, gt = gen.add_inputs(gen.n_add_cases() - 1)          # ring model turned by its symmetry angle
    mp = evaluate.ModelPoints([p3ds], device=device)
    add, adds = evaluate.add_adds(pred, gt, [0], mp)
    assert adds.item() <= 1e-6 and add.item() > 0.01
    zero = np.zeros((3, 4), np.float32)
    add, adds = evaluate.add_adds(zero[None], gt[None], [0], mp)
    g = p3ds.astype(np.float64) @ gt[:, :3].astype(np.float64).T + gt[:, 3]
    want = np.linalg.norm(g, axis=1).mean()
    assert close(add.item(), want) and close(adds.item(), want)


def test_empty_class_bad_ids_and_short_workspace(device):
    models = [synth.model_cloud(3001, 100), np.zeros((0, 3), np.float32), synth.model_cloud(3002, 700)]
    mp = evaluate.ModelPoints(models, device=device)
    pred, gt = synth.eval_pose_pair(3003)
    add, adds = evaluate.add_adds(np.stack([pred] * 3), np.stack([gt] * 3), [0, 1, 2], mp)
    add, adds = add.cpu().numpy(), adds.cpu().numpy()
    assert np.isnan(add[1]) and np.isnan(adds[1]) and np.isfinite(add[[0, 2]]).all()

    lib = _lib.load()
    P = torch.from_numpy(np.stack([pred, pred])).to(device)
    G = torch.from_numpy(np.stack([gt, gt])).to(device)
    out_a = torch.full((2,), 7.0, device=device)
    out_s = torch.full((2,), 7.0, device=device)
    need = lib.ffb6d_pose_add_adds_workspace_bytes(2, 700)
    ws = torch.empty((need,), dtype=torch.uint8, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream

    def call(cls, nbytes):
        c = torch.tensor(cls, dtype=torch.int32, device=device)
        return lib.ffb6d_pose_add_adds_f32(mp.pts.data_ptr(), mp.begin.data_ptr(), mp.n_cls, c.data_ptr(), P.data_ptr(),
                                           G.data_ptr(), 2, out_a.data_ptr(), out_s.data_ptr(), ws.data_ptr(), nbytes, stream)
    assert call([0, 3], need) == -1 and "class_of[1]" in _lib.last_error()
    assert call([-1, 0], need) == -1
    assert call([0, 2], need - 4) == -3 and "workspace" in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.all(out_a == 7.0) and torch.all(out_s == 7.0)
    assert call([0, 2], need) == 0
    torch.cuda.synchronize()
    assert torch.all(out_a != 7.0) and torch.all(out_s != 7.0)
    with pytest.raises(_lib.FFB6DNativeError):
        evaluate.add_adds(pred[None], gt[None], [5], mp)


def _unpack(golden, i, name):
    lens = golden[f"ycb{i}_{name}_len"]
    flat = golden[f"ycb{i}_{name}"]
    ends = np.cumsum(lens)
    return [list(flat[e - n:e]) for n, e in zip(lens, ends)]


@pytest.mark.parametrize("i", range(len(gen.YCB_CASES)))
def test_eval_metric_matches_the_reference(device, golden, i):
    pose_golden = np.load(os.path.join(GOLDEN, "pose_small.npz"))
    a = gen.ycb_inputs(i, pose_golden)
    mp = evaluate.ModelPoints(gen.ycb_models(), device=device)
    add, adds, kp = evaluate.eval_metric(torch.from_numpy(a["cls_ids"]).to(device), a["pred_pose_lst"], a["pred_cls_ids"],
                                         torch.from_numpy(a["RTs"]).to(device), None, None, torch.from_numpy(a["gt_kps"]).to(device),
                                         None, a["pred_kpc_lst"], models=mp, n_cls=gen.N_CLS)
    for name, got in (("add", add), ("adds", adds)):
        want = _unpack(golden, i, name)
        assert [len(x) for x in got] == [len(x) for x in want], name
        for c in range(gen.N_CLS):
            for g, w in zip(got[c], want[c]):
                assert close(g, w), (name, c, g, w)
    want = _unpack(golden, i, "kp")
    assert [len(x) for x in kp] == [len(x) for x in want]
    for c in range(gen.N_CLS):
        assert [float(v) for v in kp[c]] == [float(v) for v in want[c]], c


def _frames(B, n_pts, n_obj, n_cls):
    cases = [synth.make_pose_case(60 + b, n_pts=n_pts, n_obj=n_obj, n_cls=n_cls, mesh_seed=5) for b in range(B)]
    gts = [synth.pose_case_ground_truth(c, extra_seed=70 + b) for b, c in enumerate(cases)]
    return cases, gts


def test_eval_pose_parallel_equals_eval_metric_per_frame(device):
    B, n_obj, n_cls = 3, 3, 6
    cases, gts = _frames(B, 1500, n_obj, n_cls)
    models = evaluate.ModelPoints({c: synth.model_cloud(4000 + c, 400 + 150 * c) for c in range(1, n_cls)}, device=device)
    st = lambda k: torch.from_numpy(np.stack([c[k] for c in cases])).to(device)        # noqa: E731
    n_gt = len(gts[0][0])
    cls_ids = torch.from_numpy(np.stack([g[0] for g in gts])).to(device)
    RTs = torch.from_numpy(np.stack([g[1] for g in gts])).to(device)
    gt_kps = torch.from_numpy(np.stack([g[2] for g in gts])).to(device)
    te = evaluate.TorchEval(n_cls=n_cls, models=models)
    te.eval_pose_parallel(st("pcld"), None, st("mask"), st("ctr_of"), None, None, 0, cls_ids, RTs, st("kp_of"), gt_kps, None,
                          mesh_kps=cases[0]["mesh_kps"], mesh_ctr=cases[0]["mesh_ctr"], r_lst=cases[0]["r_lst"])
    res = te.cal_auc()
    want_add, want_adds, want_kp = ([[] for _ in range(n_cls)] for _ in range(3))
    for b in range(B):
        ids, poses, kps = pose.solve_poses(st("pcld")[b:b + 1], st("mask")[b:b + 1], st("ctr_of")[b:b + 1], st("kp_of")[b:b + 1],
                                           cases[0]["mesh_kps"], cases[0]["mesh_ctr"], r_lst=cases[0]["r_lst"])[0]
        add, adds, kp = evaluate.eval_metric(cls_ids[b], list(poses), ids, RTs[b], None, None, gt_kps[b], None, list(kps),
                                             models=models, n_cls=n_cls)
        for acc, part in ((want_add, add), (want_adds, adds), (want_kp, kp)):
            for c in range(n_cls):
                acc[c] += part[c]
    assert res["add_dis_lst"] == want_add and res["adds_dis_lst"] == want_adds
    assert [[float(v) for v in x] for x in res["pred_kp_errs"]] == [[float(v) for v in x] for x in want_kp]
    assert len(res["add_dis_lst"][0]) == B * (n_obj + 1) and n_gt == n_obj + 3
    assert len(te.pred_id2pose_lst) == B


def test_eval_poses_on_pipeline_results(device):
    from ffb6d_amd import pipeline
    from test_forward_gpu import build
    if device.type != "cuda":
        pytest.skip("streams: device only")
    B, N, H, W, n_cls = 2, 1024, 120, 160, 5
    cases, gts = _frames(B, N, 3, n_cls)
    st = lambda k: torch.from_numpy(np.stack([c[k] for c in cases])).to(device)        # noqa: E731
    fixed = (st("pcld"), st("mask"), st("ctr_of"), st("kp_of"))
    net = build(n_cls, N, device)
    pipe = pipeline.SensorToPose(net, synth.LINEMOD_K, N, cases[0]["mesh_kps"], cases[0]["mesh_ctr"], r_lst=cases[0]["r_lst"],
                                 seed=3, pose_inputs=lambda inp, out: fixed)
    fr = synth.make_batch(2, B, n_points=N, height=H, width=W)
    batch = {"rgb": torch.from_numpy(fr["rgb"]).to(device),
             "depth": torch.from_numpy(np.ascontiguousarray(fr["dpt_xyz"][:, 2])).to(device)}
    results = pipe.run([batch], overlap=False)[0]
    models = evaluate.ModelPoints({c: synth.model_cloud(5000 + c, 300 + 100 * c) for c in range(1, n_cls)}, device=device)
    cls_ids = np.stack([g[0] for g in gts])
    RTs, gt_kps = np.stack([g[1] for g in gts]), np.stack([g[2] for g in gts])
    te = evaluate.TorchEval(n_cls=n_cls, models=models)
    te.eval_poses(results, cls_ids, RTs, gt_kps=gt_kps)
    direct = pose.solve_poses(*fixed, cases[0]["mesh_kps"], cases[0]["mesh_ctr"], r_lst=cases[0]["r_lst"])
    te2 = evaluate.TorchEval(n_cls=n_cls, models=models)
    te2.eval_poses(direct, cls_ids, RTs, gt_kps=gt_kps)
    a, b = te.cal_auc(), te2.cal_auc()
    for k in ("add_dis_lst", "adds_dis_lst", "add_auc_lst", "adds_auc_lst", "add_s_auc_lst"):
        assert a[k] == b[k], k
    assert sum(len(x) for x in a["add_dis_lst"][1:]) == B * 4
