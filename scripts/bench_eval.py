"""Pose-evaluation timing on the GPU box (HIP events, every shape warmed up first):
  add_adds           one launch for B frames x O objects with M-point models (ffb6d_amd.evaluate.add_adds)
  eval_poses         TorchEval.eval_poses on solve_poses-shaped results + the per-batch read-back at summary time
  torch_reference    the reference's formulas (basic_utils.py:651-669) restated in plain torch on the same device: one
                     object at a time, the [N,N,3] broadcast for ADD-S, a .item() per distance (as eval_metric does)
and the largest difference between the two on the batch.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ffb6d_amd import evaluate, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--objects", type=int, default=5)
ap.add_argument("--model-points", type=int, default=2620)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

dev = torch.device("cuda:0")
B, O, M = args.batch, args.objects, args.model_points
clouds = {c: synth.model_cloud(100 + c, M) for c in range(1, O + 1)}
models = evaluate.ModelPoints(clouds, device=dev)
pairs = [synth.eval_pose_pair(200 + q, "near") for q in range(B * O)]
pred = np.stack([p for p, _ in pairs])
gt = np.stack([g for _, g in pairs])
cls = [1 + q % O for q in range(B * O)]
results = [(np.arange(1, O + 1), pred[b * O:(b + 1) * O].astype(np.float64), np.zeros((O, 9, 3), np.float32)) for b in range(B)]
cls_ids = np.arange(1, O + 1).reshape(1, O, 1).repeat(B, 0)
RTs = gt.reshape(B, O, 3, 4)
pred_d, gt_d = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
clouds_d = {c: torch.from_numpy(v).to(dev) for c, v in clouds.items()}


def torch_reference():
    """basic_utils.py:651-669 restated: per object, both transforms by torch.mm, ADD-S over the [N,N,3] broadcast."""
    add, adds = [], []
    for q in range(B * O):
        p3ds, P, G = clouds_d[cls[q]], pred_d[q], gt_d[q]
        pd = torch.mm(p3ds, P[:, :3].transpose(1, 0)) + P[:, 3]
        g = torch.mm(p3ds, G[:, :3].transpose(1, 0)) + G[:, 3]
        add.append(torch.mean(torch.norm(pd - g, dim=1)).item())
        n = p3ds.shape[0]
        d = torch.norm(pd.view(1, n, 3).repeat(n, 1, 1) - g.view(n, 1, 3).repeat(1, n, 1), dim=2)
        adds.append(torch.mean(torch.min(d, dim=1)[0]).item())
    return np.array(add), np.array(adds)


def run_add_adds():
    return evaluate.add_adds(pred_d, gt_d, cls, models)


def run_eval_poses():
    te = evaluate.TorchEval(n_cls=O + 1, models=models, sym_cls_ids=[])
    te.eval_poses(results, cls_ids, RTs)
    te._flush()
    return te


def timed(fn, steps):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


ms_kernel = timed(run_add_adds, args.steps)
ms_eval = timed(run_eval_poses, args.steps)
ms_ref = timed(torch_reference, max(1, args.steps // 10))
add, adds = (t.cpu().numpy() for t in run_add_adds())
ref_add, ref_adds = torch_reference()
pairs_n = B * O * M * M
print(json.dumps({
    "batch": B, "objects_per_frame": O, "model_points": M,
    "add_adds_ms_per_batch": ms_kernel, "eval_poses_ms_per_batch": ms_eval, "torch_reference_ms_per_batch": ms_ref,
    "speedup_vs_torch_reference": ms_ref / ms_kernel,
    "pair_distances_per_s": pairs_n / (ms_kernel * 1e-3),
    "max_abs_diff_add": float(np.abs(add - ref_add).max()), "max_abs_diff_adds": float(np.abs(adds - ref_adds).max()),
}))
