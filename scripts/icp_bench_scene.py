"""The scene of scripts/bench_icp_instances.py as a function, for scripts/bench_icp_plane.py (that script builds it inline from its
arguments; this is the same code with the same seed and draw order, so both measure on the same frames): `batch` frames x `classes` classes x 2
instances in frames of `n_points` points, surface models of `model_points` points (tests/icp_inst_ref.py), every instance a partial
view of at most `view_points` points under its own pose, the two instances of a class 0.3 m apart; the share `free` of every
instance's points has instance 0 in the map.  Votes (ctr_of, kp_of) = true offsets + noise, for the solver."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)
import icp_inst_ref as iref  # noqa: E402
from ffb6d_amd import synth  # noqa: E402

N_KPS = 8


def scene(batch, n_points, classes, model_points, view_points, free):
    rng = np.random.RandomState(5)
    B, N, C = batch, n_points, classes
    models = [None] + [iref.surface_model(300 + c, model_points) for c in range(C)]
    mesh_kps = ((rng.rand(C + 1, N_KPS, 3) - 0.5) * 0.1).astype(np.float32)
    mesh_ctr = np.zeros((C + 1, 3), np.float32)
    pcld = (rng.rand(B, N, 3) * [3.0, 1.6, 0.5] + [-1.5, -0.8, 2.0]).astype(np.float32)      # background behind the objects
    mask, inst = np.zeros((B, N), np.int64), np.zeros((B, N), np.uint8)
    ctr_of, kp_of = (0.2 * rng.randn(B, 1, N, 3)).astype(np.float32), (0.2 * rng.randn(B, N_KPS, N, 3)).astype(np.float32)
    rows = []
    for b in range(B):
        for c in range(1, C + 1):
            for i in (1, 2):
                pred, gt = (x.astype(np.float64) for x in synth.eval_pose_pair(1000 * b + 10 * c + i, "near"))
                t = np.array([0.45 * (c - (C + 1) / 2), 0.3 * i - 0.45 + 0.02 * rng.randn(), 1.0 + 0.2 * rng.rand()])
                pred[:, 3] += t - gt[:, 3]
                gt[:, 3] = t
                view = iref.partial_view(models[c], gt, 7000 + 100 * b + 10 * c + i, clutter=0.0)[:view_points]
                at = np.sort(rng.choice(np.flatnonzero(mask[b] == 0), len(view), replace=False))
                pcld[b, at], mask[b, at] = view, c
                inst[b, at] = np.where(rng.rand(len(at)) < free, 0, i)
                p = view.astype(np.float64)
                ctr_of[b, 0, at] = p - (gt[:, :3] @ mesh_ctr[c] + gt[:, 3]) + 0.004 * rng.randn(len(at), 3)
                kp_of[b][:, at] = p[None] - (mesh_kps[c] @ gt[:, :3].T + gt[:, 3])[:, None] + 0.004 * rng.randn(N_KPS, len(at), 3)
                rows.append((b, c, i, pred, gt))
    return dict(pcld=pcld, mask=mask, inst=inst, ctr_of=ctr_of, kp_of=kp_of, mesh_kps=mesh_kps, mesh_ctr=mesh_ctr, models=models,
                frame_of=np.array([r[0] for r in rows], np.int32), class_of=np.array([r[1] for r in rows], np.int32),
                inst_of=np.array([r[2] for r in rows], np.int32), T0=np.stack([r[3] for r in rows]), gt=np.stack([r[4] for r in rows]))
