"""Instance-aware ICP timing and effect on the GPU box (ffb6d_amd.refine.icp_refine_instances, pose.solve_instances_refined): writes
profiles/icp_instances_bench.json and prints it.  Scene: 8 frames x 5 classes x 2 instances in 12288-point frames, 2048-point surface
models (tests/icp_inst_ref.py), every instance a partial view of at most --view-points points under its own pose, the two instances of a
class 0.3 m apart; the share --free of every instance's points has instance 0 in the map.  ICP: 10 iterations, gate 0.02 m.

  (a) icp_refine over the 40 (frame, class) problems, each under the pose of the class's first instance: the class form, the yardstick;
  (b) icp_refine_instances, map mode, over the 80 instance problems;
  (c) the same in nearest mode (one more pass over P x count distances per iteration, and the distances of stopped problems);
  (d) solve_instances next to solve_instances_refined in both modes on the same frames (votes = true offsets + noise);
  (e) ADD of the 80 instances before and after ICP in both modes.
The calls of a group alternate in one process; median / min / max of --reps after two warm-up calls of every shape.  Times are host
clocks around work that ends in a device synchronise."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_inst_ref as iref  # noqa: E402
from ffb6d_amd import evaluate, pose, refine, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--n-points", type=int, default=12288)
ap.add_argument("--classes", type=int, default=5)
ap.add_argument("--model-points", type=int, default=2048)
ap.add_argument("--view-points", type=int, default=1000)
ap.add_argument("--free", type=float, default=0.4)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_instances_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
MAX_ITER, MAX_DIST, N_KPS = 10, 0.02, 8


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def summary(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=len(ms))


def alternate(fns, reps):
    for fn in fns.values():                                              # warm-up: every shape of the timed window
        fn()
        fn()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(timed(fn))
    return {k: summary(v) for k, v in times.items()}


def scene():
    rng = np.random.RandomState(5)
    B, N, C = args.batch, args.n_points, args.classes
    models = [None] + [iref.surface_model(300 + c, args.model_points) for c in range(C)]
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
                view = iref.partial_view(models[c], gt, 7000 + 100 * b + 10 * c + i, clutter=0.0)[:args.view_points]
                at = np.sort(rng.choice(np.flatnonzero(mask[b] == 0), len(view), replace=False))
                pcld[b, at], mask[b, at] = view, c
                inst[b, at] = np.where(rng.rand(len(at)) < args.free, 0, i)
                p = view.astype(np.float64)
                ctr_of[b, 0, at] = p - (gt[:, :3] @ mesh_ctr[c] + gt[:, 3]) + 0.004 * rng.randn(len(at), 3)
                kp_of[b][:, at] = p[None] - (mesh_kps[c] @ gt[:, :3].T + gt[:, 3])[:, None] + 0.004 * rng.randn(N_KPS, len(at), 3)
                rows.append((b, c, i, pred, gt))
    return dict(pcld=pcld, mask=mask, inst=inst, ctr_of=ctr_of, kp_of=kp_of, mesh_kps=mesh_kps, mesh_ctr=mesh_ctr, models=models,
                frame_of=np.array([r[0] for r in rows], np.int32), class_of=np.array([r[1] for r in rows], np.int32),
                inst_of=np.array([r[2] for r in rows], np.int32), T0=np.stack([r[3] for r in rows]), gt=np.stack([r[4] for r in rows]))


s = scene()
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
pcld, mask, inst, ctr_of, kp_of = (up(s[k]) for k in ("pcld", "mask", "inst", "ctr_of", "kp_of"))
frame_of, class_of, inst_of, T0 = (up(s[k]) for k in ("frame_of", "class_of", "inst_of", "T0"))
prepared = refine.PreparedModels(evaluate.ModelPoints(iref.models_of(s["models"]), device=dev))
first = torch.arange(0, len(s["frame_of"]), 2, device=dev)              # the class problems: one per (frame, class)
kw = dict(max_iter=MAX_ITER, max_dist=MAX_DIST)
out = dict(batch=args.batch, n_points=args.n_points, classes=args.classes, model_points=args.model_points, reps=args.reps,
           free_share=args.free, max_iter=MAX_ITER, max_dist=MAX_DIST, problems_class=int(first.numel()), problems_instance=int(frame_of.numel()),
           scene_points_per_instance=float((s["mask"] > 0).sum() / len(s["frame_of"])))

# (a) - (c) the three loops, alternating
loops = {"a_icp_refine_class": lambda: refine.icp_refine(pcld, mask, T0[first], frame_of[first], class_of[first], prepared, **kw),
         "b_icp_refine_instances_map": lambda: refine.icp_refine_instances(pcld, mask, inst, T0, frame_of, class_of, inst_of, prepared, mode="map", **kw),
         "c_icp_refine_instances_nearest": lambda: refine.icp_refine_instances(pcld, mask, inst, T0, frame_of, class_of, inst_of, prepared,
                                                                               mode="nearest", **kw)}
out.update(alternate(loops, args.reps))
out["c_over_b"] = out["c_icp_refine_instances_nearest"]["median_ms"] / out["b_icp_refine_instances_map"]["median_ms"]
out["b_over_a"] = out["b_icp_refine_instances_map"]["median_ms"] / out["a_icp_refine_class"]["median_ms"]

# (e) what it does to the poses
add = lambda T: np.array([iref.add(s["models"][c], T[p], s["gt"][p]) for p, c in enumerate(s["class_of"])])      # noqa: E731
before = add(s["T0"])
out["e_add_before"] = dict(mean=float(before.mean()), max=float(before.max()))
for mode in ("map", "nearest"):
    T, st = refine.icp_refine_instances(pcld, mask, inst, T0, frame_of, class_of, inst_of, prepared, mode=mode, **kw)
    after = add(T.cpu().numpy())
    out["e_add_after_" + mode] = dict(mean=float(after.mean()), max=float(after.max()), improved=int((after <= before).sum()),
                                      mean_pairs=float(st["n_pairs"].float().mean()))

# (d) the solver with and without the refinement
solver = (pcld, mask, ctr_of, kp_of, s["mesh_kps"], s["mesh_ctr"], 4)
res = pose.solve_instances(*solver, min_fraction=0.05)
out["d_estimates"] = int(res["est_RT"].shape[0])
opts = lambda mode: dict(models=prepared, mode=mode, **kw)      # noqa: E731
out.update(alternate({"d_solve_instances": lambda: pose.solve_instances(*solver, min_fraction=0.05),
                      "d_solve_instances_refined_map": lambda: pose.solve_instances_refined(*solver, refine=opts("map"), min_fraction=0.05),
                      "d_solve_instances_refined_nearest": lambda: pose.solve_instances_refined(*solver, refine=opts("nearest"), min_fraction=0.05)},
                     args.reps))

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out, sort_keys=True))
