"""ICP refinement (ffb6d_amd/refine.py) on one batch of 8 frames x 5 objects at N = 12288, scene sets as synth.make_pose_case
produces them: ms per icp_refine call of 10 iterations for the scan and the pruned form of the search at 2048 and 8192 model
points per class, the pairs the pruned form evaluates as a fraction of the scan form's, and the pose stage (pose.solve_poses)
without and with refinement.  Event timing after warm-up, median of repeated runs, clocks as found.

    python scripts/bench_refine.py [--out profiles/refine_bench.json] [--repeats 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ffb6d_amd import _lib, evaluate, pose, refine, synth  # noqa: E402


def ball_models(n_cls, n_pts, seed=9):
    """the objects of make_pose_case are balls of 0.07 m filled uniformly: model clouds of the same shape"""
    rng = np.random.RandomState(seed)
    out = [None]
    for _ in range(1, n_cls):
        v = rng.randn(n_pts, 3)
        out.append((v / np.linalg.norm(v, axis=1, keepdims=True) * 0.07 * rng.rand(n_pts, 1) ** (1 / 3)).astype(np.float32))
    return out


def timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), repeats=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--objects", type=int, default=5)
    ap.add_argument("--points", type=int, default=12288)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--max-dist", type=float, default=0.02)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, n_obj, N = args.frames, args.objects, args.points
    n_cls = n_obj + 1
    cases = [synth.make_pose_case(300 + b, n_pts=N, n_obj=n_obj, n_cls=n_cls, mesh_seed=4) for b in range(B)]
    stack = lambda k: torch.from_numpy(np.stack([c[k] for c in cases])).to(dev)          # noqa: E731
    pcld, mask, ctr_of, kp_of = stack("pcld"), stack("mask"), stack("ctr_of"), stack("kp_of")
    frame_of = np.repeat(np.arange(B, dtype=np.int32), n_obj)
    class_of = np.tile(np.arange(1, n_cls, dtype=np.int32), B)
    rng = np.random.RandomState(1)
    T0 = np.stack([cases[b]["RT"][c] for b, c in zip(frame_of, class_of)])
    T0[:, :, 3] += 0.005 * rng.randn(len(T0), 3)                                          # the keypoint fit's kind of error
    T0d, fo, co = (torch.from_numpy(x).to(dev) for x in (T0, frame_of, class_of))
    counts = [int((cases[b]["mask"] == c).sum()) for b, c in zip(frame_of, class_of)]
    res = dict(device=torch.cuda.get_device_name(0), frames=B, objects=n_obj, points=N, iterations=args.iters, max_dist=args.max_dist,
               scene_points=dict(min=min(counts), max=max(counts), total=sum(counts)), sizes={})
    lib = _lib.load()
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    for n_model in (2048, 8192):
        prepared = refine.PreparedModels(evaluate.ModelPoints(ball_models(n_cls, n_model), device=dev))
        row = {}
        for name, form in (("scan", 0), ("pruned", 1)):
            refine.set_form(form)
            row[name] = timed(lambda: refine.icp_refine(pcld, mask, T0d, fo, co, prepared, max_iter=args.iters, max_dist=args.max_dist),
                              args.repeats)
            ctr.zero_()
            _lib.check(lib.ffb6d_icp_set_pair_counter(ctr.data_ptr()), "ffb6d_icp_set_pair_counter")
            refine.correspondences(pcld, mask, T0d, fo, co, prepared, max_dist=args.max_dist)
            row[name]["pairs_per_iteration"] = int(ctr.item())
            lib.ffb6d_icp_set_pair_counter(None)
        row["pruned_pair_fraction"] = row["pruned"]["pairs_per_iteration"] / max(row["scan"]["pairs_per_iteration"], 1)
        refine.set_form(0)
        T, st = refine.icp_refine(pcld, mask, T0d, fo, co, prepared, max_iter=args.iters, max_dist=args.max_dist)
        row["mean_pairs_kept"] = float(st["n_pairs"].float().mean())
        # the pose stage of the pipeline without and with the refinement (default form)
        kw = dict(r_lst=cases[0]["r_lst"])
        row["solve_poses"] = timed(lambda: pose.solve_poses(pcld, mask, ctr_of, kp_of, cases[0]["mesh_kps"], cases[0]["mesh_ctr"], **kw),
                                   max(args.repeats // 2, 3), warmup=2)
        row["solve_poses_refine"] = timed(lambda: pose.solve_poses(pcld, mask, ctr_of, kp_of, cases[0]["mesh_kps"], cases[0]["mesh_ctr"],
                                                                   refine=dict(models=prepared, max_iter=args.iters, max_dist=args.max_dist),
                                                                   **kw), max(args.repeats // 2, 3), warmup=2)
        res["sizes"][str(n_model)] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
