"""Multi-instance pose solver timing on the GPU box (ffb6d_amd.pose.solve_instances / mean_shift_multi): writes
profiles/pose_instances_bench.json and prints it.  Workload: 8 frames x 5 classes of 12288-point frames.

  (a) solve_instances(max_instances=4) on frames with TWO instances of every class;
  (b) solve_instances(max_instances=1) next to solve_poses(use_ctr_clus_flter=True, refine_mask=False) on the single-instance batch
      of scripts/bench_pose.py -- the same poses as bits; the two are timed alternately, and the spread of solve_poses over its
      own repetitions is recorded next to the difference, with the time of one instance-map launch;
  (c) mean_shift_multi on the centre-vote sets of (a) next to the single fit on the same sets (the difference is what the peel
      costs) and next to the peel written in plain torch ops on the same device, starting from the same converged points.
Times are host clocks around work that ends in a device synchronise (the solvers read back), after warm-up of every shape."""
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
from ffb6d_amd import _lib, pose, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--n-points", type=int, default=12288)
ap.add_argument("--classes", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_instances_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")


def two_instance_frame(seed, n_pts, n_cls, mesh_kps, mesh_ctr, n_kps=8, noise=0.004, outliers=0.1, bg_frac=0.3):
    """synth.make_pose_case with two instances per class (0.5 m apart in y), vectorised"""
    rng = np.random.RandomState(seed)
    n_obj = 2 * n_cls
    owner = rng.choice(n_obj + 1, size=n_pts, p=[bg_frac] + [(1 - bg_frac) / n_obj] * n_obj)
    pcld = rng.uniform(-1, 1, (n_pts, 3)) * [1.0, 0.6, 0.5] + [0.0, 0.0, 1.1]
    ctr_of, kp_of = 0.2 * rng.randn(n_pts, 3), 0.2 * rng.randn(n_kps, n_pts, 3)
    mask = np.zeros(n_pts, np.int64)
    for o in range(n_obj):
        c, which = o // 2 + 1, o % 2
        R = synth.random_rotation(rng)
        t = np.array([0.5 * (c - (n_cls + 1) / 2), 0.5 * which - 0.25 + 0.02 * rng.randn(), 1.0 + 0.2 * rng.rand()])
        sel = np.flatnonzero(owner == o + 1)
        local = rng.randn(len(sel), 3)
        local *= (0.07 * rng.rand(len(sel)) ** (1 / 3) / np.linalg.norm(local, axis=1))[:, None]
        p = local @ R.T + t
        bad = (rng.rand(len(sel)) < outliers)[:, None]
        pcld[sel], mask[sel] = p, c
        ctr_of[sel] = p - (R @ mesh_ctr[c] + t) + noise * rng.randn(len(sel), 3) + bad * 0.15 * rng.randn(len(sel), 3)
        kp_of[:, sel] = p[None] - (mesh_kps[c] @ R.T + t)[:, None] + noise * rng.randn(n_kps, len(sel), 3) + bad[None] * 0.15 * rng.randn(n_kps, len(sel), 3)
    return dict(pcld=pcld.astype(np.float32), mask=mask, ctr_of=ctr_of[None].astype(np.float32), kp_of=kp_of.astype(np.float32))


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
    return times


def torch_peel(C, counts, h, K):
    """the rule of include/ffb6d_pose.h in plain torch ops, set by set: C f32 [G,M,3] converged points"""
    out = []
    for g in range(C.shape[0]):
        P = C[g, :int(counts[g])]
        near = torch.cdist(P, P) < h
        alive = torch.ones(len(P), dtype=torch.bool, device=P.device)
        sizes, centres = [], []
        for _ in range(K):
            n = (near & alive[None, :]).sum(1) * alive
            w = torch.argmax(n)
            sizes.append(n[w])
            centres.append(P[w])
            alive = alive & ~near[w]
        out.append((torch.stack(sizes), torch.stack(centres)))
    return out


stack = lambda cases, key: torch.from_numpy(np.stack([c[key] for c in cases])).to(dev)      # noqa: E731
single = [synth.make_pose_case(900 + b, n_pts=args.n_points, n_obj=args.classes, mesh_seed=9) for b in range(args.batch)]
mk, mc = single[0]["mesh_kps"], single[0]["mesh_ctr"]
double = [two_instance_frame(950 + b, args.n_points, args.classes, mk, mc) for b in range(args.batch)]
one = [stack(single, k) for k in ("pcld", "mask", "ctr_of", "kp_of")]
two = [stack(double, k) for k in ("pcld", "mask", "ctr_of", "kp_of")]
out = dict(batch=args.batch, n_points=args.n_points, classes=args.classes, reps=args.reps)

# (a) two instances per class
res = pose.solve_instances(*two, mk, mc, 4, min_fraction=0.05)
out["a_estimates"] = int(res["est_RT"].shape[0])
out["a_instances_expected"] = 2 * args.classes * args.batch
t = alternate({"solve_instances_K4": lambda: pose.solve_instances(*two, mk, mc, 4, min_fraction=0.05)}, args.reps)
out["a_solve_instances_K4"] = summary(t["solve_instances_K4"])

# (b) one instance per class: the multi entry at K = 1 next to solve_poses
want = pose.solve_poses(*one, mk, mc, use_ctr_clus_flter=True, refine_mask=False)
got = pose.solve_instances(*one, mk, mc, 1)
out["b_same_bits"] = bool(np.array_equal(got["est_RT"].cpu().numpy(), np.concatenate([p for _, p, _ in want])))
t = alternate({"solve_poses": lambda: pose.solve_poses(*one, mk, mc, use_ctr_clus_flter=True, refine_mask=False),
               "solve_instances_K1": lambda: pose.solve_instances(*one, mk, mc, 1)}, args.reps)
out["b_solve_poses"], out["b_solve_instances_K1"] = summary(t["solve_poses"]), summary(t["solve_instances_K1"])
out["b_overhead_ms"] = out["b_solve_instances_K1"]["median_ms"] - out["b_solve_poses"]["median_ms"]
out["b_solve_poses_spread_ms"] = out["b_solve_poses"]["max_ms"] - out["b_solve_poses"]["min_ms"]
B, N = one[1].shape
frame_np, class_np = pose._frame_class_pairs(one[1], None, B, mk.shape[0])
frame_of, class_of = pose._i32(frame_np, dev), pose._i32(class_np, dev)
sets1, counts1 = pose.vote_sets(one[0], one[2], one[1], frame_of, class_of)
cl1 = pose.mean_shift_multi(sets1, counts1, pose.RADIUS, 1)[1]
t = alternate({"instance_map": lambda: pose.instance_map(sets1, cl1, counts1, frame_of, B, N)}, args.reps)
out["b_instance_map"] = summary(t["instance_map"])

# (c) the peel alone: centre-vote sets of the two-instance frames
frame_np, class_np = pose._frame_class_pairs(two[1], None, B, mk.shape[0])
frame_of, class_of = pose._i32(frame_np, dev), pose._i32(class_np, dev)
sets2, counts2 = pose.vote_sets(two[0], two[2], two[1], frame_of, class_of)
conv = torch.zeros_like(sets2)
_lib.load().ffb6d_pose_set_converged_out(conv.data_ptr())
try:
    base = pose.mean_shift_multi(sets2, counts2, pose.RADIUS, 4)
    torch.cuda.synchronize()
finally:
    _lib.load().ffb6d_pose_set_converged_out(None)
host_counts = counts2.cpu().numpy()
C = conv[:, :, :3].contiguous()
ref = torch_peel(C, host_counts, pose.RADIUS, 4)
out["c_sets"], out["c_mean_points"] = int(sets2.shape[0]), float(host_counts.mean())
out["c_torch_peel_agrees"] = bool(all(torch.equal(s.int(), base[2][g]) and torch.equal(c, base[0][g]) for g, (s, c) in enumerate(ref)))
t = alternate({"mean_shift_single": lambda: pose.mean_shift(sets2, counts2, pose.RADIUS),
               "mean_shift_multi_K4": lambda: pose.mean_shift_multi(sets2, counts2, pose.RADIUS, 4),
               "torch_peel_K4": lambda: torch_peel(C, host_counts, pose.RADIUS, 4)}, args.reps)
for k, v in t.items():
    out["c_" + k] = summary(v)
out["c_peel_in_kernel_ms"] = out["c_mean_shift_multi_K4"]["median_ms"] - out["c_mean_shift_single"]["median_ms"]

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out, sort_keys=True))
