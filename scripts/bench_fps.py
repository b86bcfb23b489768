"""Farthest-point sampling (ffb6d_amd/objinfo.py, csrc/fps.hip) at the two shapes an object set asks for, next to the obvious
alternative on the same device: the same loop in plain torch ops, one iteration per sample (gather the pick, squared distances,
minimum, arg-max: five launches a step).
  keypoints     21 sets x 20480 points (a subdivision-5 icosphere's faces as points), m = 8      -> streaming form
  model_clouds  21 sets x  8192 points, m = 2048                                                 -> resident form
Both start from index 0 of every set.  ms per call from device events after warm-up, kernel and torch loop alternating in one
run, median of the repeats, clocks as found; us per step = ms / m.  A call of objinfo.farthest_point_sampling also allocates its
outputs and fills the start table; native_call_us is the time between two events right around the library call (mean of the repeats).

    python scripts/bench_fps.py [--out profiles/fps_bench.json] [--repeats 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ffb6d_amd import _lib, evaluate, objinfo  # noqa: E402

FLT_MAX = float(np.finfo(np.float32).max)


def torch_loop(pts, m):
    """pts f32 [S,N,3] -> idx i64 [S,m]; the first pick is index 0"""
    S, N, _ = pts.shape
    rows = torch.arange(S, device=pts.device)
    min_dist = torch.full((S, N), FLT_MAX, device=pts.device)
    cur = torch.zeros(S, dtype=torch.int64, device=pts.device)
    idx = torch.empty((S, m), dtype=torch.int64, device=pts.device)
    for k in range(m):
        idx[:, k] = cur
        d = pts - pts[rows, cur][:, None]
        min_dist = torch.minimum(min_dist, (d * d).sum(-1))
        cur = min_dist.argmax(1)
    return idx


def alternating(fns, repeats, warmup=2):
    """every function once per round, so that drifting clocks and neighbours hit all of them alike"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), repeats=repeats) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--sets", type=int, default=21)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fps.py measures on the GPU; no device is visible")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    cap = objinfo.resident_capacity()
    res = dict(device=torch.cuda.get_device_name(0), sets=args.sets, resident_capacity=cap, shapes={})
    for name, n, m in (("keypoints", 20480, 8), ("model_clouds", 8192, 2048)):
        rng = np.random.RandomState(n)
        p = rng.randn(args.sets, n, 3)
        p = (0.1 * p / np.linalg.norm(p, axis=-1, keepdims=True)).astype(np.float32)      # points on spheres of radius 0.1 m
        pts = torch.from_numpy(p).to(dev)
        models = evaluate.ModelPoints(list(p), device=dev)                                 # prepared once per object set, like the meshes
        row = alternating(dict(kernel=lambda: objinfo.farthest_point_sampling(models, m, start=0),
                               torch_loop=lambda: torch_loop(pts, m)), args.repeats)
        for r in row.values():
            r["us_per_step"] = 1e3 * r["median_ms"] / m
        _lib.TRACER = _lib.Tracer(names=["fps"])                                           # events right around the native call: the launch alone
        for _ in range(args.repeats):
            objinfo.farthest_point_sampling(models, m, start=0)
        torch.cuda.synchronize()
        row["kernel"]["native_call_us"] = _lib.TRACER.summary()["fps"]["avg_us"]
        _lib.TRACER = None
        mine, theirs = objinfo.farthest_point_sampling(models, m, start=0)[0].long(), torch_loop(pts, m)
        row.update(points=n, m=m, form="streaming" if lib.ffb6d_fps_workspace_bytes(args.sets, n, m) else "resident",
                   torch_over_kernel=row["torch_loop"]["median_ms"] / row["kernel"]["median_ms"],
                   sets_with_the_same_picks=int((mine == theirs).all(1).sum()))
        res["shapes"][name] = row
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
