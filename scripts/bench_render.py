"""The rasteriser (ffb6d_amd/render.py) on one training batch: 8 frames of 480 x 640 with 5 instances each of a subdivision-5
icosphere (20480 faces, radius 0.1 m, 0.6 - 1.2 m from the camera), and one close-up instance that fills a frame (the same
sphere at 0.13 m, and a two-triangle quad larger than the frame).  ms per render call (rgb, depth, label, visible) for the forms
of the raster pass: 0 = a lane per triangle, 1 = a wavefront per triangle, -1 = by box area.  Event timing after warm-up, median
of repeated runs, clocks as found.

    python scripts/bench_render.py [--out profiles/render_bench.json] [--repeats 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ffb6d_amd import render, synth  # noqa: E402


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


def pose(t, R):
    T = np.zeros((3, 4))
    T[:, :3], T[:, 3] = R, t
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--instances", type=int, default=5)
    ap.add_argument("--subdiv", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, per, H, W = args.frames, args.instances, 480, 640
    K = synth.LINEMOD_K
    quad = dict(xyz=np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32),
                rgb=np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255]], np.uint8), faces=np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    meshes = render.PreparedMeshes([None, synth.sphere_mesh(args.subdiv, 0.1, seed=1), quad], dev)
    rng = np.random.RandomState(2)
    T = []
    for _ in range(B * per):
        z = 0.6 + 0.6 * rng.rand()
        T.append(pose([(rng.rand() - 0.5) * 0.8 * z, (rng.rand() - 0.5) * 0.6 * z, z], synth.random_rotation(rng)))
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)     # noqa: E731
    batch = (up(np.stack(T), np.float64), up(np.repeat(np.arange(B), per), np.int32), up(np.ones(B * per), np.int32))
    one = lambda t, c: (up(np.stack([t]), np.float64), up([0], np.int32), up([c], np.int32))      # noqa: E731
    cases = dict(batch=(batch, B), close_up_sphere=(one(pose([0, 0, 0.13], np.eye(3)), 1), 1), close_up_quad=(one(pose([0, 0, 0.9], np.eye(3)), 2), 1))
    outputs = ("rgb", "depth", "label", "visible")
    res = dict(device=torch.cuda.get_device_name(0), frames=B, instances_per_frame=per, faces=int(meshes.max_faces), H=H, W=W,
               atomic="global 64-bit minimum", cases={})
    for name, ((Td, fo, co), nb) in cases.items():
        row = {}
        for form in (0, 1, -1):
            render.set_form(form)
            row[f"form_{form}"] = timed(lambda: render.render(meshes, Td, fo, co, K, nb, H, W, outputs=outputs), args.repeats)
        render.set_form(0)
        out = render.render(meshes, Td, fo, co, K, nb, H, W, outputs=outputs)
        row["visible_pixels"] = int(out["visible"].sum())
        res["cases"][name] = row
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
