"""BOP scene evaluation (ffb6d_amd/bop.py, csrc/bop_scene.hip) at the shape an evaluation batch has, next to the obvious
alternatives: the visibility arithmetic as plain torch ops on the same device, the matching as a numpy loop on the host.
  The batch of scripts/bench_bop.py: 8 frames x 5 objects = 40 rows at 480 x 640, the 20 480-face sphere;
  visib_compare with and without masks, and vsd_compare on the same images for a bytes-per-second comparison (the visibility pass
  reads two images per row -- the test image and the render -- where VSD reads three);
  match for 10^4 groups of 1 x 1 and of 4 x 4 at 110 configurations (10 VSD columns x 11 thresholds), against the numpy loop of
  tests/bop_scene_ref.py over a subsample of the groups, scaled to all of them.
ms per call from device events after warm-up, kernel and torch forms alternating in one run, median of the repeats, clocks as found.

    python scripts/bench_bop_scene.py [--out profiles/bop_scene_bench.json] [--repeats 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ffb6d_amd import bop, render, synth  # noqa: E402
from bench_bop import alternating  # noqa: E402


def torch_visib(test, d_obj, frm, Kd, delta, masks):
    """the comparison of bop.visib_compare in float32 torch ops -> info i32 [Q,12], visib_fract f64 [Q], mask u8 or None"""
    Q, H, W = d_obj.shape
    Kq = Kd[frm.long()].float()
    c = torch.arange(W, device=test.device, dtype=torch.float32).view(1, 1, W)
    r = torch.arange(H, device=test.device, dtype=torch.float32).view(1, H, 1)
    fx, fy, cx, cy = (Kq[:, i, j].view(Q, 1, 1) for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))

    def dist(z):
        z = torch.where(torch.isfinite(z) & (z > 0), z, torch.zeros_like(z))
        X, Y = (c - cx) * z / fx, (r - cy) * z / fy
        return torch.sqrt(X * X + Y * Y + z * z)

    def box(sel):
        cols, rows = sel.any(1), sel.any(2)
        ci = torch.arange(W, device=sel.device).view(1, W)
        ri = torch.arange(H, device=sel.device).view(1, H)
        x0, x1 = torch.where(cols, ci, W).amin(1), torch.where(cols, ci, -1).amax(1)
        y0, y1 = torch.where(rows, ri, H).amin(1), torch.where(rows, ri, -1).amax(1)
        b = torch.stack([x0, y0, x1 - x0 + 1, y1 - y0 + 1], 1)
        return torch.where(cols.any(1)[:, None], b, torch.full_like(b, -1))

    dt, dg = dist(test[frm.long()]), dist(d_obj)
    obj = dg > 0
    valid = obj & (dt > 0)
    visib = obj & ((dt == 0) | (dg - dt <= delta))
    support = valid & (dg - dt <= delta) & (dt - dg <= delta)
    counts = torch.stack([m.sum((1, 2)) for m in (obj, valid, visib, support)], 1)
    info = torch.cat([counts, box(obj), box(visib)], 1).int()
    fract = torch.where(counts[:, 0] == 0, torch.zeros((), dtype=torch.float64, device=test.device),
                        counts[:, 2].double() / counts[:, 0].clamp(min=1).double())
    return info, fract, visib.to(torch.uint8) if masks else None


def match_bench(dev, G, E, T, n_col, n_thr, repeats, sample):
    import bop_scene_ref as ref
    rng = np.random.RandomState(E * 100 + T)
    tb = ref.group_tables([(E, T)] * G)
    err = np.ascontiguousarray(rng.rand(G * E * T, n_col))
    score = rng.rand(G * E).astype(np.float32)
    thr = np.ascontiguousarray(np.sort(rng.rand(G, n_thr), axis=1))
    err_d, score_d, thr_d = (torch.from_numpy(a).to(dev) for a in (err, score, thr))
    row = alternating(dict(kernel=lambda: bop.match(err_d, score_d, tb, thr_d)), repeats)
    got_e, got_g = (t.cpu().numpy() for t in bop.match(err_d, score_d, tb, thr_d))
    sub = ref.group_tables([(E, T)] * sample)
    t0 = time.perf_counter()
    want_e, want_g = ref.match(sub, err[:sample * E * T], score[:sample * E], thr[:sample])
    host_ms = (time.perf_counter() - t0) * 1e3
    row.update(groups=G, estimates=E, instances=T, configurations=n_col * n_thr, numpy_loop_groups=sample, numpy_loop_ms=host_ms,
               numpy_loop_ms_scaled_to_all_groups=host_ms * G / sample,
               equal_to_numpy_loop=bool(np.array_equal(got_e[:sample * E], want_e) and np.array_equal(got_g[:sample * T], want_g)),
               greedy_passes_per_s=G * n_col * n_thr / (row["kernel"]["median_ms"] * 1e-3))
    row["numpy_loop_over_kernel"] = row["numpy_loop_ms_scaled_to_all_groups"] / row["kernel"]["median_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--instances", type=int, default=5)
    ap.add_argument("--subdiv", type=int, default=5)
    ap.add_argument("--groups", type=int, default=10000)
    ap.add_argument("--loop-groups", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bop_scene.py measures on the GPU; no device is visible")
    dev = torch.device("cuda:0")
    B, per, H, W = args.frames, args.instances, 480, 640
    Q = B * per
    mesh = synth.sphere_mesh(args.subdiv, 0.1, seed=1)
    meshes = render.PreparedMeshes([None, mesh], dev)
    rng = np.random.RandomState(2)
    gt, est = [], []
    for _ in range(Q):                                                           # the poses of scripts/bench_bop.py
        z = 0.6 + 0.6 * rng.rand()
        T = np.zeros((3, 4))
        T[:, :3], T[:, 3] = synth.random_rotation(rng), [(rng.rand() - 0.5) * 0.8 * z, (rng.rand() - 0.5) * 0.6 * z, z]
        E = T.copy()
        E[:, :3] = E[:, :3] @ synth.rot_z(0.05 * rng.randn())
        E[:, 3] += 0.01 * rng.randn(3)
        gt.append(T)
        est.append(E)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)     # noqa: E731
    gt, est = up(np.stack(gt), np.float64), up(np.stack(est), np.float64)
    cls, frm = up(np.ones(Q), np.int32), up(np.repeat(np.arange(B), per), np.int32)
    Kd = up(np.broadcast_to(synth.LINEMOD_K, (B, 3, 3)), np.float64)
    test = render.render(meshes, gt, frm, cls, Kd, B, H, W, outputs=("depth",))["depth"]
    test = torch.where(test > 0, test + 0.002 * torch.randn(test.shape, device=dev, generator=torch.Generator(dev).manual_seed(1)), test)
    diam_d, taus_d = up(np.array([1.0, 0.2]), np.float32), up(bop.VSD_TAUS, np.float32)
    d_est, d_gt = (d.contiguous() for d in bop.render_pairs(meshes, est, gt, cls, frm, Kd, H, W))
    res = dict(device=torch.cuda.get_device_name(0), rows=Q, frames=B, H=H, W=W, faces=int(meshes.max_faces))

    out_plain = bop.visib_compare(test, d_gt, frm, Kd)
    out_masks = bop.visib_compare(test, d_gt, frm, Kd, masks=True)
    fns = dict(visib_kernel=lambda: bop.visib_compare(test, d_gt, frm, Kd, out=out_plain),
               visib_kernel_masks=lambda: bop.visib_compare(test, d_gt, frm, Kd, out=out_masks),
               visib_torch_f32=lambda: torch_visib(test, d_gt, frm, Kd, bop.VSD_DELTA, False),
               visib_torch_f32_masks=lambda: torch_visib(test, d_gt, frm, Kd, bop.VSD_DELTA, True),
               vsd_compare_kernel=lambda: bop.vsd_compare(test, d_est, d_gt, cls, frm, Kd, diam_d, taus=taus_d),
               instance_info=lambda: bop.instance_info(test, gt, cls, frm, Kd, meshes))
    row = alternating(fns, args.repeats)
    mine, theirs = fns["visib_kernel_masks"](), fns["visib_torch_f32_masks"]()
    px = Q * H * W
    row.update(visib_image_bytes=8 * px, visib_masks_bytes=9 * px, vsd_image_bytes=12 * px,
               visib_gb_per_s=8 * px / (row["visib_kernel"]["median_ms"] * 1e-3) / 1e9,
               visib_masks_gb_per_s=9 * px / (row["visib_kernel_masks"]["median_ms"] * 1e-3) / 1e9,
               vsd_compare_gb_per_s=12 * px / (row["vsd_compare_kernel"]["median_ms"] * 1e-3) / 1e9,
               torch_over_kernel=row["visib_torch_f32"]["median_ms"] / row["visib_kernel"]["median_ms"],
               torch_over_kernel_masks=row["visib_torch_f32_masks"]["median_ms"] / row["visib_kernel_masks"]["median_ms"],
               rows_where_torch_counts_differ=int((mine[0][:, :4] != theirs[0][:, :4]).any(1).sum()),
               boxes_equal_to_torch=bool(torch.equal(mine[0][:, 4:], theirs[0][:, 4:])), mean_visib_fract=float(mine[1].mean()))
    res["visibility"] = row
    res["match"] = {name: match_bench(dev, args.groups, n, n, 10, 11, args.repeats, args.loop_groups) for name, n in (("groups_1x1", 1), ("groups_4x4", 4))}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
