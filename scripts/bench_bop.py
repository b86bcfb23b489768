"""The BOP pose errors (ffb6d_amd/bop.py, csrc/bop_eval.hip) at the shape an evaluation batch has, next to the obvious alternative
on the same device: the same arithmetic as batched plain-torch ops in float64 and in float32.
  8 frames x 5 objects = 40 rows at 480 x 640, the 20 480-face sphere of the render bench (10 242 vertices), 10 taus;
  mssd_mspd with a symmetry set of 1 and of 315 transforms (one continuous axis at the default step);
  vsd as a whole, and its two parts: rendering the 80 single-instance depth frames, comparing the three images.
The torch form of MSSD / MSPD transforms all points under all symmetries of all rows with matrix products, 64 symmetries at a
time (315 at once are 3 GB per intermediate in float64); the torch form of the VSD comparison works on the rendered frames.
ms per call from device events after warm-up, kernel and torch forms alternating in one run, median of the repeats, clocks as found.

    python scripts/bench_bop.py [--out profiles/bop_bench.json] [--repeats 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ffb6d_amd import bop, evaluate, render, synth  # noqa: E402


def alternating(fns, repeats, warmup=3):
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


def torch_mssd_mspd(pts, sym_R, sym_t, est, gt, Kq, step=64):
    """pts [n,3], sym_R [S,3,3], sym_t [S,3], est / gt [Q,3,4], Kq [Q,3,3] in one dtype -> mssd [Q], mspd [Q]"""
    def proj(P):                                                                 # [..., n, 3] -> u, v
        return (Kq[:, 0, 0].view(-1, *[1] * (P.dim() - 2)) * P[..., 0] / P[..., 2] + Kq[:, 0, 2].view(-1, *[1] * (P.dim() - 2)),
                Kq[:, 1, 1].view(-1, *[1] * (P.dim() - 2)) * P[..., 1] / P[..., 2] + Kq[:, 1, 2].view(-1, *[1] * (P.dim() - 2)))

    Pe = pts @ est[:, :, :3].transpose(1, 2) + est[:, None, :, 3]               # [Q,n,3]
    ue, ve = proj(Pe)
    best_s = best_p = None
    for s0 in range(0, sym_R.shape[0], step):
        Rs, ts = sym_R[s0:s0 + step], sym_t[s0:s0 + step]
        Rg = gt[:, None, :, :3] @ Rs[None]                                       # [Q,s,3,3]
        tg = (gt[:, None, :, :3] @ ts[None, :, :, None])[..., 0] + gt[:, None, :, 3]
        Pg = pts @ Rg.transpose(2, 3) + tg[:, :, None, :]                        # [Q,s,n,3]
        d2 = ((Pe[:, None] - Pg) ** 2).sum(-1).amax(-1).amin(-1)
        ug, vg = proj(Pg)
        p2 = (ue[:, None] - ug) ** 2 + (ve[:, None] - vg) ** 2
        p2 = torch.where((Pe[:, None, :, 2] > 0) & (Pg[..., 2] > 0), p2, torch.full_like(p2, float("inf"))).amax(-1).amin(-1)
        best_s = d2 if best_s is None else torch.minimum(best_s, d2)
        best_p = p2 if best_p is None else torch.minimum(best_p, p2)
    return best_s.sqrt(), best_p.sqrt()


def torch_vsd(test, d_est, d_gt, frm, cls, Kd, diam, delta, taus):
    """the comparison of bop.vsd_compare in float32 torch ops -> vsd f64 [Q, n_tau]"""
    Q, H, W = d_est.shape
    Kq = Kd[frm.long()].float()
    c = torch.arange(W, device=test.device, dtype=torch.float32).view(1, 1, W)
    r = torch.arange(H, device=test.device, dtype=torch.float32).view(1, H, 1)
    fx, fy, cx, cy = (Kq[:, i, j].view(Q, 1, 1) for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))

    def dist(z):
        X, Y = (c - cx) * z / fx, (r - cy) * z / fy
        return torch.sqrt(X * X + Y * Y + z * z)

    t = test[frm.long()]
    t = torch.where(torch.isfinite(t) & (t > 0), t, torch.zeros_like(t))
    dt, de, dg = dist(t), dist(d_est), dist(d_gt)
    vis_gt = (dg > 0) & ((dt == 0) | (dg - dt <= delta))
    vis_est = (de > 0) & ((dt == 0) | (de - dt <= delta) | vis_gt)
    uni, inter = (vis_gt | vis_est).sum((1, 2)), vis_gt & vis_est
    e = (dg - de).abs() / diam[cls.long()].view(Q, 1, 1)
    cost = torch.stack([(inter & (e >= tau)).sum((1, 2)) for tau in taus], 1)
    n_inter = inter.sum((1, 2))
    out = (cost + (uni - n_inter)[:, None]).double() / uni.clamp(min=1)[:, None].double()
    return torch.where(uni[:, None] == 0, torch.ones_like(out), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--instances", type=int, default=5)
    ap.add_argument("--subdiv", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bop.py measures on the GPU; no device is visible")
    dev = torch.device("cuda:0")
    B, per, H, W = args.frames, args.instances, 480, 640
    Q = B * per
    mesh = synth.sphere_mesh(args.subdiv, 0.1, seed=1)
    meshes = render.PreparedMeshes([None, mesh], dev)
    models = evaluate.ModelPoints([None, mesh["xyz"]], dev)
    diam = np.array([1.0, 0.2], np.float32)
    rng = np.random.RandomState(2)
    gt, est = [], []
    for _ in range(Q):
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
    res = dict(device=torch.cuda.get_device_name(0), rows=Q, frames=B, H=H, W=W, points=int(models.max_points), faces=int(meshes.max_faces),
               taus=len(bop.VSD_TAUS), mssd_mspd={}, vsd={})

    pts64 = models.pts.double()
    Kq = Kd[frm.long()]
    for name, sets in (("syms_1", [None, None]), ("syms_315", [None, bop.symmetry_transforms(continuous=[((0, 0, 1), (0, 0, 0))])])):
        syms = bop.SymmetrySets(sets, dev)
        f32 = [t.float() for t in (syms.sym_R, syms.sym_t, est, gt, Kq)]           # cast outside the timed calls
        fns = dict(kernel=lambda: bop.mssd_mspd(est, gt, cls, frm, Kd, models, syms),
                   torch_f64=lambda: torch_mssd_mspd(pts64, syms.sym_R, syms.sym_t, est, gt, Kq),
                   torch_f32=lambda: torch_mssd_mspd(models.pts, *f32))
        row = alternating(fns, args.repeats)
        mine, theirs = fns["kernel"](), fns["torch_f64"]()
        pairs = Q * int(syms.max_syms) * int(models.max_points)
        row.update(symmetries=int(syms.max_syms), point_pairs=pairs, gpairs_per_s=pairs / (row["kernel"]["median_ms"] * 1e-3) / 1e9,
                   torch_f64_over_kernel=row["torch_f64"]["median_ms"] / row["kernel"]["median_ms"],
                   torch_f32_over_kernel=row["torch_f32"]["median_ms"] / row["kernel"]["median_ms"],
                   max_rel_diff_to_torch_f64=[float(((a - b).abs() / b.abs().clamp(min=1e-300)).max()) for a, b in zip(mine, theirs)])
        res["mssd_mspd"][name] = row

    test = render.render(meshes, gt, frm, cls, Kd, B, H, W, outputs=("depth",))["depth"]
    test = torch.where(test > 0, test + 0.002 * torch.randn(test.shape, device=dev, generator=torch.Generator(dev).manual_seed(1)), test)
    diam_d, taus = up(diam, np.float32), [float(t) for t in np.asarray(bop.VSD_TAUS, np.float32)]
    taus_d = up(bop.VSD_TAUS, np.float32)                                        # uploaded once, as bop.vsd does for its chunks
    d_est, d_gt = (d.contiguous() for d in bop.render_pairs(meshes, est, gt, cls, frm, Kd, H, W))
    fns = dict(vsd=lambda: bop.vsd(test, est, gt, cls, frm, Kd, meshes, diam_d),
               render_part=lambda: bop.render_pairs(meshes, est, gt, cls, frm, Kd, H, W),
               compare_kernel=lambda: bop.vsd_compare(test, d_est, d_gt, cls, frm, Kd, diam_d, taus=taus_d),
               compare_torch_f32=lambda: torch_vsd(test, d_est, d_gt, frm, cls, Kd, diam_d, bop.VSD_DELTA, taus))
    row = alternating(fns, args.repeats)
    mine, theirs = fns["compare_kernel"]()[0], fns["compare_torch_f32"]()
    nbytes = 12 * Q * H * W
    row.update(image_bytes=nbytes, compare_gb_per_s=nbytes / (row["compare_kernel"]["median_ms"] * 1e-3) / 1e9,
               torch_over_kernel=row["compare_torch_f32"]["median_ms"] / row["compare_kernel"]["median_ms"],
               max_abs_diff_to_torch=float((mine - theirs).abs().max()), mean_vsd=float(mine.mean()))
    res["vsd"] = row
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
