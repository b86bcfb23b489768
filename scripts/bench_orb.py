"""Texture-aware object keypoints (ffb6d_amd/objinfo.py, csrc/orb.hip): the ORB detector, the lift and the whole
ObjectInfo.from_meshes at the sizes of the reference's tool -- 21 objects x 9 views of 480 x 640 renders of vertex-coloured
icospheres (2562 vertices, 5120 faces, radii 5 .. 15 cm).
  detect_9 / detect_189      orb_detect with its defaults on the rendered frames of one object / of all 21;
  detect_noise_9 / _189      the same on uniform-noise frames, where the candidate lists are longest (the rank count is quadratic);
  lift_189                   ffb6d_orb_lift_f32 + ffb6d_orb_compact_f32 on the 189 frames' keypoints;
  from_meshes_21             the whole call, and its stages from events right around every native call.
ms per call from device events after warm-up, every function once per round, median of the repeats in one run, clocks as found.
rule_bytes: what the detector must move by its rule -- rgb read once, every gray level written once and read once by the detector
and (but the last) once by the next level's resize, the outputs written once -- so that a share of the HBM peak can be stated.

    python scripts/bench_orb.py [--out profiles/orb_bench.json] [--repeats 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ffb6d_amd import _lib, objinfo, render, synth  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, MI355X
H, W, V = 480, 640, 9


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


def level_size(n, l):
    return (2 * n * 5 ** l + 6 ** l) // (2 * 6 ** l)


def rule_bytes(F, L=8, Q=500):
    px = [level_size(H, l) * level_size(W, l) for l in range(L)]
    return F * (3 * H * W + 2 * sum(px) + sum(px[:-1]) + Q * (5 * 4 + 8) + 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--objects", type=int, default=21)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_orb.py measures on the GPU; no device is visible")
    dev = torch.device("cuda:0")
    S = args.objects
    meshes = [None] + [synth.sphere_mesh(4, radius=0.05 + 0.1 * i / max(S - 1, 1), seed=i) for i in range(S)]
    prepared = render.PreparedMeshes(meshes, device=dev)
    radius = objinfo.box_info(prepared)[2]
    poses = objinfo.view_poses(radius, 3, 3)[1:].reshape(-1, 3, 4).contiguous()                      # the S objects, class 0 left out
    F = S * V
    out = render.render(prepared, poses, torch.arange(F, dtype=torch.int32, device=dev),
                        torch.arange(1, S + 1, dtype=torch.int32, device=dev).repeat_interleave(V), objinfo.DEFAULT_K, F, H, W,
                        outputs=("rgb", "depth", "visible"))
    rgb, depth, visible = out["rgb"], out["depth"], out["visible"]
    noise = torch.randint(0, 256, (F, 3, H, W), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(1))
    count, kps, _ = objinfo.orb_detect(rgb)
    Q = int(kps.shape[1])
    K = np.asarray(objinfo.DEFAULT_K)
    lib = _lib.load()
    slot_pts = torch.empty((F, Q, 3), dtype=torch.float32, device=dev)
    slot_ok = torch.empty((F, Q), dtype=torch.int32, device=dev)
    pts = torch.empty((F * Q, 3), dtype=torch.float32, device=dev)
    begin = torch.empty((S + 1,), dtype=torch.int64, device=dev)
    n_found = torch.empty((S,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def lift():
        _lib.check(lib.ffb6d_orb_lift_f32(kps.data_ptr(), count.data_ptr(), depth.data_ptr(), visible.data_ptr(), poses.data_ptr(), F, Q, H, W,
                                          K[0, 0], K[1, 1], K[0, 2], K[1, 2], 500, slot_pts.data_ptr(), slot_ok.data_ptr(), st), "lift")
        _lib.check(lib.ffb6d_orb_compact_f32(slot_pts.data_ptr(), slot_ok.data_ptr(), S, V, Q, pts.data_ptr(), begin.data_ptr(),
                                             n_found.data_ptr(), st), "compact")

    rows = alternating(dict(detect_9=lambda: objinfo.orb_detect(rgb[:V]), detect_189=lambda: objinfo.orb_detect(rgb),
                            detect_noise_9=lambda: objinfo.orb_detect(noise[:V]), detect_noise_189=lambda: objinfo.orb_detect(noise),
                            lift_189=lift, from_meshes_21=lambda: objinfo.ObjectInfo.from_meshes(prepared, n_keypoints=8)), args.repeats)
    for name, frames in (("detect_9", V), ("detect_189", F), ("detect_noise_9", V), ("detect_noise_189", F)):
        r = rows[name]
        r["frames"], r["rule_bytes"] = frames, rule_bytes(frames)
        r["share_of_hbm_peak"] = r["rule_bytes"] / (1e-3 * r["median_ms"]) / HBM_PEAK
        r["us_per_frame"] = 1e3 * r["median_ms"] / frames
    _lib.TRACER = _lib.Tracer()                                # events right around every native call of from_meshes
    for _ in range(args.repeats):
        objinfo.ObjectInfo.from_meshes(prepared, n_keypoints=8)
    torch.cuda.synchronize()
    stages = {k: dict(ms_per_call=v["total_ms"] / args.repeats, launches_per_call=v["launches"] / args.repeats)
              for k, v in _lib.TRACER.summary().items()}
    _lib.TRACER = None
    rows["from_meshes_21"]["stages"] = stages
    info = objinfo.ObjectInfo.from_meshes(prepared, n_keypoints=8)
    res = dict(device=torch.cuda.get_device_name(0), objects=S, views=V, frame=[H, W], quota_sum=Q, hbm_peak_bytes_per_s=HBM_PEAK,
               keypoints_per_rendered_frame=float(count.float().mean()), keypoints_per_noise_frame=float(objinfo.orb_detect(noise[:V])[0].float().mean()),
               lifted_points_per_object=[int(v) for v in info.n_found.cpu()[1:]], rows=rows)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
