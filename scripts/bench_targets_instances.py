"""Device time of the per-instance pose targets (train_data.pose_targets_instances) for a batch of 8 frames, N = 12288 points,
K = 8 keypoints and 10 instances per frame (4 classes, so every frame holds several instances of a class), against
  * train_data.pose_targets at the same B, N, K with O = 10 object slots per frame (the class image of the same scene): the
    same output traffic, one launch where the new call makes two;
  * the same arithmetic in plain torch operations on the same device (gather, double matmul, subtract, bincount).

    python scripts/bench_targets_instances.py [--iters 200] [--rounds 7] [--json profiles/targets_instances_bench.json]

Each figure is the time of one CALL of the Python entry point -- output allocation and launches included -- from device events
around `iters` back-to-back calls, all inputs already on the device.  The three variants are timed in interleaved rounds in one
process; the record holds the median and the minimum over the rounds.  Before timing, the three are compared on the data they
are timed on: labels equal, offsets equal (the torch arithmetic may contract or reorder: 1e-6 m)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ffb6d_amd import synth, train_data  # noqa: E402

B, H, W, N, N_CLS, N_KPS, PER_FRAME = 8, 480, 640, 12288, 5, 8, 10


def torch_targets(cld, choose, inst_img, frame_of, class_of, poses, kps, ctr):
    """the rule of ffb6d_pose_targets_inst in torch operations (choose is taken to lie inside the image)"""
    Bn, n_inst, n_cls = cld.shape[0], frame_of.shape[0], kps.shape[0]
    i = inst_img.reshape(Bn, -1).gather(1, choose)
    ii = i.clamp(0, n_inst - 1).long()
    cls = class_of[ii]
    ok = (i >= 0) & (i < n_inst) & (frame_of[ii] == torch.arange(Bn, device=cld.device)[:, None]) & (cls >= 1) & (cls < n_cls)
    safe = class_of.long().clamp(0, n_cls - 1)
    m = torch.cat([kps[safe], ctr[safe][:, None]], 1).double()
    x = m @ poses[:, :, :3].transpose(1, 2) + poses[:, None, :, 3]                     # [I,K+1,3]
    ofs = ((cld.double()[:, :, None, :] - x[ii]) * ok[:, :, None, None]).float()
    return dict(labels=torch.where(ok, cls, torch.zeros_like(cls)), inst_of_point=torch.where(ok, i, torch.full_like(i, -1)),
                kp_targ_ofst=ofs[:, :, :-1].contiguous(), ctr_targ_ofst=ofs[:, :, -1].contiguous(), kp_3ds=x[:, :-1].float(),
                ctr_3ds=x[:, -1].float(), n_points=torch.bincount(ii[ok], minlength=n_inst).int())


def time_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "targets_instances_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    n_inst = B * PER_FRAME
    frame_np = np.repeat(np.arange(B), PER_FRAME).astype(np.int32)
    class_np = rng.randint(1, N_CLS, n_inst).astype(np.int32)
    poses_np = np.zeros((n_inst, 3, 4))
    for i in range(n_inst):
        poses_np[i, :, :3], poses_np[i, :, 3] = synth.random_rotation(rng), [rng.randn() * 0.3, rng.randn() * 0.3, 0.8 + 0.4 * rng.rand()]
    # every frame: vertical stripes of its 10 instances, a fifth of the pixels background
    stripe = (np.arange(W) * PER_FRAME // W)[None, None, :] + (PER_FRAME * np.arange(B))[:, None, None]
    inst_np = np.where(rng.rand(B, H, W) < 0.8, np.broadcast_to(stripe, (B, H, W)), -1).astype(np.int32)
    label_np = np.where(inst_np >= 0, class_np[np.clip(inst_np, 0, None)], 0).astype(np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                                                       # noqa: E731
    cld = up((rng.rand(B, N, 3) - 0.5).astype(np.float32))
    choose = up(rng.randint(0, H * W, (B, N)))
    inst_img, label_img, frame_of, class_of, poses = up(inst_np), up(label_np), up(frame_np), up(class_np), up(poses_np)
    kps, ctr = up((rng.rand(N_CLS, N_KPS, 3) - 0.5).astype(np.float32)), up((rng.rand(N_CLS, 3) - 0.5).astype(np.float32))
    slot_ids, slot_RTs = class_of.reshape(B, PER_FRAME).contiguous(), poses.reshape(B, PER_FRAME, 3, 4).contiguous()

    variants = {
        "pose_targets_instances": lambda: train_data.pose_targets_instances(cld, choose, inst_img, frame_of, class_of, poses, kps, ctr),
        "pose_targets_O10": lambda: train_data.pose_targets(cld, choose, label_img, slot_ids, slot_RTs, kps, ctr),
        "torch_ops": lambda: torch_targets(cld, choose, inst_img, frame_of, class_of, poses, kps, ctr),
    }
    got, old, want = (variants[k]() for k in ("pose_targets_instances", "pose_targets_O10", "torch_ops"))
    torch.cuda.synchronize()
    assert torch.equal(got["labels"], want["labels"]) and torch.equal(got["labels"], old["labels"])
    assert torch.equal(got["inst_of_point"], want["inst_of_point"]) and torch.equal(got["n_points"], want["n_points"])
    diff = {k: float((got[k] - want[k]).abs().max()) for k in ("kp_targ_ofst", "ctr_targ_ofst", "kp_3ds", "ctr_3ds")}
    assert max(diff.values()) <= 1e-6, diff
    owned = int((got["labels"] > 0).sum())

    for fn in variants.values():                                            # warm-up of every shape the timed window uses
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            rounds[k].append(time_ms(fn, args.iters))
    out_bytes = 4 * B * N * (3 * N_KPS + 3 + 2) + 4 * n_inst * (3 * N_KPS + 4)
    res = {}
    for k, ms in rounds.items():
        res[k] = dict(call_us_median=round(1e3 * float(np.median(ms)), 2), call_us_min=round(1e3 * min(ms), 2),
                      rounds_us=[round(1e3 * m, 2) for m in ms])
        print(f"{k:26s} median {res[k]['call_us_median']:8.2f} us / call   min {res[k]['call_us_min']:8.2f} us", flush=True)
    line = dict(bench="targets_instances", batch=B, height=H, width=W, n_points=N, n_classes=N_CLS, n_kps=N_KPS,
                instances_per_frame=PER_FRAME, iters=args.iters, rounds=args.rounds, owned_points=owned,
                output_bytes_instances=out_bytes, max_abs_diff_vs_torch=diff, gpu=torch.cuda.get_device_name(0),
                what="one call of the Python entry point (allocation and launches included), device events around `iters` calls, "
                     "variants interleaved per round", results=res)
    print(json.dumps(line))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(line, fh, indent=1)


if __name__ == "__main__":
    main()
