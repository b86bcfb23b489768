"""Device time of the training-sample arithmetic (ffb6d_amd/train_data.py) for a batch of 8 frames of 480x640, N = 12800,
22 classes, 8 keypoints, 6 objects per frame; against the numpy restatements on one CPU thread.

    python scripts/bench_train_data.py [--iters 50] [--json OUT]

Prints one line per measurement (ms per batch, device events around `iters` calls after warm-up) and, at the end, one
JSON line with all of them."""
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

from ffb6d_amd import synth, train_data  # noqa: E402

B, H, W, N, N_CLS, N_KPS, N_OBJ = 8, 480, 640, 12800, 22, 8, 6


def device_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def cpu_ms(fn, reps=2):
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    torch.set_num_threads(1)
    from train_data_ref import filter_ref, hsv_jitter_ref, pose_targets_ref
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    rgb_np = rng.randint(0, 256, (B, 3, H, W)).astype(np.uint8)
    rgb = torch.from_numpy(rgb_np).to(dev)
    lab = torch.from_numpy(rng.randint(0, N_CLS, (B, H, W)).astype(np.uint8)).to(dev)
    depth = torch.from_numpy((0.5 + rng.rand(B, H, W)).astype(np.float32) * (rng.rand(B, H, W) > 0.1)).to(dev)
    cld = torch.from_numpy((rng.rand(B, N, 3) - 0.5).astype(np.float32)).to(dev)
    choose = torch.from_numpy(rng.randint(0, H * W, (B, N))).to(dev)
    ids = np.stack([rng.choice(np.arange(1, N_CLS), N_OBJ, replace=False) for _ in range(B)])
    RTs = np.stack([[synth.random_rotation(rng).tolist() for _ in range(N_OBJ)] for _ in range(B)])
    RTs = np.concatenate([RTs, rng.rand(B, N_OBJ, 3, 1)], axis=3)
    kps = (rng.rand(N_CLS, N_KPS, 3) - 0.5).astype(np.float32)
    ctr = (rng.rand(N_CLS, 3) - 0.5).astype(np.float32)
    ids_d = torch.from_numpy(ids.astype(np.int32)).to(dev)
    RTs_d = torch.from_numpy(RTs).to(dev)
    kps_d, ctr_d = torch.from_numpy(kps).to(dev), torch.from_numpy(ctr).to(dev)

    res = {}

    def rec(name, ms, cpu=None):
        res[name] = dict(device_ms=round(ms, 4), **({"cpu_1thread_ms": round(cpu, 1)} if cpu is not None else {}))
        print(f"{name:28s} {ms:8.3f} ms / batch" + (f"   numpy, 1 thread: {cpu:9.1f} ms" if cpu is not None else ""), flush=True)

    lab_np, cld_np, ch_np = lab.cpu().numpy(), cld.cpu().numpy(), choose.cpu().numpy()
    rec("pose_targets", device_ms(lambda: train_data.pose_targets(cld, choose, lab, ids_d, RTs_d, kps_d, ctr_d), args.iters),
        cpu_ms(lambda: [pose_targets_ref(cld_np[b], lab_np[b].reshape(-1)[ch_np[b]], ids[b], RTs[b], kps, ctr) for b in range(B)]))
    forced = {"hsv": dict(hsv=(1.3, 1.2)), "sharpen": dict(sharpen=10.5), "motion": dict(motion=(37, 15)),
              "gauss3": dict(gauss=(3, 0.7)), "gauss5": dict(gauss=(5, 0.7)), "noise": dict(noise_sigma=12, extra_noise=True)}
    cpu_stage = {
        "hsv": lambda: [hsv_jitter_ref(rgb_np[b, 0], rgb_np[b, 1], rgb_np[b, 2], 1.3, 1.2) for b in range(B)],
        "sharpen": lambda: [filter_ref(rgb_np[b], train_data.sharpen_taps(10.5)) for b in range(B)],
        "motion": lambda: [filter_ref(rgb_np[b], train_data.motion_blur_taps(37, 15)) for b in range(B)],
        "gauss3": lambda: [filter_ref(rgb_np[b], train_data.gaussian_taps(3, 0.7)) for b in range(B)],
        "gauss5": lambda: [filter_ref(rgb_np[b], train_data.gaussian_taps(5, 0.7)) for b in range(B)],
        "noise": lambda: [np.clip(rgb_np[b] + rng.randn(3, H, W) * 12, 0, 255).astype(np.uint8) for b in range(B)],
    }
    for name, p in forced.items():
        rec("rgb_add_noise:" + name, device_ms(lambda: train_data.rgb_add_noise(rgb, [p] * B, 7), args.iters),
            cpu_ms(cpu_stage[name], reps=1))
    mix = [train_data.draw_noise_params(np.random.RandomState(100 + b), "ycb") for b in range(B)]
    rec("rgb_add_noise:reference_mix", device_ms(lambda: train_data.rgb_add_noise(rgb, mix, 7), args.iters))
    rec("add_real_back", device_ms(lambda: train_data.add_real_back(rgb, depth, lab, rgb, depth, lab, "ycb"), args.iters))
    nrm = torch.zeros((B, 3, H, W), dtype=torch.float32, device=dev)
    common = (rgb, depth, lab, synth.LINEMOD_K, N, ids_d, RTs_d, kps_d, ctr_d)
    rec("builder:no_augmentation", device_ms(lambda: train_data.assemble_training_batch(*common, normals=nrm, seed=1), 10))
    rec("builder:augmentation", device_ms(lambda: train_data.assemble_training_batch(
        *common, normals=nrm, seed=1, synthetic=[True] * B, noise_params=mix, back=dict(rgb=rgb, depth=depth, label=lab),
        second_noise_params=[mix[b] if b % 5 == 0 else None for b in range(B)], aug_seed=2), 10))
    line = dict(bench="train_data", batch=B, height=H, width=W, n_points=N, n_classes=N_CLS, n_kps=N_KPS, n_objects=N_OBJ,
                gpu=torch.cuda.get_device_name(0), results=res)
    print(json.dumps(line))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(line, fh, indent=1)


if __name__ == "__main__":
    main()
