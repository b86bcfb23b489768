"""Device time of the ColorJitter kernels (ffb6d_amd/csrc/color_jitter.hip) for a batch of 8 frames of 480x640: each single operation
forced on, torchvision's full four-operation chain (per-frame random orders, the reference's ranges), and the same chain written in
plain torch ops on the same device, alternating with the kernels call by call.

    python scripts/bench_color_jitter.py [--iters 200] [--json OUT]    (default: profiles/color_jitter_bench.json)

Kernel rows time ffb6d_color_jitter_u8 alone (records already on the device): one pair of device events per call, median over
`iters` calls after warm-up.  `wrapper` rows time train_data.color_jitter, which also builds and uploads the records.  Bytes are what
the two passes must move: 6 per pixel (3 read + 3 written), 9 when the frame's chain holds a contrast (the sum pass reads the frame
once more).  Prints one line per measurement and, at the end, one JSON line with all of them."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ffb6d_amd import _lib, train_data  # noqa: E402

B, H, W = 8, 480, 640


def median_ms(fns, iters, warmup=10):
    """Median device time of each callable, the callables alternating call by call inside one run."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    pairs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for _ in fns]
    for i in range(iters):
        for k, fn in enumerate(fns):
            pairs[k][i][0].record()
            fn()
            pairs[k][i][1].record()
    torch.cuda.synchronize()
    return [float(np.median([a.elapsed_time(b) for a, b in p])) for p in pairs]


def kernel_call(rgb, params):
    """ffb6d_color_jitter_u8 with everything already on the device -> (callable, bytes moved, output tensor)"""
    lib = _lib.load()
    rec = train_data.jitter_records(params)
    _lib.check(lib.ffb6d_jitter_frames_check(rec.ctypes.data, B), "ffb6d_jitter_frames_check")
    need = int(lib.ffb6d_color_jitter_workspace_bytes(B, H, W))
    ws = torch.empty(need, dtype=torch.uint8, device=rgb.device)
    drec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(rgb.device)
    out = torch.empty_like(rgb)
    stream = torch.cuda.current_stream(rgb.device).cuda_stream

    def call():
        _lib.check(lib.ffb6d_color_jitter_u8(rgb.data_ptr(), drec.data_ptr(), out.data_ptr(), B, H, W, ws.data_ptr(), need, stream),
                   "ffb6d_color_jitter_u8")

    contrast = sum(1 in r["op"][:r["n_ops"]] for r in rec)
    return call, 3 * H * W * (2 * B + int(contrast)), out


# ---- the same chain in plain torch ops (float32 on the device; torchvision's tensor-backend formulas, not Pillow's bytes) ----------
def _grey(x):
    return 0.299 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3]


def _blend(x, d, f):
    return (d + f * (x - d)).clamp_(0, 255).floor_()


def _hue(x, h):
    x = x / 255.0
    r, g, b = x.unbind(1)
    mx, mn = x.max(1).values, x.min(1).values
    eq = mx == mn
    cr = mx - mn
    ones = torch.ones_like(mx)
    s = cr / torch.where(eq, ones, mx)
    crd = torch.where(eq, ones, cr)
    rc, gc, bc = (mx - r) / crd, (mx - g) / crd, (mx - b) / crd
    hr = (mx == r) * (bc - gc)
    hg = ((mx == g) & (mx != r)) * (2.0 + rc - bc)
    hb = ((mx != g) & (mx != r)) * (4.0 + gc - rc)
    hh = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    hh = (hh + h.view(-1, 1, 1)) % 1.0
    i = torch.floor(hh * 6.0)
    f = hh * 6.0 - i
    i = i.to(torch.int64) % 6
    p, q, t = mx * (1.0 - s), mx * (1.0 - s * f), mx * (1.0 - s * (1.0 - f))
    tab = torch.stack([torch.stack([mx, q, p, p, t, mx]), torch.stack([t, mx, mx, q, p, p]), torch.stack([p, p, t, mx, mx, q])])
    out = torch.gather(tab, 1, i.unsqueeze(0).unsqueeze(0).expand(3, 1, *i.shape)).squeeze(1)
    return (out.permute(1, 0, 2, 3) * 255.0).clamp_(0, 255).floor_()


def torch_chain(rgb, orders, fb, fc, fs, fh):
    """orders: the batch's frames grouped by order would be the fast way to write this; a training loader that jitters a batch with
    torch ops applies ONE order per batch, which is what is timed here (orders[0]), with per-frame factors."""
    x = rgb.float()
    for op in orders[0]:
        if op == 0:
            x = _blend(x, torch.zeros_like(x[:, :1, :1, :1]), fb)
        elif op == 1:
            x = _blend(x, _grey(x).mean((1, 2, 3), keepdim=True).round_(), fc)
        elif op == 2:
            x = _blend(x, _grey(x), fs)
        else:
            x = _hue(x, fh)
    return x.to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "color_jitter_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rgb = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (B, 3, H, W)).astype(np.uint8)).to(dev)
    res = {}

    def rec(name, ms, nbytes=None):
        res[name] = dict(device_ms=round(ms, 4))
        if nbytes is not None:
            res[name].update(bytes=nbytes, gb_per_s=round(nbytes / ms / 1e6, 1))
        print(f"{name:32s} {ms:8.4f} ms / batch" + (f"   {nbytes / ms / 1e6:8.1f} GB/s of {nbytes} bytes" if nbytes is not None else ""),
              flush=True)

    singles = {"copy": None, "brightness": dict(order=(0,), brightness=1.1), "contrast": dict(order=(1,), contrast=1.1),
               "saturation": dict(order=(2,), saturation=1.1), "hue": dict(order=(3,), hue=0.03)}
    for name, p in singles.items():
        call, nbytes, _ = kernel_call(rgb, [p] * B)
        rec("kernel:" + name, median_ms([call], args.iters)[0], nbytes)
    g = torch.Generator().manual_seed(1)
    chain = [train_data.draw_jitter_params(g) for _ in range(B)]
    call, nbytes, _ = kernel_call(rgb, chain)
    fb, fc, fs = (torch.tensor([p[k] for p in chain], dtype=torch.float32, device=dev).view(B, 1, 1, 1)
                  for k in ("brightness", "contrast", "saturation"))
    fh = torch.tensor([p["hue"] for p in chain], dtype=torch.float32, device=dev)
    orders = [p["order"] for p in chain]
    ms_kernel, ms_torch = median_ms([call, lambda: torch_chain(rgb, orders, fb, fc, fs, fh)], args.iters)
    rec("kernel:full_chain", ms_kernel, nbytes)
    rec("torch_ops:full_chain", ms_torch)
    rec("wrapper:full_chain", median_ms([lambda: train_data.color_jitter(rgb, chain)], args.iters)[0])
    rec("rgb_hsv (existing stage)", median_ms([lambda: train_data.rgb_add_noise(rgb, [dict(hsv=(1.3, 1.2))] * B, 7)], args.iters)[0])
    line = dict(bench="color_jitter", batch=B, height=H, width=W, iters=args.iters, gpu=torch.cuda.get_device_name(0),
                chain=[dict(p, order=list(p["order"])) for p in chain], results=res)
    print(json.dumps(line))
    if args.json:
        with open(args.json, "w") as fh_:
            json.dump(line, fh_, indent=1)


if __name__ == "__main__":
    main()
