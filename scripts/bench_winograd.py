#!/usr/bin/env python3
"""One wide trunk convolution (3x3, stride 1, BatchNorm + residual + ReLU) alone on the chip, direct against Winograd F(2x2,3x3) and
F(4x4,3x3): MIOpen + affine_act_ against input transform -> batched GEMM -> output transform (forward_pm.conv_wino, m = 2 / 4), each
stage timed by itself with device events.  Prints one JSON line per width: microseconds per launch, the GEMMs' TFLOP/s and their share
of the fp32 MFMA peak (the F(4x4) GEMM also under every plan its tile_hint reaches), each transform's GB/s by algorithmic bytes.
argv: [B H W] (default 8 60 80: the trunk map of the benchmark) [reps]

argv: narrow [reps] -- the narrow trunk layers instead, (8,120,160,64->64), (8,60,80,128->128) and (8,60,80,128->256): MIOpen's convolution +
affine_act_ with the pinned find-db as bench.py uses it (device events around the pair, so MIOpen's zero-fill is inside), the unfused F(4x4)
path where the batched GEMM accepts the shape, and the fused kernel (csrc/winograd_fused.h) in its three workgroup shapes (median of five
rounds over the forms, with the smallest and largest) and in the automatic per-width choice; TFLOP/s of the fused kernel by the Winograd
multiplies, GB/s by x + residual + out.  One JSON line per shape (profiles/winograd_narrow_layers.jsonl, winograd_narrow2_layers.jsonl)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from ffb6d_amd import forward_pm, ops, ops_pm

PEAK_TFLOPS = 157.3        # fp32 MFMA, MI355X
dev = torch.device("cuda:0")
NARROW = len(sys.argv) > 1 and sys.argv[1] == "narrow"
if NARROW:
    from ffb6d_amd import miopen_pin
    MIOPEN_DB = miopen_pin.use(only_solver=miopen_pin.FWD_SOLVER)
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
else:
    B, H, W = (int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (8, 60, 80)
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
torch.manual_seed(0)


def timed(fn):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def narrow():
    for B, H, W, cin, cout in ((8, 120, 160, 64, 64), (8, 60, 80, 128, 128), (8, 60, 80, 128, 256)):
        conv = torch.nn.Conv2d(cin, cout, 3, 1, 1, bias=False).to(dev)
        x, res = torch.randn(B, H, W, cin, device=dev), torch.randn(B, H, W, cout, device=dev)
        scale, shift = torch.rand(cout, device=dev) + .5, torch.randn(cout, device=dev)
        u4 = forward_pm.wino4_weights(conv)
        out = torch.empty(B, H, W, cout, device=dev)
        px, T4 = B * H * W, ops_pm.wino4_tiles(B, H, W)[0]
        rec = {"shape": [B, H, W, cin, cout], "tiles4": T4, "miopen": MIOPEN_DB,
               "direct_conv_us": timed(lambda: forward_pm.conv(x, conv)),
               "direct_conv_affine_us": timed(lambda: ops_pm.affine_act_(forward_pm.conv(x, conv), scale, shift, act=ops.ACT_RELU, residual=res))}
        if forward_pm.wino_ok(conv, x, m=4) or (cin >= 128 and cin % 32 == 0):
            rec["wino4_unfused_total_us"] = timed(lambda: forward_pm.conv_wino(x, conv, scale, shift, residual=res, m=4))
        runs = {form: [] for form in (1, 2, 3)}
        for _ in range(5):                                 # the forms in turn, five times: median, and the spread a choice has to beat
            for form in runs:
                runs[form].append(timed(lambda: ops_pm.wino4_conv(x, u4, scale, shift, act=ops.ACT_RELU, residual=res, out=out, form=form)))
        for form, t in runs.items():
            rec["fused_form%d_us" % form] = sorted(t)[2]
            rec["fused_form%d_min_max_us" % form] = [round(min(t), 3), round(max(t), 3)]
        rec["auto_form"] = ops_pm.wino4_conv_form(cin, cout)
        rec["fused_us"] = timed(lambda: ops_pm.wino4_conv(x, u4, scale, shift, act=ops.ACT_RELU, residual=res, out=out))
        rec["fused_tflops"] = 2.0 * 36 * T4 * cin * cout / rec["fused_us"] * 1e-6
        rec["fused_frac_of_fp32_mfma_peak"] = rec["fused_tflops"] / PEAK_TFLOPS
        rec["fused_GBps"] = 4.0 * px * (cin + 2 * cout) / rec["fused_us"] * 1e-3
        rec["direct_conv_tflops"] = 2.0 * 9 * px * cin * cout / rec["direct_conv_us"] * 1e-6
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)


with torch.no_grad():
    if NARROW:
        narrow()
    for cin, cout in () if NARROW else ((256, 256), (256, 512), (512, 512)):
        conv = torch.nn.Conv2d(cin, cout, 3, 1, 1, bias=False).to(dev)
        x, res = torch.randn(B, H, W, cin, device=dev), torch.randn(B, H, W, cout, device=dev)
        scale, shift = torch.rand(cout, device=dev) + .5, torch.randn(cout, device=dev)
        T, Tp = ops_pm.wino_tiles(B, H, W)
        u = forward_pm.wino_weights(conv)
        v, m = ops_pm.wino_input(x), torch.empty(16, Tp, cout, device=dev)
        ops_pm.mlp_batched(v, u, out=m)
        rec = {"shape": [B, H, W, cin, cout], "tiles": T,
               "direct_conv_us": timed(lambda: forward_pm.conv(x, conv)),
               "direct_conv_affine_us": timed(lambda: ops_pm.affine_act_(forward_pm.conv(x, conv), scale, shift, act=ops.ACT_RELU, residual=res)),
               "wino_total_us": timed(lambda: forward_pm.conv_wino(x, conv, scale, shift, residual=res, m=2)),
               "wino_input_us": timed(lambda: ops_pm.wino_input(x, out=v)),
               "wino_gemm_us": timed(lambda: ops_pm.mlp_batched(v, u, out=m)),
               "wino_gemm_lds_form_us": timed(lambda: ops_pm.mlp_batched(v, u, out=m, tile_hint=7)),
               "wino_output_us": timed(lambda: ops_pm.wino_output(m, (B, H, W), scale, shift, act=ops.ACT_RELU, residual=res))}
        px = B * H * W
        rec["wino_gemm_tflops"] = 2.0 * 16 * T * cin * cout / rec["wino_gemm_us"] * 1e-6
        rec["wino_gemm_frac_of_fp32_mfma_peak"] = rec["wino_gemm_tflops"] / PEAK_TFLOPS
        rec["wino_input_GBps"] = 4.0 * (px * cin + 16 * T * cin) / rec["wino_input_us"] * 1e-3
        rec["wino_output_GBps"] = 4.0 * (16 * T * cout + 2 * px * cout) / rec["wino_output_us"] * 1e-3
        T4, Tp4 = ops_pm.wino4_tiles(B, H, W)
        u4 = forward_pm.wino4_weights(conv)
        v4, m4 = ops_pm.wino4_input(x), torch.empty(36, Tp4, cout, device=dev)
        ops_pm.mlp_batched(v4, u4, out=m4)
        rec.update({"tiles4": T4, "variant": forward_pm.wino_variant(B, H, W),
                    "wino4_total_us": timed(lambda: forward_pm.conv_wino(x, conv, scale, shift, residual=res, m=4)),
                    "wino4_input_us": timed(lambda: ops_pm.wino4_input(x, out=v4)),
                    "wino4_gemm_us": timed(lambda: ops_pm.mlp_batched(v4, u4, out=m4)),
                    "wino4_gemm_lds_form_us": timed(lambda: ops_pm.mlp_batched(v4, u4, out=m4, tile_hint=7)),
                    "wino4_output_us": timed(lambda: ops_pm.wino4_output(m4, (B, H, W), scale, shift, act=ops.ACT_RELU, residual=res))})
        for plan in (1, 2, 4):                         # whole-point-tile plans: sequences of `plan` channel tiles (cout / 128 of them)
            if plan * 128 <= cout:
                rec["wino4_gemm_plan%d_us" % plan] = timed(lambda: ops_pm.mlp_batched(v4, u4, out=m4, tile_hint=8 + 256 * plan))
        rec["wino4_gemm_tflops"] = 2.0 * 36 * T4 * cin * cout / rec["wino4_gemm_us"] * 1e-6
        rec["wino4_gemm_frac_of_fp32_mfma_peak"] = rec["wino4_gemm_tflops"] / PEAK_TFLOPS
        rec["wino4_input_GBps"] = 4.0 * (px * cin + 36 * T4 * cin) / rec["wino4_input_us"] * 1e-3
        rec["wino4_output_GBps"] = 4.0 * (36 * T4 * cout + 2 * px * cout) / rec["wino4_output_us"] * 1e-3
        rec["direct_conv_tflops"] = 2.0 * 9 * px * cin * cout / rec["direct_conv_us"] * 1e-6
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)
