#!/usr/bin/env python3
"""The long-row fp32 GEMM launches of the benchmark step, each alone on the chip: the tile-sequence form (automatic choice) against the
split-bf16 form (tile_hint 10, csrc/mlp_pm_split.hip).

  layers [reps]   one JSON line per layer: microseconds per launch of both forms (median of five alternating rounds, with min and max),
                  fp32-equivalent TFLOP/s and the share of the 157.3 TFLOP/s fp32 MFMA peak   -> profiles/split_gemm_layers.jsonl
  accuracy        one JSON object: per layer shape (K and Cout of the network, 512 rows) the error of both forms against float64 in units
                  of the output range, their ratio, the distance of the device's bits from the CPU restatement (tests/split_gemm_ref.py)
                  in ulps, and the restatement's own error over three seeds                 -> profiles/split_gemm_accuracy.json
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

from ffb6d_amd import ops, ops_pm

PEAK_TFLOPS = 157.3
dev = torch.device("cuda:0")
# the 8 x 60 x 80 trunk map of the benchmark: F(4x4) makes 36 matrices of Tp = 2432 rows
WINO = [(256, 256, 7), (256, 512, 1), (512, 512, 9)]                  # (K, Cout, launches per step)
# (K, Cout, B, P, epilogue, rows of Y per frame, name): the single-source long-row launches (the heads' first layer has two sources)
LONG = [(1024, 2304, 8, 4800, None, 0, "z-GEMM 60x80"), (1024, 1024, 8, 4800, "gather", 48, "p2r ds3"),
        (256, 576, 8, 19200, None, 0, "z-GEMM 120x160"), (512, 1024, 8, 4800, "add", 0, "psp bottleneck"),
        (512, 512, 8, 4800, "gather", 192, "p2r ds2"), (256, 256, 8, 19200, "gather", 192, "p2r up0")]


def timed(fn, reps):
    for _ in range(2):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def ab(old, new, reps):
    runs = {"seq": [], "split": []}
    for _ in range(5):
        runs["seq"].append(timed(old, reps))
        runs["split"].append(timed(new, reps))
    return {k: (round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)) for k, v in runs.items()}


def long_case(K, C, B, P, epi, py, gen_seed=0):
    g = torch.Generator(device=dev).manual_seed(gen_seed)
    x = torch.randn(B, P, K, device=dev, generator=g).clamp_min(0)
    w = torch.randn(C, K, device=dev, generator=g) / K ** 0.5
    bias = torch.randn(C, device=dev, generator=g)
    kw = {}
    if epi == "add":
        kw["add"] = torch.randn(B, P, C, device=dev, generator=g)
    elif epi == "gather":
        kw["gather"] = (torch.randn(B, py, C, device=dev, generator=g), torch.randint(0, py, (B, P), device=dev, generator=g, dtype=torch.int32))
    return x, w, bias, kw


def layers(reps):
    for K, C, n in WINO:
        G, R = 36, 2432
        v, u = torch.randn(G, R, K, device=dev), torch.randn(G, C, K, device=dev) / K ** 0.5
        u3, m = ops_pm.split_weight(u), torch.empty(G, R, C, device=dev)
        t = ab(lambda: ops_pm.mlp_batched(v, u, out=m), lambda: ops_pm.mlp_batched(v, u, out=m, tile_hint=10, w_split=u3), reps)
        flop = 2.0 * G * R * K * C
        emit("wino4 %d->%d" % (K, C), K, C, G * R, n, t, flop)
    for K, C, B, P, epi, py, name in LONG:
        x, w, bias, kw = long_case(K, C, B, P, epi, py)
        w3, out = ops_pm.split_weight(w), torch.empty(B, P, C, device=dev)
        t = ab(lambda: ops_pm.mlp(x, w, bias, ops.ACT_RELU, out=out, **kw),
               lambda: ops_pm.mlp(x, w, bias, ops.ACT_RELU, out=out, tile_hint=10, w_split=w3, **kw), reps)
        emit(name, K, C, B * P, 1, t, 2.0 * B * P * K * C)


def emit(name, K, C, rows, n, t, flop):
    rec = {"layer": name, "K": K, "cout": C, "rows": rows, "launches_per_step": n,
           "seq_us_med_min_max": t["seq"], "split_us_med_min_max": t["split"],
           "seq_tflops": round(flop / t["seq"][0] * 1e-6, 1), "split_tflops": round(flop / t["split"][0] * 1e-6, 1),
           "split_frac_of_fp32_mfma_peak": round(flop / t["split"][0] * 1e-6 / PEAK_TFLOPS, 3),
           "speedup": round(t["seq"][0] / t["split"][0], 3)}
    print(json.dumps(rec), flush=True)


def accuracy():
    import split_gemm_ref as ref
    out = {"rows": 512, "bar": "1e-5 of the output range (tests/test_pm_forms_gpu.py::_check)", "layers": []}
    shapes = [(K, C, None, 0, "wino4 %d->%d" % (K, C)) for K, C, _ in WINO] + [(K, C, epi, py, name) for K, C, _, _, epi, py, name in LONG]
    for K, C, epi, py, name in shapes:
        x, w, bias, kw = long_case(K, C, 1, 512, epi, py or 1, gen_seed=K + C)
        if name.startswith("wino4"):
            bias, act = None, ops.ACT_NONE
        else:
            act = ops.ACT_NONE                        # the bare product + epilogue rows: an activation only hides error
        want = x[0].double() @ w.double().T
        if bias is not None:
            want = want + bias.double()
        if "add" in kw:
            want = want + kw["add"][0].double()
        if "gather" in kw:
            want = want + kw["gather"][0][0].double()[kw["gather"][1][0].long()]
        rng = float(want.abs().max())
        seq = ops_pm.mlp(x, w, bias, act, **kw)[0]
        new = ops_pm.mlp(x, w, bias, act, tile_hint=10, **kw)[0]
        e_seq, e_new = float((seq.double() - want).abs().max()) / rng, float((new.double() - want).abs().max()) / rng
        # the CPU restatement on the same operands (bits) and on two more seeds (its spread)
        acc = ref.gemm(x[0].cpu(), w.cpu())
        extra = kw["add"][0].cpu() if "add" in kw else (kw["gather"][0][0].cpu()[kw["gather"][1][0].long().cpu()] if "gather" in kw else None)
        rest = ref.epilogue(acc, None if bias is None else bias.cpu(), extra, 0)
        e_rest = [float((rest.double() - want.cpu()).abs().max()) / rng]
        for seed in (1, 2):
            g = torch.Generator().manual_seed(seed)
            xs, ws = torch.randn(128, K, generator=g).clamp_min(0), torch.randn(C, K, generator=g) / K ** 0.5
            ws64 = xs.double() @ ws.double().T
            e_rest.append(float((ref.gemm(xs, ws).double() - ws64).abs().max()) / float(ws64.abs().max()))
        out["layers"].append({"layer": name, "K": K, "cout": C, "err_new_over_range": e_new, "err_seq_over_range": e_seq,
                              "ratio_new_to_seq": e_new / e_seq, "err_restatement_over_range_3_seeds": e_rest,
                              "predicted_ratio": e_rest[0] / e_seq, "ratio_over_predicted": e_new / e_rest[0],
                              "ulps_device_vs_restatement": ref.ulps(new.cpu().contiguous(), rest.contiguous()),
                              "routable_by_accuracy": e_new <= 2.0 * e_rest[0] and e_new <= 1e-5})
    print(json.dumps(out, indent=1), flush=True)


if __name__ == "__main__":
    with torch.no_grad():
        if len(sys.argv) > 1 and sys.argv[1] == "accuracy":
            accuracy()
        else:
            layers(int(sys.argv[2]) if len(sys.argv) > 2 else 10)
