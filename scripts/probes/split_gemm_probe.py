#!/usr/bin/env python3
"""Phase-removal probe of the split-bf16 GEMM form (csrc/mlp_pm_split.hip): the kernel alone on the chip, whole (variant 0) and with
one phase left out -- 1 = no split (X images get the raw upper halves: no conversions, no subtractions), 2 = no MFMAs (fragment reads
kept), 4 = no epilogue, 6 = neither MFMAs nor epilogue: the operand stream alone.  The variants give wrong results; they exist in a
build of their own (-DFFB6D_SPLIT_PROBES), the library instantiates variant 0 only.

    python scripts/probes/split_gemm_probe.py build     # hipcc -> scripts/probes/_split_probe.so (cross-compiles without a GPU)
    python scripts/probes/split_gemm_probe.py           # one JSON line per shape: microseconds per variant, median of five rounds
"""
import ctypes
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
SO = os.path.join(HERE, "_split_probe.so")

if len(sys.argv) > 1 and sys.argv[1] == "build":
    from ffb6d_amd import build
    csrc = build.CSRC
    cmd = [build.hipcc_path()] + build.FLAGS + ["-DFFB6D_SPLIT_PROBES", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                                                os.path.join(csrc, "errors.hip"), os.path.join(csrc, "mlp_pm_split.hip"), "-o", SO]
    subprocess.run(cmd, check=True)
    print(SO)
    sys.exit(0)

import torch

from ffb6d_amd import _lib

lib = ctypes.CDLL(SO)
for name in ("ffb6d_mlp_pm_split_w", "ffb6d_mlp_pm_split_f32"):
    getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
dev = torch.device("cuda:0")


def timed(fn, reps=10):
    for _ in range(2):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


for K, C, rows in ((1024, 1024, 38400), (512, 512, 38400), (256, 256, 153600)):
    x = torch.randn(rows, K, device=dev).clamp_min(0)
    w = torch.randn(C, K, device=dev) / K ** 0.5
    bias, out = torch.randn(C, device=dev), torch.empty(rows, C, device=dev)
    w3 = torch.empty(3, C, K, dtype=torch.bfloat16, device=dev)
    assert lib.ffb6d_mlp_pm_split_w(w.data_ptr(), w3.data_ptr(), w.numel(), None) == 0
    rec = {"K": K, "cout": C, "rows": rows}
    runs = {v: [] for v in (0, 1, 2, 4, 6)}
    for _ in range(5):
        for v in runs:
            def launch(v=v):
                rc = lib.ffb6d_mlp_pm_split_f32(w3.data_ptr(), bias.data_ptr(), x.data_ptr(), K, K, None, 0, None, 0, 0, None, 0, None, 0, 0,
                                                rows, out.data_ptr(), C, rows, C, 1, v, None)
                assert rc == 0
            runs[v].append(timed(launch))
    for v, t in runs.items():
        rec["variant%d_us" % v] = round(statistics.median(t), 1)
    print(json.dumps(rec), flush=True)
