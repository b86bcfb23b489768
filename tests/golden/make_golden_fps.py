"""tests/golden/make_golden_fps.py -- farthest-point-sampling goldens produced by RUNNING THE REFERENCE
(build container only; needs /root/reference and g++):  python tests/golden/make_golden_fps.py

The reference's utils/dataset_tools/fps/src/farthest_point_sampling.cpp is compiled (g++ -O2, as its cffi build does) into a
TEMPORARY directory and called through ctypes; neither its source nor anything compiled from it is kept.  fps_ref.npz holds,
for every case i of CASES (data only):
  pts{i}   f32 [n,3]   the input set (tests/fps_ref.py KINDS[kind](n, seed), stored so that the fixture stands on its own)
  ctr{i}   i16 [m]     farthest_point_sampling_init_center's index sequence
  rnd{i}   i16 [m]     farthest_point_sampling's index sequence; its first index comes from srand(time(0)), rand() % n: it is
                       the `start` to replay the sequence with
  kind, n, m           the case table
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fps_ref  # noqa: E402

REF_SRC = "/root/reference/ffb6d/utils/dataset_tools/fps/src/farthest_point_sampling.cpp"
OUT = os.path.join(HERE, "fps_ref.npz")

# (kind, n, m, seed): every n of {1, 5, 64, 65, 300, 1000, 5000}, every kind, m up to 2048 and m > n
CASES = [("random", 1, 4, 701), ("random", 5, 8, 702), ("lattice", 64, 8, 703), ("lattice", 65, 80, 704),
         ("duplicate", 64, 40, 705), ("duplicate", 65, 8, 706), ("identical", 5, 3, 707), ("identical", 300, 8, 708),
         ("random", 300, 8, 709), ("lattice", 300, 300, 710), ("random", 1000, 2048, 711), ("duplicate", 1000, 600, 712),
         ("random", 5000, 2048, 713), ("lattice", 5000, 64, 714)]


def main():
    out = {"kind": np.array([c[0] for c in CASES]), "n": np.array([c[1] for c in CASES], np.int32),
           "m": np.array([c[2] for c in CASES], np.int32)}
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libfps.so")
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-w", REF_SRC, "-o", so], check=True)
        lib = ctypes.CDLL(so)
        for i, (kind, n, m, seed) in enumerate(CASES):
            pts = fps_ref.KINDS[kind](n, seed)
            out[f"pts{i}"] = pts
            for key, fn in (("ctr", lib.farthest_point_sampling_init_center), ("rnd", lib.farthest_point_sampling)):
                idx = np.full(m, -1, np.int32)
                fn(ctypes.c_void_p(pts.ctypes.data), ctypes.c_void_p(idx.ctypes.data), ctypes.c_int(n), ctypes.c_int(m))
                assert idx.min() >= 0 and idx.max() < n
                out[f"{key}{i}"] = idx.astype(np.int16)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
