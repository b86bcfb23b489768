"""tests/golden/make_golden_ms_multi.py -- goldens of MeanShiftTorch.fit_multi_clus produced by RUNNING THE REFERENCE
(only where the reference checkout that oracle/ref_harness.py looks for exists):  python tests/golden/make_golden_ms_multi.py

ms_multi.npz holds, for seeded mixtures of Gaussians (with and without uniform outliers), the outputs of the unmodified
reference's MeanShiftTorch(bandwidth).fit_multi_clus (ffb6d/utils/meanshift_pytorch.py:60-85):
  c{i}_centres f32 [k,3] / c{i}_labels i32 [M] / c{i}_n_in i64 [k] / c{i}_n_cmp (how many leading clusters a test compares)
The inputs are regenerated from the seed by the tests (only outputs are stored).

Asserted per case, so that the comparison is sharp (a case that fails is replaced, not tolerated):
  * no pairwise distance of the reference's converged points lies within 5 % of the bandwidth of the bandwidth itself
    (5 % of 0.04 m = 2 mm = 4 x the 5e-4 m the centres may differ by; each endpoint may move by that much) -- the tests then
    need no allowance for labels that flip;
  * the compared clusters (the first n_cmp) have pairwise different sizes, each larger than every later one: the order of
    equal-sized clusters depends on the tie behaviour of torch.max, which the reference does not define.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

# (seed, blob sizes, uniform outliers, bandwidth)
CASES = [(1, (3, 2), 0, 0.04), (2, (300, 200, 100), 0, 0.04), (3, (300, 200, 100), 12, 0.05), (4, (600, 130, 60), 20, 0.05),
         (5, (40, 25), 0, 0.04), (6, (33, 20, 11), 0, 0.05), (7, (120, 70, 45, 20), 6, 0.04)]


def mixture(seed, sizes, outliers):
    """f32 [sum(sizes) + outliers, 3]: Gaussian blobs (sigma 1 cm) around centres 0.3 m apart, uniform outliers, shuffled"""
    rng = np.random.RandomState(seed)
    parts = [0.01 * rng.randn(n, 3) + [0.3 * k - 0.3, 0.1 * rng.randn(), 1.0] for k, n in enumerate(sizes)]
    if outliers:
        parts.append(rng.uniform(-1, 1, (outliers, 3)) * [0.8, 0.5, 0.4] + [0.0, 0.0, 1.0])
    a = np.concatenate(parts).astype(np.float32)
    return a[rng.permutation(len(a))]


def compared(n_in):
    """number of leading clusters with pairwise different sizes, each larger than every later one"""
    n = 0
    while n < len(n_in) and all(n_in[n] > v for v in n_in[n + 1:]):
        n += 1
    return n


def main():
    from oracle import ref_harness as rh
    ms_mod, _ = rh.reference_pose_modules()
    out = {}
    for i, (seed, sizes, outliers, bw) in enumerate(CASES):
        v = torch.from_numpy(mixture(seed, sizes, outliers))
        ms = ms_mod.MeanShiftTorch(bandwidth=bw)
        centres, labels, n_in = ms.fit_multi_clus(v)
        C, _ = ms.fit(v, ret_mid_res=True)
        d = torch.norm(C[None].double() - C[:, None].double(), dim=2).numpy()
        assert not ((d > 0.95 * bw) & (d < 1.05 * bw)).any(), (i, "a converged pair at the bandwidth")
        n_cmp = compared(n_in)
        assert n_cmp >= min(len(sizes), 2), (i, n_in)
        assert int(labels.min()) >= 1 and int(labels.max()) == len(n_in)
        out[f"c{i}_centres"] = torch.stack(centres).numpy()
        out[f"c{i}_labels"] = labels.numpy().astype(np.int32)
        out[f"c{i}_n_in"] = np.asarray(n_in, np.int64)
        out[f"c{i}_n_cmp"] = np.int64(n_cmp)
        print(i, "points", len(v), "clusters", len(n_in), "sizes", n_in[:8], "compared", n_cmp)
    path = os.path.join(HERE, "ms_multi.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
