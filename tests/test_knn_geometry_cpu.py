"""KNN on degenerate and tied geometry without a GPU (inputs: tests/knn_cases.py).

  * the C oracle against a float32 brute force written with np.lexsort((index, distance)): the tie rule stated a third time,
    guarding the reference the GPU tests compare with;
  * the three search kernels (csrc/knn.hip scan; csrc/knn_pruned.hip wave-per-64-queries sweep for K = 1 / 32 and 16-lane row
    kernel for 2 <= K <= 16) executed by the SIMT emulator at the smallest shapes that cross the seams: the S >= 512 routing
    threshold, a partial tile, the 16-tile level-2 box (1024 points) -- the pre-flight of tests/test_knn_geometry_gpu.py;
  * the share of rows the permutation check of the GPU file has to exclude, measured with the oracle alone."""
import os

import numpy as np
import pytest
import torch

import knn_cases
from oracle import knn as oknn

needs_clang = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"), reason="needs ROCm's clang++ to build the emulated library")


@pytest.mark.parametrize("name", ["lattice", "origin_heavy", "tiny", "offset", "identical_offset"])
def test_oracle_equals_the_numpy_lexsort_brute_force(name):
    _, sup, qry = knn_cases.build(name, 600, 100, B=2)
    want_i, want_d = knn_cases.brute_force(sup, qry, 16)
    got_i, got_d = oknn.knn_batch(sup, qry, 16, return_dist=True)
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(got_d, want_d)
    knn_cases.check_contract(sup, qry, got_i, got_d, name)


def test_the_tiny_cloud_really_is_subnormal_and_tied():
    """what the `tiny` case is there for: were the oracle built with flush-to-zero every distance would be 0"""
    _, sup, qry = knn_cases.build("tiny", 600, 100)
    _, d = oknn.knn_batch(sup, qry, 16, return_dist=True)
    assert (d < np.finfo(np.float32).tiny).all() and (d > 0).any() and (d[:, :, 0] == 0).all()
    assert (np.diff(d, axis=-1) == 0).any()


def test_two_clusters_takes_the_near_points_then_the_nearest_far_ones():
    _, sup, qry = knn_cases.build("two_clusters", 1025, 64)
    idx, d = oknn.knn_batch(sup, qry, 16, return_dist=True)
    near = np.flatnonzero(np.linalg.norm(sup[0], axis=1) < 1.0)
    assert len(near) == knn_cases.TWO_CLUSTERS_NEAR
    rows = idx[0, 0::2]                                             # the queries near the small cluster
    assert all(set(r[:10]) == set(near) and not set(r[10:]) & set(near) for r in rows)
    assert (d[0, 0::2, 10] > 2000).all()
    assert (d[0, 1::2, 0] > 50).all()                               # gap queries: nothing nearby at all


def test_lattice_rows_cut_inside_the_twelve_way_tie():
    _, sup, qry = knn_cases.build("lattice", 2048, 2048)
    assert knn_cases.lattice_dims(2048) == (16, 16, 8)
    _, d = oknn.knn_batch(sup, qry, 20, return_dist=True)
    interior = ((sup[0] >= 1) & (sup[0] <= np.array([14, 14, 6]))).all(axis=1)
    np.testing.assert_array_equal(d[0][interior][:, :19], np.tile(np.array([0] + [1] * 6 + [2] * 12, np.float32), (interior.sum(), 1)))
    assert interior.sum() > 1000


def test_permutation_check_excludes_next_to_no_rows():
    sup, qry, _ = knn_cases.permutation_cloud()
    assert len(np.unique(sup[0], axis=0)) == 3000                   # duplicate free: the self-search check relies on it
    # measured: 0 of 500 rows (0.0 %) have a tie among their 17 smallest distances
    assert knn_cases.rows_with_a_tie(sup, qry, 16).mean() <= 0.01


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels on the SIMT emulator
# ---------------------------------------------------------------------------------------------------------------------------
def _emulated(sup, qry, K, dtype=torch.int64):
    from ffb6d_amd import nearest_neighbors as nn
    i, d = nn.knn_batch_device(torch.from_numpy(sup), torch.from_numpy(qry), K, dtype=dtype, return_dist=True)
    return i.numpy(), d.numpy()


def _check(name, sup, qry, K, got_i, got_d):
    want_i, want_d = oknn.knn_batch(sup, qry, K, return_dist=True)
    tag = f"{name} S={sup.shape[1]} Q={qry.shape[1]} K={K}"
    np.testing.assert_array_equal(got_d, want_d, err_msg=tag)
    np.testing.assert_array_equal(got_i, want_i, err_msg=tag)
    knn_cases.check_contract(sup, qry, got_i, got_d, tag)


@needs_clang
@pytest.mark.parametrize("S", [512, 513, 1025])
@pytest.mark.parametrize("K", [1, 16, 32])
@pytest.mark.parametrize("name", ["identical_origin", "identical_offset", "lattice", "plane_tenth", "outside"])
def test_seam_cases_on_the_emulator(emu, name, K, S):
    _, sup, qry = knn_cases.build(name, S, 33)
    _check(name, sup, qry, K, *_emulated(sup, qry, K))


@needs_clang
@pytest.mark.parametrize("name,S,Q,K,B", [
    ("lattice", 500, 17, 16, 1),              # the scan, just under the routing threshold
    ("origin_heavy", 511, 17, 5, 2),          # ... K padded 5 -> 8, two frames
    ("origin_heavy", 1025, 33, 16, 2),        # zeros across many tiles, per-frame boxes
    ("origin_heavy", 1025, 33, 1, 1),
    ("two_clusters", 1025, 32, 16, 1),        # the 10 near points, then the bound of the far tiles decides
    ("two_clusters", 1025, 32, 1, 1),
    ("two_clusters", 513, 17, 3, 1),          # K padded 3 -> 4
    ("line_zero", 1023, 16, 15, 1),           # two zero-extent axes
    ("line_tenth", 1024, 15, 17, 1),          # K padded 17 -> 32: the wave kernel with Kout < K
    ("plane_zero", 1024, 16, 2, 1),
    ("offset", 1025, 33, 16, 1),              # quantised distances
    ("offset", 1025, 33, 31, 1),
    ("wrap_dup", 1025, 33, 8, 1),
    ("signed", 1025, 17, 16, 1),
    ("tiny", 1025, 17, 16, 1),                # subnormal distances
    ("tiny", 600, 17, 1, 1),
    ("lattice", 1025, 33, 8, 1),              # cuts inside the 6-way tie at d2 = 1
    # named regressions of the mutation study (each is the only kind of input that notices `<` for `<=` in one comparison):
    ("lattice", 2048, 257, 3, 1),             # row kernel, level-2 test: two level-2 boxes (z < 4, z >= 4) and a neighbour at d2 = 1
                                              # across their common face, whose level-2 bound EQUALS the K-th distance after the seeds
    ("line_lattice", 513, 64, 1, 1),          # wave kernel, boxbox_bound(...) <= wmax: the next tile is exactly as far from the
    ("line_lattice", 1025, 65, 1, 1),         # wave's query box as the wave's largest nearest distance
    ("line_lattice", 1025, 33, 16, 1),
    ("lattice_mid", 1025, 33, 1, 1),          # the nearest neighbour itself is a 2-, 4- or 8-way tie
    ("lattice_mid", 513, 33, 1, 2),
    ("lattice_mid", 1025, 33, 16, 1),
    # a single call is one entry in the table of a batched kernel: query block (local % gx) and frame (local / gx) both count
    ("origin_heavy", 513, 257, 1, 2),         # wave kernel, two query blocks, two frames
    ("lattice", 513, 257, 32, 2),             # wave kernel with a register list and its LDS queue, two frames
    ("lattice", 500, 257, 16, 2),             # scan, two blocks, two frames
])
def test_more_geometries_on_the_emulator(emu, name, S, Q, K, B):
    _, sup, qry = knn_cases.build(name, S, Q, B=B)
    _check(name, sup, qry, K, *_emulated(sup, qry, K, torch.int32 if B == 2 else torch.int64))


@needs_clang
def test_mixed_batch_on_the_emulator(emu):
    name, sup, qry = knn_cases.mixed_batch(1025, 17)
    for K in (1, 16):
        _check(name, sup, qry, K, *_emulated(sup, qry, K))


@needs_clang
def test_prepared_entry_points_and_a_batched_launch_on_the_emulator(emu):
    """knn_prepared with raw and with prepared queries and search_many (more searches of one kernel than one batched launch
    holds: the flush at 12) give what the single call gives"""
    from ffb6d_amd import nearest_neighbors as nn
    cases = [knn_cases.build(n, 512 + 7 * i, 5 + i, B=1, seed=i) for i, n in enumerate(
        ["lattice", "identical_offset", "origin_heavy", "outside", "plane_zero", "two_clusters", "wrap_dup", "offset", "line_tenth",
         "signed", "tiny", "uniform", "identical_origin"])]
    searches, want = [], []
    for i, (name, sup, qry) in enumerate(cases):
        s, q = torch.from_numpy(sup), torch.from_numpy(qry)
        ps, pq = nn.PreparedPoints(s), nn.PreparedPoints(q)
        one16 = nn.knn_batch_device(s, q, 16)
        one1 = nn.knn_batch_device(s, q, 1)
        assert torch.equal(nn.knn_prepared(ps, q, 16), one16), name
        assert torch.equal(nn.knn_prepared(ps, pq, 16), one16), name
        assert torch.equal(nn.knn_prepared(ps, pq, 1), one1), name
        searches += [(ps, q, 16), (ps, pq, 1)]
        want += [one16, one1]
        if i % 5 == 0:
            small = s[:, :100 + i].contiguous()
            searches.append((small, q, 16))
            want.append(nn.knn_batch_device(small, q, 16))
    for got, ref, (sup, qry, K) in zip(nn.search_many(searches), want, searches):
        assert torch.equal(got, ref), (K, tuple(ref.shape))
