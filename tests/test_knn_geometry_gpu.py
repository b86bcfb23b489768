"""The three KNN search kernels (csrc/knn.hip scan; csrc/knn_pruned.hip wave-per-64-queries sweep for K = 1 / 32 and 16-lane row
kernel for 2 <= K <= 16) on degenerate and tied geometry (tests/knn_cases.py), at the shapes next to every seam:

    S   500 511 | 512 513 (routing threshold of ffb6d_knn_uses_pruning), 1023 1024 1025 (16 tiles = one level-2 box), 2048 2049
    K   1 | 2 3 5 8 15 16 | 17 31 32 (kernel per range; padded K 3->4, 5->8, 15->16, 17->32 with Kout < K)
    Q   1, 15 16 17 (queries per row block), 63 64 65 (wave), 255 256 257 (block of the wave kernel)

(a) indices AND distances bit for bit against the C oracle, (e) the contract asserted on the output itself in plain numpy
(knn_cases.check_contract), (b) every entry point equals knn_batch_device, (c) more searches than one batched launch holds,
(d) metamorphic checks that need no oracle.  Bar: bit-exact (BASELINE.json north_star)."""
import numpy as np
import pytest
import torch

import knn_cases
from ffb6d_amd import nearest_neighbors as nn
from oracle import knn as oknn

pytestmark = pytest.mark.gpu

S_SWEEP = (500, 511, 512, 513, 1023, 1024, 1025, 2048, 2049)
K_SWEEP = (1, 2, 3, 5, 8, 15, 16, 17, 31, 32)
Q_SWEEP = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257)
SWEPT = ("lattice", "origin_heavy", "two_clusters")


def _cases():
    c = []
    for g in knn_cases.GEOMETRIES:
        c += [(g, 2049, 257, 16, 1, torch.int64), (g, 1025, 65, 1, 1, torch.int64)]
        c += [(g, 1025, 65, 32, 1, torch.int32)]              # the other index dtype, the wave kernel with a register list
        c += [(g, 1023, 63, 16, 2, torch.int32)]              # two frames from different seeds
    for g in SWEPT:
        c += [(g, S, 65, K, 1, torch.int64) for S in S_SWEEP for K in (1, 16, 32)]
        c += [(g, S, 65, K, 1, torch.int64) for S in (500, 1025) for K in K_SWEEP]
        c += [(g, 1025, Q, K, 1, torch.int64) for Q in Q_SWEEP for K in (1, 16, 32)]
        c += [(g, 500, Q, 16, 1, torch.int64) for Q in (1, 255, 256, 257)]
        c += [(g, 2048, 257, K, 1, torch.int64) for K in K_SWEEP]      # two level-2 boxes
        c += [(g, 2049, 257, K, 2, torch.int64) for K in (1, 5, 32)]
    c += [("origin_heavy", 5000, 2000, K, 1, torch.int64) for K in (1, 16, 32)]      # the largest case
    c += [("lattice", 4096, 2000, 16, 1, torch.int64)]
    c += [("line_lattice", S, Q, 1, 1, torch.int64) for S in (513, 1025) for Q in (64, 257)]      # see tests/test_knn_geometry_cpu.py
    c += [("origin_heavy", 500, 1025, 1, 2, torch.int64)]     # scan with 4 queries per lane: two blocks, two frames in one flattened grid
    c += [("lattice", 500, 257, 32, 2, torch.int32)]
    seen, out = set(), []
    for x in c:
        if x[:5] not in seen:
            seen.add(x[:5])
            out.append(x)
    return out


def _run(device, sup, qry, K, dtype=torch.int64):
    i, d = nn.knn_batch_device(torch.from_numpy(sup).to(device), torch.from_numpy(qry).to(device), K, dtype=dtype, return_dist=True)
    assert i.dtype == dtype
    return i.cpu().numpy(), d.cpu().numpy()


def _check(tag, sup, qry, K, got_i, got_d):
    want_i, want_d = oknn.knn_batch(sup, qry, K, return_dist=True)
    np.testing.assert_array_equal(got_d, want_d, err_msg=tag)
    np.testing.assert_array_equal(got_i, want_i, err_msg=tag)
    knn_cases.check_contract(sup, qry, got_i, got_d, tag)


@pytest.mark.parametrize("name,S,Q,K,B,dtype", _cases(), ids=lambda v: str(v).replace("torch.", ""))
def test_geometry_matches_the_oracle_and_the_contract(device, name, S, Q, K, B, dtype):
    _, sup, qry = knn_cases.build(name, S, Q, B=B)
    _check(f"{name} S={S} Q={Q} K={K} B={B}", sup, qry, K, *_run(device, sup, qry, K, dtype))


@pytest.mark.parametrize("S,Q,K", [(2049, 257, 16), (1025, 65, 1), (1024, 64, 32), (500, 17, 16), (513, 16, 3)])
def test_mixed_batch_has_per_frame_boxes_keys_and_strides(device, S, Q, K):
    name, sup, qry = knn_cases.mixed_batch(S, Q)
    _check(f"{name} S={S} Q={Q} K={K}", sup, qry, K, *_run(device, sup, qry, K))
    assert (_run(device, sup, qry, K)[0][0] == np.arange(K)).all()               # the `identical` frame: 0..K-1 everywhere


@pytest.mark.parametrize("name", ["identical_origin", "identical_offset"])
@pytest.mark.parametrize("K", [1, 16, 32])
def test_identical_points_give_the_first_k_indices_at_distance_zero(device, name, K):
    _, sup, qry = knn_cases.build(name, 2049, 257)
    got_i, got_d = _run(device, sup, qry, K)
    assert (got_i == np.arange(K)).all() and (got_d == 0).all()


# (b) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice", "identical_origin", "identical_offset", "origin_heavy", "outside"])
def test_every_entry_point_equals_the_single_call(device, name):
    _, sup, qry = knn_cases.build(name, 2049, 257, B=2)
    s, q = torch.from_numpy(sup).to(device), torch.from_numpy(qry).to(device)
    ps, pq = nn.PreparedPoints(s), nn.PreparedPoints(q)
    one = {K: nn.knn_batch_device(s, q, K, return_dist=True) for K in (1, 2, 16, 32)}
    for K in (2, 16):                                                             # raw queries
        i, d = nn.knn_prepared(ps, q, K, return_dist=True)
        assert torch.equal(i, one[K][0]) and torch.equal(d, one[K][1]), (name, K)
    for K in (1, 16, 32):                                                         # prepared queries
        i, d = nn.knn_prepared(ps, pq, K, return_dist=True)
        assert torch.equal(i, one[K][0]) and torch.equal(d, one[K][1]), (name, K)
        assert torch.equal(nn.knn_prepared(ps, pq, K, dtype=torch.int32), one[K][0].int()), (name, K)
    small = s[:, :500].contiguous()
    searches = [(ps, q, 2), (ps, q, 16), (ps, pq, 16), (ps, pq, 1), (small, q, 16), (small, q, 1)]
    want = [one[2][0], one[16][0], one[16][0], one[1][0], nn.knn_batch_device(small, q, 16), nn.knn_batch_device(small, q, 1)]
    for dt in (torch.int64, torch.int32):
        for got, ref, (_, _, K) in zip(nn.search_many(searches, dtype=dt), want, searches):
            assert got.dtype == dt and torch.equal(got, ref.to(dt)), (name, K, dt)


def test_more_than_256_segments_sort_on_64_bit_keys(device):
    """257 frames: a prepare with more than 256 (set, frame) segments carries the segment number above bit 32 of the sort key
    and sorts with rocPRIM instead of the segmented 32-bit sort -- single calls and sets prepared together alike"""
    _, sup, qry = knn_cases.build("two_clusters", 513, 17, B=257)
    s, q = torch.from_numpy(sup).to(device), torch.from_numpy(qry).to(device)
    for K in (1, 16):
        _check(f"two_clusters S=513 Q=17 K={K} B=257", sup, qry, K, *_run(device, sup, qry, K))
    for m, p in zip(nn.prepare_many([s, q]), (s, q)):
        one = nn.PreparedPoints(p)
        assert m.S == one.S and torch.equal(m.blob[:-256], one.blob[:-256])     # (the last < 256 bytes are alignment padding)


# (c) ------------------------------------------------------------------------------------------------------------------------
def test_more_searches_than_one_batched_launch_holds(device):
    """13 pruned K = 16, 13 pruned K = 1 and 3 scan searches, interleaved, in ONE search_many call: the row kernel and the K = 1
    kernel each flush a full table of MAX_SEARCHES = 12 (find_search with every slot in use) and launch once more for the 13th"""
    names = [n for n in knn_cases.GEOMETRIES if n not in ("uniform", "identical_origin", "plane_zero", "line_zero")]
    assert len(names) == 13
    searches, want = [], []
    for i, n in enumerate(names):
        S, Q = 512 + 61 * i, 16 * i + 1 + i % 3                                   # distinct, on and off the tile and row-block edges
        _, sup, qry = knn_cases.build(n, S, Q, B=2, seed=10 + i)
        s, q = torch.from_numpy(sup).to(device), torch.from_numpy(qry).to(device)
        ps, pq = nn.PreparedPoints(s), nn.PreparedPoints(q)
        searches += [(ps, q if i % 2 else pq, 16), (ps, pq, 1)]
        want += [nn.knn_batch_device(s, q, 16), nn.knn_batch_device(s, q, 1)]
        if i % 5 == 0:
            small = s[:, :300 + 100 * (i // 5) + i].contiguous()                  # 300, 405, 510 points: the scan
            searches.append((small, q, 16))
            want.append(nn.knn_batch_device(small, q, 16))
    assert sum(1 for s in searches if s[2] == 1) == 13 and len(searches) == 29
    for n, (got, ref) in enumerate(zip(nn.search_many(searches), want)):
        assert torch.equal(got, ref), (n, tuple(ref.shape))


# (d) ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clouds():
    sup, qry, perm = knn_cases.permutation_cloud()
    _, lsup, lqry = knn_cases.build("lattice", 2048, 500)
    return {"uniform": (sup, qry, perm), "lattice": (lsup, lqry, np.random.RandomState(6).permutation(2048))}


@pytest.mark.parametrize("name", ["uniform", "lattice"])
@pytest.mark.parametrize("e", [-30, 40])
def test_scaling_by_a_power_of_two_changes_nothing_but_the_scale(device, clouds, name, e):
    """all coordinate differences are multiples of 2^-23 below 2^5, so the scaled arithmetic is the unscaled one with another
    exponent: same indices, distances times exactly 2^(2e) (nothing under- or overflows: 2^-106 <= d2 * 2^-60, d2 * 2^80 < 2^91)"""
    sup, qry, _ = clouds[name]
    f = np.float32(2.0 ** e)
    base_i, base_d = _run(device, sup, qry, 16)
    got_i, got_d = _run(device, sup * f, qry * f, 16)
    np.testing.assert_array_equal(got_i, base_i)
    np.testing.assert_array_equal(got_d, base_d * f * f)


@pytest.mark.parametrize("name", ["uniform", "lattice"])
def test_permuting_the_support_maps_the_indices_through_the_permutation(device, clouds, name):
    sup, qry, perm = clouds[name]
    base_i, base_d = _run(device, sup, qry, 16)
    got_i, got_d = _run(device, np.ascontiguousarray(sup[:, perm]), qry, 16)       # new point j is old point perm[j]
    np.testing.assert_array_equal(got_d, base_d)
    if name == "lattice":
        # Ties everywhere, and K = 16 cuts inside a 12-way tie: WHICH members of the cut run win depends on the index order, so
        # the mapped rows are compared in canonical tie order (oracle.knn.canonical_ties on both sides) up to the cut run -- every
        # entry nearer than the row's last distance -- and the cut run by its distances (equal above) and by the contract, which
        # each result has to meet for its own index order.
        mapped, _ = oknn.canonical_ties(perm[got_i[0]], sup[0], qry[0])
        base, ties = oknn.canonical_ties(base_i[0], sup[0], qry[0])
        complete = base_d[0] < base_d[0][:, -1:]
        assert ties > 400 and complete.sum() > 7 * 400
        np.testing.assert_array_equal(mapped[complete], base[complete])
        knn_cases.check_contract(np.ascontiguousarray(sup[:, perm]), qry, got_i, got_d, "lattice permuted")
        knn_cases.check_contract(sup, qry, base_i, base_d, "lattice")
        return
    tied = knn_cases.rows_with_a_tie(sup, qry, 16)
    # measured with the oracle (tests/test_knn_geometry_cpu.py): 0 of 500 rows (0.0 %) are excluded
    assert tied.mean() <= 0.01
    np.testing.assert_array_equal(perm[got_i][~tied], base_i[~tied])


@pytest.mark.parametrize("name", ["uniform", "lattice"])
def test_permuting_the_queries_permutes_the_rows(device, clouds, name):
    sup, qry, _ = clouds[name]
    qperm = np.random.RandomState(8).permutation(qry.shape[1])
    for K in (1, 16, 32):
        base_i, base_d = _run(device, sup, qry, K)
        got_i, got_d = _run(device, sup, np.ascontiguousarray(qry[:, qperm]), K)
        np.testing.assert_array_equal(got_i, base_i[:, qperm])
        np.testing.assert_array_equal(got_d, base_d[:, qperm])


@pytest.mark.parametrize("K", [1, 16, 32])
def test_self_search_of_a_duplicate_free_cloud_starts_with_the_point_itself(device, clouds, K):
    sup = clouds["uniform"][0]
    assert len(np.unique(sup[0], axis=0)) == sup.shape[1]
    s = torch.from_numpy(sup).to(device)
    i, d = nn.knn_batch_device(s, s, K, return_dist=True)                          # one tensor on both sides: one prepare
    assert (i[:, :, 0].cpu().numpy() == np.arange(sup.shape[1])).all() and (d[:, :, 0] == 0).all()
    i2, d2 = nn.knn_batch_device(s, s.clone(), K, return_dist=True)
    assert torch.equal(i, i2) and torch.equal(d, d2)
