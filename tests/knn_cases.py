"""Deterministic point-set builders for the KNN geometry tests (tests/test_knn_geometry_gpu.py, test_knn_geometry_cpu.py) and a
plain-numpy statement of the KNN contract.  No tests live here.

Uniform random clouds in [0,1)^3 are the one input on which a spatial-pruning bug stays invisible: no exact distance ties, a box
with three non-zero extents, distinct Morton keys, no query outside the support's box.  Real FFB6D input is the opposite: a
regular pixel grid, thousands of invalid pixels at (0,0,0), clouds wrap-padded with exact duplicates (linemod_dataset.py:198,
276-277), near-planar patches, metres or millimetres.  The builders below are those inputs in small:

    build(name, S, Q, B=1, seed=0) -> (name, support float32 [B,S,3], query float32 [B,Q,3])      name in GEOMETRIES
    mixed_batch(S, Q, seed=0)      -> ("mixed_batch", support [3,S,3], query [3,Q,3])

Frame b of a batch is built from seed + b, so the frames of a batch differ.  Every builder puts its points in an order that is
unrelated to their position (a seeded shuffle where the construction has a spatial order of its own), so that the lowest-index
tie rule has to hold across tiles of the Morton-ordered search; `wrap_dup` is the exception, its index order IS its structure.

Scope: all coordinates are finite with |x| <= 1e6 and no squared distance overflows.  NaN, infinities and squared distances
beyond FLT_MAX are undefined in the reference (nanoflann compares with `<` and seeds its result set with the largest float,
nanoflann.hpp:79-145) and are out of scope here: no builder produces them and no test asks what the kernels do with them."""
import numpy as np

from oracle.knn import sqdist_f32

F = np.float32


def _rng(seed, name):
    return np.random.RandomState((seed * 1000003 + sum(ord(c) * (i + 1) for i, c in enumerate(name))) % (2 ** 31))


def _self_queries(sup, Q):
    """the first Q points of the cloud (the cloud again from the start when Q > S)"""
    return sup[np.arange(Q) % sup.shape[0]].copy()


def lattice_dims(S):
    """nx = ny ~ sqrt(S / 8), nz layers to hold S points: 16 x 16 x 8 for 2048"""
    n = max(2, int(round((S / 8.0) ** 0.5)))
    return n, n, -(-S // (n * n))


def _lattice(S, Q, g):
    """Integer lattice with spacing 1 (the first S points in raster order when S is no product nx*ny*nz), shuffled; it is its own
    query set.  An interior row has 6 neighbours at d2 = 1 and 12 at d2 = 2: K = 16 cuts inside the 12-way tie, whose members lie
    in different tiles."""
    nx, ny, nz = lattice_dims(S)
    i = np.arange(S)
    sup = np.stack([i % nx, (i // nx) % ny, i // (nx * ny)], axis=1).astype(F)
    sup = sup[g.permutation(S)]
    return sup, _self_queries(sup, Q)


def _lattice_mid(S, Q, g):
    """the lattice again, queried from the midpoints of its edges, faces and cells: the NEAREST neighbour is a 2-, 4- or 8-way
    exact tie (d2 = 0.25, 0.5, 0.75), mostly across tiles -- the K = 1 kernel has to pick the lowest index"""
    sup, _ = _lattice(S, Q, g)
    offs = np.array([[.5, 0, 0], [0, .5, 0], [0, 0, .5], [.5, .5, 0], [0, .5, .5], [.5, .5, .5]], F)
    pick = g.randint(0, S, Q)
    return sup, (sup[pick] + offs[g.randint(0, len(offs), Q)]).astype(F)


def _line_lattice(S, Q, g):
    """S points at x = 0 .. S-1 on a line (y = z = 0.1), shuffled, queried from the midpoints x = j + 0.5: every query has two
    nearest neighbours at exactly d2 = 0.25.  Morton order is x order here, so tile t holds x in [64 t, 64 t + 64) and the 64
    queries of a wave end half a unit in front of the next tile: the box of that tile is EXACTLY as far from the wave's query
    box as the wave's largest nearest distance, and it holds the tie member with the lower index in every other case."""
    sup = np.stack([np.arange(S), np.full(S, 0.1), np.full(S, 0.1)], axis=1).astype(F)[g.permutation(S)]
    qry = np.stack([(np.arange(Q) % (S - 1)) + 0.5, np.full(Q, 0.1), np.full(Q, 0.1)], axis=1).astype(F)[g.permutation(Q)]
    return sup, qry


def _identical(point):
    def make(S, Q, g):
        """S copies of one point: all extents and all Morton keys are 0; every row must be 0..K-1 at distance 0"""
        return np.tile(np.asarray(point, F), (S, 1)), np.tile(np.asarray(point, F), (Q, 1))
    return make


def _origin_heavy(S, Q, g):
    """a random cloud in which 40 % of the points are exactly (0,0,0) at scattered indices (invalid-depth pixels spanning many
    tiles); queries: the cloud itself, the last one replaced by the origin"""
    sup = (g.rand(S, 3) - 0.5).astype(F)
    sup[g.permutation(S)[:(2 * S) // 5]] = 0
    qry = _self_queries(sup, Q)
    qry[-1] = 0
    return sup, qry


def _wrap_dup(S, Q, g):
    """concatenate([base, base[:n]]) with n ~ S/3: np.pad(..., 'wrap') of a cloud that is too short.  NOT shuffled."""
    n = S // 3
    base = g.rand(S - n, 3).astype(F)
    sup = np.concatenate([base, base[:n]], axis=0)
    return sup, sup[(np.arange(Q) * 7) % S].copy()      # originals and copies among the queries for any Q


def _flat(n_const, value):
    def make(S, Q, g):
        """the last `n_const` coordinates constant (plane: z; line: y and z): zero-extent axes.  Queries: support points at the
        even slots, points off the plane / line at the odd ones"""
        sup = g.rand(S, 3).astype(F)
        sup[:, 3 - n_const:] = F(value)
        qry = _self_queries(sup, Q)
        qry[1::2] = (g.rand(Q, 3).astype(F) * F(2) - F(0.5))[1::2]
        return sup, qry
    return make


TWO_CLUSTERS_NEAR = 10


def _two_clusters(S, Q, g):
    """10 points within 0.01 of the origin, S - 10 in a unit ball 50 units away; queries near the small cluster (even slots) and
    in the empty gap between the two (odd slots).  K = 16 takes the 10 near points, then the 6 nearest far ones."""
    near = ((g.rand(TWO_CLUSTERS_NEAR, 3) - 0.5) * 0.02).astype(F)
    v = g.randn(S - TWO_CLUSTERS_NEAR, 3)
    v *= (g.rand(S - TWO_CLUSTERS_NEAR, 1) ** (1 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
    far = (v + np.array([30.0, 40.0, 0.0])).astype(F)
    sup = np.concatenate([near, far], axis=0)[g.permutation(S)]
    qry = ((g.rand(Q, 3) - 0.5) * 0.02).astype(F)
    t = (0.2 + 0.6 * g.rand(Q, 1))
    gap = (t * np.array([30.0, 40.0, 0.0]) + (g.rand(Q, 3) - 0.5)).astype(F)
    qry[1::2] = gap[1::2]
    return sup, qry


def _outside(S, Q, g):
    """support uniform in [0,1)^3; queries in [5,6)^3, in [-6,-5)^3 and on a line that passes the box at distance 3, in turn:
    every one of them clamps to a corner or edge cell of the support's Morton frame"""
    sup = g.rand(S, 3).astype(F)
    r = g.rand(Q, 3)
    line = np.stack([r[:, 0] * 9.0 - 4.0, np.full(Q, -3.0), np.full(Q, 0.5)], axis=1)
    qry = np.where((np.arange(Q) % 3 == 0)[:, None], r + 5.0, np.where((np.arange(Q) % 3 == 1)[:, None], r - 6.0, line))
    return sup, qry.astype(F)


def _offset(S, Q, g):
    """1000 + 0.01 * rand: millimetres far from the origin.  float32 has about 164 values per axis in that range, so the
    rounded distances tie all the time"""
    sup = F(1000) + F(0.01) * g.rand(S, 3).astype(F)
    return sup.astype(F), _self_queries(sup, Q)


def _signed(S, Q, g):
    """uniform in [-1e4, 1e4)^3, queries drawn on their own"""
    return ((g.rand(S, 3) * 2e4) - 1e4).astype(F), ((g.rand(Q, 3) * 2e4) - 1e4).astype(F)


def _tiny(S, Q, g):
    """[1,2) * 2^-70: every squared distance is subnormal or zero (the products of differences that are multiples of 2^-93
    mostly underflow).  Defined in the reference -- plain IEEE arithmetic, and neither oracle/Makefile nor the product build
    flushes subnormals or enables fast-math -- so the kernels have to reproduce it bit for bit."""
    sup = ((F(1) + g.rand(S, 3).astype(F)) * F(2.0 ** -70)).astype(F)
    return sup, _self_queries(sup, Q)


def _uniform(S, Q, g):
    """uniform in [1,2)^3: all differences are multiples of 2^-23 (the metamorphic scaling checks rely on it); queries drawn on
    their own"""
    return (F(1) + g.rand(S, 3).astype(F)).astype(F), (F(1) + g.rand(Q, 3).astype(F)).astype(F)


_BUILDERS = {
    "lattice": _lattice,
    "lattice_mid": _lattice_mid,
    "line_lattice": _line_lattice,
    "identical_origin": _identical((0.0, 0.0, 0.0)),
    "identical_offset": _identical((0.3, -1.7, 2.5)),
    "origin_heavy": _origin_heavy,
    "wrap_dup": _wrap_dup,
    "plane_zero": _flat(1, 0.0),
    "plane_tenth": _flat(1, 0.1),          # 0.1 is no float32 and no sum of a few powers of two
    "line_zero": _flat(2, 0.0),
    "line_tenth": _flat(2, 0.1),
    "two_clusters": _two_clusters,
    "outside": _outside,
    "offset": _offset,
    "signed": _signed,
    "tiny": _tiny,
    "uniform": _uniform,
}
GEOMETRIES = tuple(_BUILDERS)


def build(name, S, Q, B=1, seed=0):
    frames = [_BUILDERS[name](S, Q, _rng(seed + b, name)) for b in range(B)]
    sup = np.ascontiguousarray(np.stack([f[0] for f in frames]), dtype=F)
    qry = np.ascontiguousarray(np.stack([f[1] for f in frames]), dtype=F)
    assert sup.shape == (B, S, 3) and qry.shape == (B, Q, 3)
    assert np.isfinite(sup).all() and np.isfinite(qry).all() and max(np.abs(sup).max(), np.abs(qry).max()) <= 1e6
    return name, sup, qry


def mixed_batch(S, Q, seed=0):
    """B = 3: frame 0 `identical_offset`, frame 1 `plane_tenth`, frame 2 `uniform` -- per-frame boxes, keys and strides"""
    parts = [build(n, S, Q, 1, seed + i) for i, n in enumerate(("identical_offset", "plane_tenth", "uniform"))]
    return "mixed_batch", np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])


def permutation_cloud():
    """the uniform cloud of the metamorphic checks (S = 3000, Q = 500) and its fixed support permutation"""
    _, sup, qry = build("uniform", 3000, 500, seed=3)
    return sup, qry, np.random.RandomState(5).permutation(3000)


def rows_with_a_tie(sup, qry, K):
    """[B,Q] bool: rows with an exact tie among their K + 1 smallest oracle distances"""
    from oracle.knn import knn_batch
    _, d = knn_batch(sup, qry, K + 1, return_dist=True)
    return (np.diff(d, axis=-1) == 0).any(axis=-1)


# ---------------------------------------------------------------------------------------------------------------------------
# the contract in plain numpy, stated twice, neither through the C oracle
# ---------------------------------------------------------------------------------------------------------------------------
def brute_force(sup, qry, K):
    """float32 brute force with np.lexsort((index, distance)): (idx int64 [B,Q,K], dist float32 [B,Q,K])"""
    B, S, _ = sup.shape
    idx = np.empty((B, qry.shape[1], K), np.int64)
    for b in range(B):
        d = sqdist_f32(qry[b][:, None, :], sup[b][None, :, :])
        index = np.broadcast_to(np.arange(S), d.shape)
        idx[b] = np.lexsort((index, d), axis=-1)[:, :K]
    dist = np.stack([np.take_along_axis(sqdist_f32(qry[b][:, None, :], sup[b][None, :, :]), idx[b], axis=1) for b in range(B)])
    return idx, dist.astype(F)


def check_contract(sup, qry, idx, dist, tag=""):
    """The tie rule asserted on a result itself (idx [B,Q,K] any integer dtype, dist [B,Q,K] float32):
      1. dist == sqdist_f32(query, support[idx]);
      2. rows non-decreasing in distance, strictly increasing in index inside a run of equal distances;
      3. no index twice in a row, all indices in [0, S);
      4. no support point outside the row is nearer than the row's last distance, and none at exactly that distance has a
         smaller index than the last entry (the largest index of the row's last tie run)."""
    B, S, _ = sup.shape
    idx = np.asarray(idx).astype(np.int64)
    dist = np.asarray(dist)
    assert idx.shape == dist.shape and idx.shape[:2] == qry.shape[:2], tag
    assert dist.dtype == np.float32, tag
    K = idx.shape[2]
    assert ((idx >= 0) & (idx < S)).all(), f"{tag}: index outside [0, S)"
    for b in range(B):
        i, d = idx[b], dist[b]
        np.testing.assert_array_equal(d, sqdist_f32(qry[b][:, None, :], sup[b][i]), err_msg=f"{tag}: frame {b}: distances are not those of the indices")
        dd, di = np.diff(d, axis=1), np.diff(i, axis=1)
        assert (dd >= 0).all(), f"{tag}: frame {b}: a row is not sorted by distance"
        assert (di[dd == 0] > 0).all(), f"{tag}: frame {b}: a tie run is not in ascending index order"
        assert (np.diff(np.sort(i, axis=1), axis=1) > 0).all(), f"{tag}: frame {b}: an index is repeated in a row"
        full = sqdist_f32(qry[b][:, None, :], sup[b][None, :, :])
        outside = np.ones(full.shape, bool)
        np.put_along_axis(outside, i, False, axis=1)
        last_d, last_i = d[:, K - 1:K], i[:, K - 1:K]
        assert not (outside & (full < last_d)).any(), f"{tag}: frame {b}: a nearer support point was left out"
        assert not (outside & (full == last_d) & (np.arange(S)[None, :] < last_i)).any(), \
            f"{tag}: frame {b}: a support point at the last distance with a lower index was left out"
