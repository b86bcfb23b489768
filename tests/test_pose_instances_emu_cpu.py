"""The peel of csrc/pose.hip (ffb6d_mean_shift_multi_f32, include/ffb6d_pose.h) on the SIMT emulator (tests/simt), without a GPU:
the unmodified kernel source compiled for the host, run through the C ABI on tiny sets and held against the numpy restatement
(tests/pose_instances_ref.py) run on the kernel's OWN converged points (ffb6d_pose_set_converged_out) -- cluster ids, ball sizes and
cluster counts equal, centres bit-equal to converged points; cluster 1 against the single fit as bits; the instance map and the
per-instance vote sets."""
import numpy as np
import pytest

import pose_instances_ref as ref
from tests.simt.build import load, ptr as _p

BW = 0.04


@pytest.fixture(scope="module")
def emu_pose():
    """the emulated library (tests/simt/build.py)"""
    return load()


def pack(clouds, stride):
    """sets f32 [G,stride,4] (.w = the vote's index as bits; NaN behind every count: padding must not matter), counts i32 [G]"""
    sets = np.full((len(clouds), stride, 4), np.nan, np.float32)
    for g, c in enumerate(clouds):
        sets[g, :len(c), :3] = c
        sets[g, :len(c), 3] = np.arange(len(c), dtype=np.int32).view(np.float32)
    return sets, np.array([len(c) for c in clouds], np.int32)


def run_multi(lib, sets, counts, K, min_inside, max_iter=300):
    G, stride, _ = sets.shape
    wbytes = lib.ffb6d_mean_shift_multi_workspace_bytes(G, stride)
    assert wbytes == lib.ffb6d_mean_shift_workspace_bytes(G, stride)
    ws = np.zeros(wbytes, np.uint8)
    centers, cluster = np.full((G, K, 3), 7, np.float32), np.full((G, stride), 7, np.uint8)
    n_in, n_clus, iters = np.full((G, K), 7, np.int32), np.full(G, 7, np.int32), np.full(G, 7, np.int32)
    conv = np.full((G, stride, 4), 7, np.float32)
    lib.ffb6d_pose_set_converged_out(_p(conv))
    try:
        rc = lib.ffb6d_mean_shift_multi_f32(_p(sets), _p(counts), 1, G, stride, 0, BW, max_iter, 0, K, min_inside, _p(centers), _p(cluster),
                                            _p(n_in), _p(n_clus), _p(iters), _p(ws), wbytes, None)
    finally:
        lib.ffb6d_pose_set_converged_out(None)
    assert rc == 0, lib.ffb6d_last_error()
    return centers, cluster, n_in, n_clus, iters, conv


def run_single(lib, sets, counts, max_iter=300):
    G, stride, _ = sets.shape
    wbytes = lib.ffb6d_mean_shift_workspace_bytes(G, stride)
    ws = np.zeros(wbytes, np.uint8)
    centers, labels = np.full((G, 3), 7, np.float32), np.full((G, stride), 7, np.uint8)
    n_in, iters = np.full(G, 7, np.int32), np.full(G, 7, np.int32)
    rc = lib.ffb6d_mean_shift_f32(_p(sets), _p(counts), 1, G, stride, 0, BW, max_iter, 0, _p(centers), _p(labels), _p(n_in), _p(iters),
                                  _p(ws), wbytes, None)
    assert rc == 0, lib.ffb6d_last_error()
    return centers, labels, n_in, iters


def tiny_sets():
    """Counts 0, 1, 3, 40, 64 behind one stride: empty; one point; three points (two of them within the bandwidth); three
    separated blobs of 20 / 13 / 7; all points equal (40); every vote twice (64); and a constructed tie -- two balls of three
    points each, the second ball holds index 0."""
    blobs = ref.blobs(3, (20, 13, 7))
    twice = ref.blobs(4, (18, 10, 4))
    twice = np.concatenate([twice, twice])
    tie = np.float32([[1.0, 0, 1], [0, 0, 1], [0.001, 0, 1], [1.001, 0, 1], [0, 0.001, 1], [1, 0.001, 1]])
    three = np.float32([[0, 0, 1], [0.5, 0, 1], [0.5, 0.01, 1]])
    clouds = [np.zeros((0, 3), np.float32), np.float32([[0.1, 0.2, 0.3]]), three, blobs, np.tile(np.float32([[0.3, 0.2, 1.1]]), (40, 1)),
              twice, tie]
    assert [len(c) for c in clouds] == [0, 1, 3, 40, 40, 64, 6]
    return clouds


@pytest.mark.parametrize("min_inside", [1, 5])
@pytest.mark.parametrize("K", [1, 2, 4, 9])
def test_peel_on_the_emulator_equals_the_restatement_on_the_kernels_own_points(emu_pose, K, min_inside):
    lib = emu_pose
    clouds = tiny_sets()
    sets, counts = pack(clouds, 64)
    centers, cluster, n_in, n_clus, iters, conv = run_multi(lib, sets, counts, K, min_inside)
    s_centers, s_labels, s_n_in, s_iters = run_single(lib, sets, counts)
    for g, c in enumerate(clouds):
        M = len(c)
        C = conv[g, :M, :3]
        assert np.array_equal(conv[g, :M, 3].view(np.int32), np.arange(M))                # the votes' own .w
        w_centres, w_cluster, w_n_in = ref.peel(C, BW, K, min_inside)
        k = len(w_n_in)
        assert int(n_clus[g]) == k, (g, n_clus[g], w_n_in)
        assert np.array_equal(cluster[g, :M], w_cluster) and not cluster[g, M:].any(), g
        assert list(n_in[g, :k]) == w_n_in and not n_in[g, k:].any() and not centers[g, k:].any(), g
        assert np.array_equal(centers[g, :k].view(np.uint32), w_centres.view(np.uint32)), g   # bit-equal to converged points
        assert all(w_n_in[i] >= w_n_in[i + 1] for i in range(k - 1))
        assert int(iters[g]) == int(s_iters[g])
        if M and (min_inside == 1 or s_n_in[g] >= min_inside):                             # cluster 1 = the single fit, as bits
            assert np.array_equal(centers[g, 0].view(np.uint32), s_centers[g].view(np.uint32)) and n_in[g, 0] == s_n_in[g], g
            assert np.array_equal(cluster[g, :M] == 1, s_labels[g, :M] == 1), g
    # what the sets were built for
    full = ref.peel(conv[3, :40, :3], BW)[2]
    assert full == [20, 13, 7]
    assert list(n_in[3, :min(K, 3)]) == ([20, 13, 7] if min_inside == 1 else [20, 13, 7][:3])[:min(K, 3)]
    assert int(n_clus[0]) == 0 and int(n_clus[4]) == 1 and int(n_in[4, 0]) == 40
    assert list(n_in[5, :min(K, 3)]) == [36, 20, 8][:min(K, 3)]                             # every vote twice
    if min_inside == 1:
        assert int(n_clus[1]) == 1 and int(n_clus[2]) == min(K, 2) and list(n_in[2, :min(K, 2)]) == [2, 1][:min(K, 2)]
        # the tie: both balls hold three points; index 0 lies in the ball around x = 1, which therefore wins
        assert int(n_in[6, 0]) == 3 and abs(centers[6, 0, 0] - 1.0) < 0.01 and cluster[6, 0] == 1
        if K >= 2:
            assert int(n_in[6, 1]) == 3 and abs(centers[6, 1, 0]) < 0.01 and list(cluster[6, :6]) == [1, 2, 2, 1, 2, 1]
    else:
        assert int(n_clus[1]) == 0 and int(n_clus[2]) == 0 and int(n_clus[6]) == 0


def test_a_set_alone_equals_the_set_in_a_batch_and_unconverged_points_peel_too(emu_pose):
    """ragged counts behind one stride: every set equals its own single-set call bit for bit; max_iter = 0 (one round: most
    points still distinct, many overlapping balls) exercises the subtraction of removed members from the survivors' sizes"""
    lib = emu_pose
    clouds = tiny_sets()
    for max_iter in (300, 0):
        sets, counts = pack(clouds, 64)
        batch = run_multi(lib, sets, counts, 4, 1, max_iter)
        for g, c in enumerate(clouds):
            s1, c1 = pack([c], max(len(c), 1))
            alone = run_multi(lib, s1, c1, 4, 1, max_iter)
            M = len(c)
            assert np.array_equal(alone[0][0].view(np.uint32), batch[0][g].view(np.uint32)), (max_iter, g)
            assert np.array_equal(alone[1][0, :M], batch[1][g, :M]) and np.array_equal(alone[2][0], batch[2][g])
            assert alone[3][0] == batch[3][g] and alone[4][0] == batch[4][g]
            w = ref.peel(batch[5][g, :M, :3], BW, 4, 1)
            assert np.array_equal(batch[1][g, :M], w[1]) and list(batch[2][g, :len(w[2])]) == w[2], (max_iter, g)


def test_bad_arguments_are_refused(emu_pose):
    lib = emu_pose
    sets, counts = pack(tiny_sets()[:4], 64)
    G = 4
    wbytes = lib.ffb6d_mean_shift_multi_workspace_bytes(G, 64)
    ws = np.zeros(wbytes, np.uint8)
    out = [np.full((G, 256, 3), 7, np.float32), np.full((G, 64), 7, np.uint8), np.full((G, 256), 7, np.int32), np.full(G, 7, np.int32)]
    call = lambda K, mi, nbytes: lib.ffb6d_mean_shift_multi_f32(_p(sets), _p(counts), 1, G, 64, 0, BW, 300, 0, K, mi, _p(out[0]), _p(out[1]),
                                                                _p(out[2]), _p(out[3]), None, _p(ws), nbytes, None)      # noqa: E731
    assert call(0, 1, wbytes) == -1 and call(256, 1, wbytes) == -1 and call(2, 0, wbytes) == -1 and call(2, 1, wbytes - 1) == -3
    assert all((o == 7).all() for o in out)                                                # nothing was written
    assert call(255, 1, wbytes) == 0


def test_instance_map_and_per_instance_vote_sets(emu_pose):
    """two frames of 48 points, classes 1 and 2; class 1 of frame 0 has two centre clusters: the map carries the cluster id of
    every point's centre vote, the per-instance vote sets select by (class, id) in point order"""
    lib = emu_pose
    rng = np.random.RandomState(1)
    B, N, S = 2, 48, 2
    pcld = rng.rand(B, N, 3).astype(np.float32)
    mask = rng.randint(0, 3, (B, N)).astype(np.int64)
    target = np.zeros((B, N, 3), np.float32)
    target[:, :, 0] = mask                                                                  # centre votes: x = class ...
    target[0, (mask[0] == 1) & (np.arange(N) % 3 == 0), 1] = 0.5                            # ... class 1 of frame 0: a second centre
    ctr_of = (pcld - target)[:, None].copy()
    kp_of = rng.rand(B, S, N, 3).astype(np.float32)
    frame_of, class_of = np.array([0, 0, 1, 1], np.int32), np.array([1, 2, 1, 2], np.int32)
    P = 4
    sets, counts = np.zeros((P, N, 4), np.float32), np.zeros(P, np.int32)
    assert lib.ffb6d_vote_sets_f32(_p(pcld), _p(ctr_of), _p(mask), 64, None, _p(frame_of), _p(class_of), P, B, 1, N, N, _p(sets), _p(counts),
                                   None) == 0
    centers, cluster, n_in, n_clus, _, _ = run_multi(lib, sets, counts, 3, 1)
    assert list(n_clus) == [2, 1, 1, 1]
    inst = np.zeros((B, N), np.uint8)
    assert lib.ffb6d_set_clusters_to_points(_p(sets), _p(cluster), _p(counts), _p(frame_of), P, N, N, _p(inst), None) == 0
    want = np.zeros((B, N), np.uint8)
    for p in range(P):
        idx = np.flatnonzero(mask[frame_of[p]] == class_of[p])
        want[frame_of[p], idx] = cluster[p, :len(idx)]
    assert np.array_equal(inst, want) and set(np.unique(inst[0][mask[0] == 1])) == {1, 2} and not inst[mask == 0].any()
    rows = [(0, 1, 1), (0, 1, 2), (0, 2, 1), (1, 1, 1), (1, 2, 1), (1, 2, 2)]
    f, c, k = (np.array(x, np.int32) for x in zip(*rows))
    ksets, kcounts = np.full((len(rows) * S, N, 4), 7, np.float32), np.full(len(rows), 7, np.int32)
    assert lib.ffb6d_vote_sets_inst_f32(_p(pcld), _p(kp_of), _p(mask), 64, _p(inst), _p(f), _p(c), _p(k), len(rows), B, S, N, N, _p(ksets),
                                        _p(kcounts), None) == 0, lib.ffb6d_last_error()
    for e, (b, cls, kk) in enumerate(rows):
        idx = np.flatnonzero((mask[b] == cls) & (inst[b] == kk))
        assert kcounts[e] == len(idx) and (len(idx) > 0) == (e != 5)
        for s in range(S):
            got = ksets[e * S + s, :len(idx)]
            assert np.array_equal(got[:, :3], pcld[b, idx] - kp_of[b, s, idx]) and np.array_equal(got[:, 3].view(np.int32), idx)
