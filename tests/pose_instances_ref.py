"""tests/pose_instances_ref.py -- TEST INFRASTRUCTURE ONLY (never imported by the product path).

Plain numpy / torch restatement of
  * the peel of include/ffb6d_pose.h (ffb6d_mean_shift_multi_f32; MeanShiftTorch.fit_multi_clus, meanshift_pytorch.py:60-85):
    `peel` on given converged points, `fit_multi_clus` = the mean-shift iteration of oracle/pose_ref.py, then the peel;
  * the dataflow of pose.solve_instances: centre clusters per (frame, class), keypoint votes of the points whose centre vote
    lies in a cluster, one least-squares fit per cluster, the score;
and the generator of frames with several instances of one class that the GPU test solves.  Pinned to the reference by
tests/golden/make_golden_ms_multi.py (fixture tests/golden/ms_multi.npz) and tests/test_pose_instances_cpu.py.
"""
import numpy as np
import torch

from ffb6d_amd import synth
from oracle import pose_ref


def converged_points(votes, bandwidth, max_iter=300):
    """The points MeanShiftTorch.fit ends with (meanshift_pytorch.py:35-49): the loop of oracle.pose_ref.mean_shift_fit.
    votes f32 tensor [M,3] -> (f32 tensor [M,3], rounds)."""
    M, c = votes.shape
    pts = votes.clone()
    norm_c = bandwidth * np.sqrt(2 * np.pi)
    rounds = 0
    while True:
        rounds += 1
        dist = torch.norm(pts.reshape(1, M, c) - pts.reshape(M, 1, c), dim=2)
        wgt = (torch.exp(-0.5 * ((dist / bandwidth)) ** 2) / norm_c).reshape(M, M, 1)
        moved = torch.sum(wgt * pts, dim=1) / torch.sum(wgt, dim=1)
        step = torch.norm(moved - pts, dim=1)
        pts = moved
        if torch.max(step) < bandwidth * 1e-3 or rounds > max_iter:
            break
    return pts, rounds


def within(C, i, bandwidth):
    """|C_i - C_j| < bandwidth for every j, in the kernels' arithmetic: fp32, sqrtf(dx*dx + dy*dy + dz*dz), every product and
    sum rounded on its own."""
    d = C[i][None, :] - C
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    return np.sqrt(dx * dx + dy * dy + dz * dz, dtype=np.float32) < np.float32(bandwidth)


def peel(C, bandwidth, max_clusters=None, min_inside=1):
    """The rule of include/ffb6d_pose.h on converged points C f32 [M,3] -> (centres f32 [k,3], cluster int32 [M] (0 = none),
    n_inside list).  max_clusters=None: no cap (the reference's full sequence when min_inside = 1).  The ball sizes are
    recounted on the alive points at every peel (the definition; the kernels subtract instead)."""
    C = np.ascontiguousarray(C, np.float32)
    M = len(C)
    cluster = np.zeros(M, np.int32)
    centres, n_inside = [], []
    near = np.stack([within(C, i, bandwidth) for i in range(M)]) if M else np.zeros((0, 0), bool)
    while True:
        alive = np.flatnonzero(cluster == 0)
        if len(alive) == 0 or (max_clusters is not None and len(centres) == max_clusters):
            break
        sizes = near[alive][:, alive].sum(1)
        w = alive[int(np.argmax(sizes))]                        # np.argmax: the first of equal sizes = the lowest index
        if sizes.max() < min_inside:
            break
        members = alive[near[w, alive]]
        centres.append(C[w].copy())
        n_inside.append(int(sizes.max()))
        cluster[members] = len(centres)
    return np.array(centres, np.float32).reshape(-1, 3), cluster, n_inside


def fit_multi_clus(votes, bandwidth, max_clusters=None, min_inside=1, max_iter=300):
    """votes f32 array [M,3] -> peel of the converged points."""
    C, _ = converged_points(torch.from_numpy(np.ascontiguousarray(votes, np.float32)), bandwidth, max_iter)
    return peel(C.numpy(), bandwidth, max_clusters, min_inside)


def solve_instances(pcld, mask, ctr_of, kp_of, mesh_kps, mesh_ctr, max_instances, min_inside=1, min_fraction=0.0, classes=None,
                    radius=0.04):
    """The dataflow of pose.solve_instances on numpy frames (pcld [B,N,3], mask [B,N], ctr_of [B,1,N,3], kp_of [B,n_kps,N,3]).
    Returns rows ordered by (frame, class, instance): list of dict(frame, cls, instance, RT [3,4], kps [n_kps+1,3], n_inside,
    score)."""
    rows = []
    for b in range(len(pcld)):
        cls_ids = sorted(set(int(c) for c in np.unique(mask[b]) if c > 0)) if classes is None else list(classes)
        ctr_votes = pcld[b] - ctr_of[b, 0]
        for c in cls_ids:
            sel = np.flatnonzero(mask[b] == c)
            if len(sel) == 0:
                continue
            centres, cluster, n_in = fit_multi_clus(ctr_votes[sel], radius, max_instances, min_inside)
            for k, (ctr, n) in enumerate(zip(centres, n_in)):
                score = np.float32(n) / np.float32(len(sel))
                if score < min_fraction:
                    continue
                pts = sel[cluster == k + 1]
                kps = [np.asarray(pose_ref.mean_shift_fit(torch.from_numpy(pcld[b, pts] - kp_of[b, s, pts]), radius)[0])
                       for s in range(kp_of.shape[1])]
                found = np.stack(kps + [ctr]).astype(np.float32)
                model = np.concatenate([mesh_kps[c], mesh_ctr[c].reshape(1, 3)]).astype(np.float32)
                rows.append(dict(frame=b, cls=c, instance=k + 1, RT=pose_ref.best_fit_transform(model, found), kps=found,
                                 n_inside=n, score=score))
    return rows


def blobs(seed, sizes, spread=0.004, gap=0.5, outliers=0):
    """Gaussian blobs of the given sizes around well separated centres (+ uniform outliers), shuffled: f32 [sum(sizes)+outliers,3]."""
    rng = np.random.RandomState(seed)
    parts = [np.array([gap * k, 0.1 * rng.randn(), 1.0]) + spread * rng.randn(n, 3) for k, n in enumerate(sizes)]
    if outliers:
        parts.append(rng.uniform(-1, 1, (outliers, 3)) * [gap * len(sizes), 0.5, 0.5] + [0, 0, 1])
    pts = np.concatenate(parts).astype(np.float32)
    return pts[rng.permutation(len(pts))]


def make_multi_instance_frames(seed, n_pts=2048, instances=(2, 3), n_kps=8, noise=0.004, outliers=0.1, bg_frac=0.25, placed=None,
                               local=None):
    """Frames with `instances[b]` instances of class 1 (0.4 m apart) and one instance of class 2; votes = true offsets + noise +
    outliers as synth.make_pose_case builds them.  placed: the instances to use instead, a list over frames of [(class id, RT)]
    (classes 1 and 2); local(c, rng): a point of object c in its model frame (default: a ball of 0.07 m).
    Returns dict: pcld f32 [B,N,3], mask i64 [B,N], ctr_of f32 [B,1,N,3], kp_of f32 [B,n_kps,N,3], mesh_kps f32 [3,n_kps,3],
    mesh_ctr f32 [3,3], poses: list over frames of [(class id, RT f64 [3,4])]."""
    rng = np.random.RandomState(seed)
    mesh_kps = (rng.rand(3, n_kps, 3).astype(np.float32) - 0.5) * 0.2
    mesh_ctr = (rng.rand(3, 3).astype(np.float32) - 0.5) * 0.02
    B = len(instances) if placed is None else len(placed)
    pcld = np.zeros((B, n_pts, 3), np.float32)
    mask = np.zeros((B, n_pts), np.int64)
    ctr_of = np.zeros((B, 1, n_pts, 3), np.float32)
    kp_of = np.zeros((B, n_kps, n_pts, 3), np.float32)
    poses = []
    for b in range(B):
        if placed is not None:
            here = list(placed[b])
        else:
            objs = [1] * instances[b] + [2]
            here = []
            for j, c in enumerate(objs):
                t = np.array([0.4 * (j - (len(objs) - 1) / 2), 0.05 * rng.randn(), 1.0 + 0.2 * rng.rand()])
                RT = np.zeros((3, 4))
                RT[:, :3], RT[:, 3] = synth.random_rotation(rng), t
                here.append((c, RT))
        objs = [c for c, _ in here]
        poses.append(here)
        owner = rng.choice(len(objs) + 1, size=n_pts, p=[bg_frac] + [(1 - bg_frac) / len(objs)] * len(objs))
        for i in range(n_pts):
            if owner[i] == 0:
                pcld[b, i] = [rng.uniform(-1, 1), rng.uniform(-0.6, 0.6), rng.uniform(0.6, 1.6)]
                ctr_of[b, 0, i] = 0.2 * rng.randn(3)
                kp_of[b, :, i] = 0.2 * rng.randn(n_kps, 3)
                continue
            c, RT = here[owner[i] - 1]
            R, t = RT[:, :3], RT[:, 3]
            if local is None:
                at = rng.randn(3)
                at *= 0.07 * rng.rand() ** (1 / 3) / np.linalg.norm(at)
            else:
                at = local(c, rng)
            p = R @ at + t
            pcld[b, i] = p
            mask[b, i] = c
            ctr_of[b, 0, i] = p - (R @ mesh_ctr[c] + t) + noise * rng.randn(3)
            kp_of[b, :, i] = p[None] - (mesh_kps[c] @ R.T + t) + noise * rng.randn(n_kps, 3)
            if rng.rand() < outliers:
                ctr_of[b, 0, i] += 0.15 * rng.randn(3)
                kp_of[b, :, i] += 0.15 * rng.randn(n_kps, 3)
    return dict(pcld=pcld, mask=mask, ctr_of=ctr_of, kp_of=kp_of, mesh_kps=mesh_kps, mesh_ctr=mesh_ctr, poses=poses)
