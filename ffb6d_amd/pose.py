"""Pose solver on the GPU: the step after FFB6D.forward.

Host-side mirror of the reference's
    MeanShiftTorch                      ffb6d/utils/meanshift_pytorch.py:27-85 (fit, fit_multi_clus)
    best_fit_transform                  ffb6d/utils/pvn3d_eval_utils_kpls.py:28-61
    cal_frame_poses / cal_frame_poses_lm   ffb6d/utils/pvn3d_eval_utils_kpls.py:65-158,220-285
over the C ABI of include/ffb6d_pose.h.  The reference solves one object at a time (one mean
shift for the centre, one per keypoint, each with host round trips); `solve_poses` runs all
(frame, object, keypoint) vote sets of a batch through the same launches; `solve_instances` does the same for
every centre cluster of a class (several instances of an object in a frame), each with a score.

The mesh keypoints / centres / radii the reference reads from dataset files through
`Basic_Utils` (pvn3d_eval_utils_kpls.py:149-152,277-280, common.py:89-94) are arguments here.
There is no CPU fallback: tensors must live on a GPU and the HIP library must be built.
"""
import numpy as np
import torch

from . import _lib
from .ops import _need_gpu, _stream

RADIUS = 0.04          # bandwidth used by both flows (pvn3d_eval_utils_kpls.py:76,231)
CHECK_EVERY = 8        # rounds between convergence polls


FIT_SPREAD = 1         # csrc/pose.hip ffb6d_pose_set_fit_spread: 1 = the fits' first two rounds chip-wide when the call has few sets


def set_fit_spread(mode):
    """0 never / 1 when G <= CUs / 2 (default) / 2 always; returns the previous setting.  Results do not depend on it."""
    global FIT_SPREAD
    prev, FIT_SPREAD = FIT_SPREAD, int(mode)
    _lib.load().ffb6d_pose_set_fit_spread(FIT_SPREAD)
    return prev


def _i32(values, device):
    return torch.tensor(list(values), dtype=torch.int32, device=device)


def _mask_bits(mask):
    if mask.dtype == torch.int64:
        return 64
    if mask.dtype == torch.int32:
        return 32
    raise TypeError(f"mask must be int32 or int64, got {mask.dtype}")


def _vote_sets(pcld, offsets, mask, frame_of, class_of, keep=None, inst=None, inst_of=None):
    """vote_sets (inst_of is None) and vote_sets_inst around their entry points"""
    _need_gpu(pcld, offsets, mask)
    B, N, _ = pcld.shape
    S = offsets.shape[1]
    P = frame_of.numel()
    pcld, offsets, mask = pcld.contiguous().float(), offsets.contiguous().float(), mask.contiguous()
    sets = torch.empty((P * S, N, 4), dtype=torch.float32, device=pcld.device)
    counts = torch.zeros((P,), dtype=torch.int32, device=pcld.device)
    head = (pcld.data_ptr(), offsets.data_ptr(), mask.data_ptr(), _mask_bits(mask))
    tail = (P, B, S, N, N, sets.data_ptr(), counts.data_ptr(), _stream(pcld))
    if inst_of is None:
        name, rows = "ffb6d_vote_sets_f32", (keep.data_ptr() if keep is not None else None, frame_of.data_ptr(), class_of.data_ptr())
    else:
        name, rows = "ffb6d_vote_sets_inst_f32", (inst.data_ptr(), frame_of.data_ptr(), class_of.data_ptr(), inst_of.data_ptr())
    with torch.cuda.device(pcld.device), _lib.traced("vote_sets", 4 * (3 * B * N * (S + 1)) + 16 * P * S * N, (P, S, N)):
        rc = getattr(_lib.load(), name)(*head, *rows, *tail)
    _lib.check(rc, name)
    return sets, counts


def vote_sets(pcld, offsets, mask, frame_of, class_of, keep=None):
    """Votes `pcld - offsets` of the points with mask == class, per (frame, class) pair.
    pcld [B,N,3], offsets [B,S,N,3], mask [B,N] -> sets f32 [P*S, N, 4], counts i32 [P]."""
    return _vote_sets(pcld, offsets, mask, frame_of, class_of, keep=keep)


def mean_shift(sets, counts, bandwidth, max_iter=300, sets_per_count=1, want_labels=True, check_every=CHECK_EVERY,
               max_count=None):
    """MeanShiftTorch.fit for every set: sets f32 [G,M,4], counts i32 [G/sets_per_count] ->
    centers f32 [G,3], labels bool [G,M] (or None), n_inside i32 [G], rounds i32 [G].
    max_count: accepted and ignored (the library sizes its grids itself; None = 0)."""
    _need_gpu(sets, counts)
    G, M, _ = sets.shape
    dev = sets.device
    centers = torch.empty((G, 3), dtype=torch.float32, device=dev)
    labels = torch.empty((G, M), dtype=torch.uint8, device=dev) if want_labels else None
    n_inside = torch.empty((G,), dtype=torch.int32, device=dev)
    rounds = torch.empty((G,), dtype=torch.int32, device=dev)
    lib = _lib.load()
    wbytes = lib.ffb6d_mean_shift_workspace_bytes(G, M)
    ws = torch.empty((max(wbytes, 1),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _lib.traced("mean_shift", 16 * G * M, (G, M)):
        rc = lib.ffb6d_mean_shift_f32(
            sets.data_ptr(), counts.data_ptr(), sets_per_count, G, M, int(max_count or 0), float(bandwidth), int(max_iter),
            int(check_every), centers.data_ptr(), labels.data_ptr() if labels is not None else None,
            n_inside.data_ptr(), rounds.data_ptr(), ws.data_ptr(), wbytes, _stream(sets))
    _lib.check(rc, "ffb6d_mean_shift_f32")
    return centers, (labels.bool() if labels is not None else None), n_inside, rounds


MAX_CLUSTERS = 255     # cluster ids are u8 in the C ABI (include/ffb6d_pose.h)


def vote_sets_inst(pcld, offsets, mask, inst, frame_of, class_of, inst_of):
    """vote_sets per instance: row p takes the points with mask == class_of[p] and inst == inst_of[p] (inst u8 [B,N], the
    map written by `instance_map`)."""
    _need_gpu(inst)
    return _vote_sets(pcld, offsets, mask, frame_of, class_of, inst=inst, inst_of=inst_of)


def mean_shift_multi(sets, counts, bandwidth, max_clusters, min_inside=1, max_iter=300, sets_per_count=1,
                     check_every=CHECK_EVERY, workspace=None):
    """MeanShiftTorch.fit_multi_clus for every set (the rule is stated in include/ffb6d_pose.h): sets f32 [G,M,4], counts i32
    [G/sets_per_count] -> centers f32 [G,K,3], cluster u8 [G,M] (0 = in no returned cluster), n_inside i32 [G,K],
    n_clusters i32 [G], rounds i32 [G]; K = max_clusters (1 .. 255), balls smaller than min_inside end a set's sequence.
    workspace: None, or a uint8 tensor of at least ffb6d_mean_shift_multi_workspace_bytes(G, M) bytes."""
    _need_gpu(sets, counts)
    G, M, _ = sets.shape
    K = int(max_clusters)
    dev = sets.device
    lib = _lib.load()
    centers = torch.empty((G, max(K, 0), 3), dtype=torch.float32, device=dev)
    cluster = torch.empty((G, M), dtype=torch.uint8, device=dev)
    n_inside = torch.empty((G, max(K, 0)), dtype=torch.int32, device=dev)
    n_clusters = torch.empty((G,), dtype=torch.int32, device=dev)
    rounds = torch.empty((G,), dtype=torch.int32, device=dev)
    if workspace is None:
        workspace = torch.empty((max(lib.ffb6d_mean_shift_multi_workspace_bytes(G, M), 1),), dtype=torch.uint8, device=dev)
    _need_gpu(workspace)
    with torch.cuda.device(dev), _lib.traced("mean_shift_multi", 16 * G * M, (G, M, K)):
        rc = lib.ffb6d_mean_shift_multi_f32(
            sets.data_ptr(), counts.data_ptr(), sets_per_count, G, M, 0, float(bandwidth), int(max_iter), int(check_every), K,
            int(min_inside), centers.data_ptr(), cluster.data_ptr(), n_inside.data_ptr(), n_clusters.data_ptr(), rounds.data_ptr(),
            workspace.data_ptr(), workspace.numel(), _stream(sets))
    _lib.check(rc, "ffb6d_mean_shift_multi_f32")
    return centers, cluster, n_inside, n_clusters, rounds


def instance_map(sets, cluster, counts, frame_of, B, N):
    """inst u8 [B,N]: 0, or the cluster id of the point's centre vote (sets / cluster / counts of the centre-vote sets of the
    (frame, class) pairs; ffb6d_set_clusters_to_points)."""
    _need_gpu(sets, cluster, counts, frame_of)
    inst = torch.zeros((B, N), dtype=torch.uint8, device=sets.device)
    with torch.cuda.device(sets.device):
        rc = _lib.load().ffb6d_set_clusters_to_points(sets.data_ptr(), cluster.data_ptr(), counts.data_ptr(), frame_of.data_ptr(),
                                                     frame_of.numel(), sets.shape[1], N, inst.data_ptr(), _stream(sets))
    _lib.check(rc, "ffb6d_set_clusters_to_points")
    return inst


class MeanShiftTorch:
    """Same constructor and `fit` contract as the reference class (meanshift_pytorch.py:27-58):
    fit(A [N,3] on the GPU) -> (centre [3], labels bool [N])."""

    def __init__(self, bandwidth=0.05, max_iter=300):
        self.bandwidth = bandwidth
        self.stop_thresh = bandwidth * 1e-3
        self.max_iter = max_iter

    def fit_batch(self, clouds):
        """list of [N_i,3] tensors -> (centers [G,3], list of bool [N_i] labels)."""
        dev = clouds[0].device
        M = max(int(c.shape[0]) for c in clouds)
        sets = torch.zeros((len(clouds), M, 4), dtype=torch.float32, device=dev)
        for g, c in enumerate(clouds):
            sets[g, : c.shape[0], :3] = c
        counts = _i32([c.shape[0] for c in clouds], dev)
        centers, labels, _, _ = mean_shift(sets, counts, self.bandwidth, self.max_iter)
        return centers, [labels[g, : c.shape[0]] for g, c in enumerate(clouds)]

    def fit(self, A):
        _need_gpu(A)
        if A.dim() != 2 or A.shape[1] != 3 or A.shape[0] < 1:
            raise ValueError(f"expected a non-empty [N,3] tensor, got {tuple(A.shape)}")
        centers, labels = self.fit_batch([A])
        return centers[0], labels[0]

    def fit_multi_clus(self, A, max_clusters=None):
        """The reference's return contract (meanshift_pytorch.py:60-85): (list of centres [3], int labels [N] with ids 1..,
        list of ball sizes).  max_clusters=None: every cluster as the reference returns them, up to the 255 ids of the C ABI
        (a set that needs more raises); an integer K: the first K of that sequence, points of later clusters labelled 0."""
        _need_gpu(A)
        if A.dim() != 2 or A.shape[1] != 3 or A.shape[0] < 1:
            raise ValueError(f"expected a non-empty [N,3] tensor, got {tuple(A.shape)}")
        N = int(A.shape[0])
        sets = torch.zeros((1, N, 4), dtype=torch.float32, device=A.device)
        sets[0, :, :3] = A
        K = MAX_CLUSTERS if max_clusters is None else int(max_clusters)
        centers, cluster, n_inside, n_clusters, _ = mean_shift_multi(sets, _i32([N], A.device), self.bandwidth, K, 1, self.max_iter)
        n = int(n_clusters[0])
        labels = cluster[0].int()
        if max_clusters is None and n == K and bool((labels == 0).any()):
            raise ValueError(f"the set has more than {MAX_CLUSTERS} clusters (cluster ids are u8); pass max_clusters")
        return [centers[0, k] for k in range(n)], labels, [int(v) for v in n_inside[0, :n].tolist()]


def best_fit_transform_batch(model, found):
    """model, found f32 [P,n,3] on the GPU -> T f64 [P,3,4]."""
    _need_gpu(model, found)
    if model.shape != found.shape or model.dim() != 3 or model.shape[2] != 3:
        raise ValueError(f"shape mismatch {tuple(model.shape)} / {tuple(found.shape)}")
    P, n, _ = model.shape
    model, found = model.contiguous().float(), found.contiguous().float()
    T = torch.empty((P, 3, 4), dtype=torch.float64, device=model.device)
    with torch.cuda.device(model.device):
        rc = _lib.load().ffb6d_best_fit_transform_f32(model.data_ptr(), found.data_ptr(), P, n, T.data_ptr(),
                                                      _stream(model))
    _lib.check(rc, "ffb6d_best_fit_transform_f32")
    return T


def best_fit_transform(A, B, device=None):
    """numpy in, numpy [3,4] out, like pvn3d_eval_utils_kpls.py:28-61 (A: model points, B: camera)."""
    assert A.shape == B.shape
    device = device or torch.device("cuda", torch.cuda.current_device())
    T = best_fit_transform_batch(torch.from_numpy(np.ascontiguousarray(A, np.float32)).to(device)[None],
                                 torch.from_numpy(np.ascontiguousarray(B, np.float32)).to(device)[None])
    return T[0].cpu().numpy()


def _on_device(x):
    return torch.is_tensor(x) and x.is_cuda


def _mesh_tensors(mesh_kps, mesh_ctr, dev):
    """host data, or device tensors as objinfo.ObjectInfo holds them -> f32 tensors on `dev`"""
    f32 = lambda x: x.to(device=dev, dtype=torch.float32) if _on_device(x) else torch.as_tensor(np.asarray(x, np.float32), device=dev)   # noqa: E731
    return f32(mesh_kps), f32(mesh_ctr)


def _gate_distances(r_lst, classes_dev, classes_np, dev):
    """0.8 radii (:98) of classes_dev when the radii live on the device (the same product, in double, no read-back), else of classes_np"""
    if _on_device(r_lst):
        return (r_lst.to(device=dev, dtype=torch.float64)[classes_dev.long() - 1] * 0.8).float()
    return torch.tensor([np.float32(float(r_lst[c - 1]) * 0.8) for c in classes_np], dtype=torch.float32, device=dev)


def _refine_mask(pcld, ctr_of, mask, centers, row_class, row_begin, row_dist):
    """The centre mask filter (:83-108): a foreground point takes the class of the nearest centre among its frame's rows, within row_dist."""
    B, N, _ = pcld.shape
    new_mask = torch.empty_like(mask)
    with torch.cuda.device(pcld.device):
        rc = _lib.load().ffb6d_refine_mask_by_center(pcld.data_ptr(), ctr_of.data_ptr(), mask.data_ptr(), _mask_bits(mask),
                                                     centers.data_ptr(), row_class.data_ptr(), row_begin.data_ptr(),
                                                     row_dist.data_ptr(), B, N, new_mask.data_ptr(), _stream(pcld))
    _lib.check(rc, "ffb6d_refine_mask_by_center")
    return new_mask


def _model_and_found(mesh_kps, mesh_ctr, row_class, kcenters, centers):
    """model and found points [R,n_kps+1,3] of R rows: the keypoints, then the centre (cls_kps rows, :124,136)"""
    R = row_class.shape[0]
    found = torch.cat([kcenters.view(R, -1, 3), centers.view(R, 1, 3)], dim=1)
    cls_long = row_class.long()
    return torch.cat([mesh_kps[cls_long], mesh_ctr[cls_long].view(R, 1, 3)], dim=1), found


def _fit(model, found, n_kps, use_ctr):
    return best_fit_transform_batch(model, found) if use_ctr else best_fit_transform_batch(model[:, :n_kps], found[:, :n_kps])


def solve_poses(pcld, mask, ctr_of, kp_of, mesh_kps, mesh_ctr, r_lst=None, use_ctr=True,
                use_ctr_clus_flter=True, refine_mask=None, classes=None, radius=RADIUS, max_iter=300, stats=None, refine=None):
    """All objects of all frames at once.
      pcld f32 [B,N,3]; mask int [B,N] predicted class per point (0 = background);
      ctr_of f32 [B,1,N,3], kp_of f32 [B,n_kps,N,3] (end_points['pred_ctr_ofs'/'pred_kp_ofs']);
      mesh_kps [n_cls,n_kps,3], mesh_ctr [n_cls,3] model-frame keypoints indexed by class id;
      r_lst[cls_id-1] object radii (needed when refine_mask); all three host data or device tensors (objinfo.ObjectInfo);
      classes: None = every class present in a frame's mask (YCB flow, :82); or a list of class ids
               solved in every frame whether present or not (LineMOD flow: [1], :238-241);
      refine_mask: centre-clustering mask filter (:83-108); default = use_ctr_clus_flter and classes is None.
      stats: optional dict, receives the rounds made per set of each mean-shift pass.
      refine: None, or dict(models=refine.PreparedModels, max_iter=..., max_dist=..., [tol, min_pairs, metric, min_eig]): the fitted poses of every
              (frame, object) pair go through ONE refine.icp_refine call (ICP against the points of `pcld` that the `mask` given
              here assigns to the object) before they are read back; the keypoints column stays as fitted ("refine" in stats
              receives the call's n_pairs / rms / iters).  metric="plane" (models prepared with normals) is the point-to-plane
              metric of refine.icp_refine: fewer iterations for the same pose; "refine" in stats then also holds rms_plane.
    Returns a list over frames of (class_ids int array, poses [n,3,4] float64, kps [n,n_kps+1,3] float32);
    objects without points get the identity pose and zero keypoints (:114-117 / :239-240)."""
    _need_gpu(pcld, mask, ctr_of, kp_of)
    B, N, _ = pcld.shape
    n_kps = kp_of.shape[1]
    dev = pcld.device
    mesh_kps, mesh_ctr = _mesh_tensors(mesh_kps, mesh_ctr, dev)
    if refine_mask is None:
        refine_mask = use_ctr_clus_flter and classes is None
    mask = mask.contiguous()
    mask_given = mask
    lib = _lib.load()

    frame_np, class_np = _frame_class_pairs(mask, classes, B, mesh_kps.shape[0])
    P = len(class_np)
    if P == 0:
        return [(np.zeros(0, np.int64), np.zeros((0, 3, 4)), np.zeros((0, n_kps + 1, 3), np.float32)) for _ in range(B)]
    frame_of, class_of = _i32(frame_np, dev), _i32(class_np, dev)
    ctr_of = ctr_of.contiguous().float()
    pcld = pcld.contiguous().float()

    if refine_mask:
        if r_lst is None:
            raise ValueError("refine_mask needs r_lst (object radii, common.py:89-94)")
        sets, counts = vote_sets(pcld, ctr_of, mask, frame_of, class_of)
        centers, _, _, rounds = mean_shift(sets, counts, radius, max_iter, want_labels=False)
        if stats is not None:
            stats["rounds_refine"], stats["counts_refine"] = rounds, counts
        begin = np.zeros(B + 1, np.int32)
        np.add.at(begin, frame_np + 1, 1)
        pair_begin = _i32(np.cumsum(begin), dev)
        mask = _refine_mask(pcld, ctr_of, mask, centers, class_of, pair_begin, _gate_distances(r_lst, class_of, class_np, dev))

    # object centres (+ the labels of the winning centre cluster)
    sets, counts = vote_sets(pcld, ctr_of, mask, frame_of, class_of)
    centers, labels, _, rounds = mean_shift(sets, counts, radius, max_iter, want_labels=use_ctr_clus_flter)
    if stats is not None:
        stats["rounds_ctr"], stats["counts_ctr"] = rounds, counts
    keep = None
    if use_ctr_clus_flter:
        keep = torch.zeros((B, N), dtype=torch.uint8, device=dev)
        lab8 = labels.to(torch.uint8)
        with torch.cuda.device(dev):
            rc = lib.ffb6d_set_labels_to_points(sets.data_ptr(), lab8.data_ptr(), counts.data_ptr(), frame_of.data_ptr(),
                                                P, N, N, keep.data_ptr(), _stream(pcld))
        _lib.check(rc, "ffb6d_set_labels_to_points")
    # keypoints: n_kps sets per pair
    ksets, kcounts = vote_sets(pcld, kp_of, mask, frame_of, class_of, keep=keep)
    kcenters, _, _, rounds = mean_shift(ksets, kcounts, radius, max_iter, sets_per_count=n_kps, want_labels=False)
    if stats is not None:
        stats["rounds_kps"], stats["counts_kps"] = rounds, kcounts
    model, found = _model_and_found(mesh_kps, mesh_ctr, class_of, kcenters, centers)
    T = _fit(model, found, n_kps, use_ctr)
    if refine is not None:
        from . import refine as _refine
        opts = dict(refine)
        T, rstats = _refine.icp_refine(pcld, mask_given, T, frame_of, class_of, opts.pop("models"), **opts)
        if stats is not None:
            stats["refine"] = rstats

    empty = (counts == 0).cpu().numpy()
    T = T.cpu().numpy()
    found = found.cpu().numpy()
    T[empty] = np.identity(4)[:3, :]
    found[empty] = 0
    out = []
    for b in range(B):
        sel = frame_np == b
        out.append((class_np[sel].astype(np.int64), T[sel], found[sel]))
    return out


def _frame_class_pairs(mask, classes, B, n_cls):
    """(frame, class) pairs as solve_poses forms them: classes=None reads the classes present per frame back from the mask."""
    if classes is None:
        present = torch.zeros((B, n_cls), dtype=torch.bool, device=mask.device)
        present.scatter_(1, mask.clamp(0, n_cls - 1).long(), True)
        present[:, 0] = False
        present = present.cpu().numpy()
        per_frame = [np.nonzero(present[b])[0] for b in range(B)]
    else:
        per_frame = [np.asarray(classes, np.int64) for _ in range(B)]
    frame_np = np.concatenate([np.full(len(c), b, np.int32) for b, c in enumerate(per_frame)]) if B else np.zeros(0, np.int32)
    class_np = np.concatenate(per_frame).astype(np.int32) if B else np.zeros(0, np.int32)
    return frame_np, class_np


def solve_instances(pcld, mask, ctr_of, kp_of, mesh_kps, mesh_ctr, max_instances, min_inside=1, min_fraction=0.0, classes=None,
                    use_ctr=True, radius=RADIUS, max_iter=300, stats=None, **unsupported):
    """Every instance of every class of every frame, scored: the centre votes of a (frame, class) pair go through
    `mean_shift_multi` (up to max_instances centre clusters, largest first), every cluster becomes an estimate whose keypoint
    votes are those of the points whose centre vote lies in the cluster.  Inputs as solve_poses.
      max_instances  1 .. 255: cap per (frame, class);  min_inside: smallest centre cluster (in votes) that is an instance;
      min_fraction   drops instances whose score is below it.
    Returns a dict of DEVICE tensors, rows ordered by (frame, class, instance):
      est_RT f64 [E,3,4], est_class / est_frame / est_instance i32 [E] (instance ids 1..), est_score f32 [E],
      kps f32 [E,n_kps+1,3] (keypoints, then the centre), n_inside i32 [E]
    -- est_RT, est_class, est_frame, est_score are what bop.BOPSceneEval.add_batch takes.
    est_score = n_inside / (points of the class in the frame): the share of the class's centre votes that agree on the
    instance, in (0, 1]; the scores of a (frame, class) sum to at most 1.  Computed on the device.
    One read-back: the table of valid (pair, cluster) slots is turned into row indices (torch.nonzero), which sizes E -- after
    the centre pass, before the keypoint votes are gathered.  (classes=None reads the present classes back first, as solve_poses.)
    Not done here, because solve_poses ties both to ONE instance per class: the cross-class centre mask filter (`refine_mask`;
    one centre per pair) and ICP refinement (`refine=`; refine.icp_refine selects its scene points by class).  Passing either
    raises; solve_instances_refined has the instance-aware form of both."""
    if unsupported:
        raise TypeError(f"solve_instances does not take {sorted(unsupported)}: the centre mask filter and ICP refinement are "
                        "defined for one instance per class (use solve_poses, or solve_instances_refined)")
    return _solve_instances(pcld, mask, ctr_of, kp_of, mesh_kps, mesh_ctr, max_instances, min_inside, min_fraction, classes, use_ctr,
                            radius, max_iter, stats)


def solve_instances_refined(pcld, mask, ctr_of, kp_of, mesh_kps, mesh_ctr, max_instances, refine=None, min_inside=1, min_fraction=0.0,
                            classes=None, use_ctr=True, radius=RADIUS, max_iter=300, stats=None, refine_mask=False, r_lst=None):
    """`solve_instances` with the two steps it leaves out, both instance-aware.  Arguments as solve_instances, and
      refine: None, or dict(models=refine.PreparedModels, mode="nearest" | "map", max_iter=..., max_dist=..., [tol, min_pairs, metric,
              min_eig]; metric="plane" needs models prepared with normals and takes fewer iterations, see refine.icp_refine):
              the fitted poses go through ONE refine.icp_refine_instances call with the instance map the solver has ("nearest",
              the default: the instances of a (frame, class) compete for every point of the class, also those whose centre vote
              fell in no cluster; "map": every instance keeps the points of its centre cluster).  The keypoints stay as fitted.
      refine_mask=True, r_lst: the cross-class centre mask filter of solve_poses (:83-108) with one row per centre cluster: a
              first centre pass finds the clusters of the given mask, every foreground point goes to the class of the nearest
              cluster centre within 0.8 radii, and the solver runs on that mask (ICP included).  The first pass sizes its rows
              with a second read-back of the same kind as the one below (torch.nonzero on the table of valid slots).
    Returns the dict of solve_instances with est_RT refined, and
      est_RT_fit f64 [E,3,4] the fitted poses, icp_pairs i32 [E] / icp_rms f32 [E] / icp_iters i32 [E] (zero without `refine`),
      inst u8 [B,N]: the instance map as ICP left it (refine.icp_refine_instances), or the centre-cluster map without `refine`.
    est_score stays the vote share.  With `refine` no read-back is added to the one solve_instances makes."""
    return _solve_instances(pcld, mask, ctr_of, kp_of, mesh_kps, mesh_ctr, max_instances, min_inside, min_fraction, classes, use_ctr,
                            radius, max_iter, stats, refined=True, refine=refine, refine_mask=refine_mask, r_lst=r_lst)


def _instance_rows(n_in, n_clus, counts, K, min_fraction):
    """the valid (pair, cluster) slots as row indices, in (pair, cluster) order, and the scores [P,K]; torch.nonzero reads back"""
    score = n_in.float() / counts.clamp(min=1).float()[:, None]
    valid = (torch.arange(K, device=n_in.device)[None, :] < n_clus[:, None]) & (score >= float(min_fraction))
    pk = valid.nonzero()
    return pk[:, 0], pk[:, 1], score


def _solve_instances(pcld, mask, ctr_of, kp_of, mesh_kps, mesh_ctr, max_instances, min_inside, min_fraction, classes, use_ctr, radius,
                     max_iter, stats, refined=False, refine=None, refine_mask=False, r_lst=None):
    """The body of solve_instances and solve_instances_refined (`refined`: the keys of the latter)."""
    _need_gpu(pcld, mask, ctr_of, kp_of)
    B, N, _ = pcld.shape
    n_kps = kp_of.shape[1]
    dev = pcld.device
    K = int(max_instances)
    mesh_kps, mesh_ctr = _mesh_tensors(mesh_kps, mesh_ctr, dev)
    mask = mask.contiguous()
    frame_np, class_np = _frame_class_pairs(mask, classes, B, mesh_kps.shape[0])
    P = len(class_np)
    i32 = lambda n: torch.zeros((n,), dtype=torch.int32, device=dev)                                                        # noqa: E731
    empty = dict(est_RT=torch.zeros((0, 3, 4), dtype=torch.float64, device=dev), est_class=i32(0), est_frame=i32(0), est_instance=i32(0),
                 est_score=torch.zeros((0,), dtype=torch.float32, device=dev),
                 kps=torch.zeros((0, n_kps + 1, 3), dtype=torch.float32, device=dev), n_inside=i32(0))
    if refined:
        empty.update(est_RT_fit=empty["est_RT"], icp_pairs=i32(0), icp_rms=empty["est_score"], icp_iters=i32(0),
                     inst=torch.zeros((B, N), dtype=torch.uint8, device=dev))
    if P == 0:
        return empty
    frame_of, class_of = _i32(frame_np, dev), _i32(class_np, dev)
    ctr_of = ctr_of.contiguous().float()
    pcld = pcld.contiguous().float()

    if refine_mask:
        # 0. the centre clusters of the given mask, one row each, decide the class of every foreground point
        if r_lst is None:
            raise ValueError("refine_mask needs r_lst (object radii, common.py:89-94)")
        sets, counts = vote_sets(pcld, ctr_of, mask, frame_of, class_of)
        centers, _, n_in, n_clus, rounds = mean_shift_multi(sets, counts, radius, K, min_inside, max_iter)
        if stats is not None:
            stats["rounds_refine"], stats["counts_refine"] = rounds, counts
        p_of, k_of, _ = _instance_rows(n_in, n_clus, counts, K, min_fraction)
        row_class = class_of[p_of]
        per_frame = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
        per_frame.index_add_(0, frame_of[p_of].long() + 1, torch.ones_like(p_of))
        row_begin = per_frame.cumsum(0).int()
        row_dist = _gate_distances(r_lst, row_class, class_np, dev)                # per row from device radii, per pair from host radii
        if not _on_device(r_lst):
            row_dist = row_dist[p_of]
        mask = _refine_mask(pcld, ctr_of, mask, centers[p_of, k_of].contiguous(), row_class, row_begin, row_dist)

    # 1. centre clusters of every (frame, class)
    sets, counts = vote_sets(pcld, ctr_of, mask, frame_of, class_of)
    centers, cluster, n_in, n_clus, rounds = mean_shift_multi(sets, counts, radius, K, min_inside, max_iter)
    if stats is not None:
        stats["rounds_ctr"], stats["counts_ctr"], stats["n_clusters"] = rounds, counts, n_clus
    # 2. instance id of every point
    inst = instance_map(sets, cluster, counts, frame_of, B, N)
    # 3. one row per found instance (the sizes do not increase along k: the kept slots of a pair are a prefix)
    p_of, k_of, score = _instance_rows(n_in, n_clus, counts, K, min_fraction)       # the read-back that sizes E
    E = int(p_of.shape[0])
    if E == 0:
        return dict(empty, inst=inst) if refined else empty
    est_frame, est_class, est_instance = frame_of[p_of], class_of[p_of], (k_of + 1).int()
    ksets, kcounts = vote_sets_inst(pcld, kp_of, mask, inst, est_frame, est_class, est_instance)
    kcenters, _, _, rounds = mean_shift(ksets, kcounts, radius, max_iter, sets_per_count=n_kps, want_labels=False)
    if stats is not None:
        stats["rounds_kps"], stats["counts_kps"] = rounds, kcounts
    model, found = _model_and_found(mesh_kps, mesh_ctr, est_class, kcenters, centers[p_of, k_of])
    T = _fit(model, found, n_kps, use_ctr)
    out = dict(est_RT=T, est_class=est_class, est_frame=est_frame, est_instance=est_instance, est_score=score[p_of, k_of],
               kps=found, n_inside=n_in[p_of, k_of])
    if not refined:
        return out
    out.update(est_RT_fit=T, icp_pairs=i32(E), icp_rms=torch.zeros((E,), dtype=torch.float32, device=dev), icp_iters=i32(E), inst=inst)
    if refine is not None:
        from . import refine as _refine
        opts = dict(refine)
        opts.setdefault("mode", "nearest")
        T, rstats = _refine.icp_refine_instances(pcld, mask, inst, T, est_frame, est_class, est_instance, opts.pop("models"), **opts)
        out.update(est_RT=T, icp_pairs=rstats["n_pairs"], icp_rms=rstats["rms"], icp_iters=rstats["iters"], inst=rstats["inst"])
    return out


def cal_frame_poses_lm(pcld, mask, ctr_of, pred_kp_of, use_ctr, n_cls, use_ctr_clus_flter, obj_id,
                       debug=False, mesh_kps=None, mesh_ctr=None):
    """Signature of pvn3d_eval_utils_kpls.py:220-285 plus the mesh keypoints of `obj_id`
    (mesh_kps [n_kps,3], mesh_ctr [3]) the reference loads from its dataset files (:277-280).
    pcld [N,3], mask [N], ctr_of [1,N,3], pred_kp_of [n_kps,N,3] -> [pose [3,4]]."""
    if mesh_kps is None or (use_ctr and mesh_ctr is None):
        raise ValueError("mesh_kps / mesh_ctr of the object are required")
    n_kps = pred_kp_of.shape[0]
    kps = np.zeros((2, n_kps, 3), np.float32)
    kps[1] = mesh_kps
    ctr = np.zeros((2, 3), np.float32)
    if mesh_ctr is not None:
        ctr[1] = np.asarray(mesh_ctr).reshape(3)
    res = solve_poses(pcld[None], mask[None], ctr_of[None], pred_kp_of[None], kps, ctr, use_ctr=use_ctr,
                      use_ctr_clus_flter=use_ctr_clus_flter, refine_mask=False, classes=[1])
    return [res[0][1][0]]


def cal_frame_poses(pcld, mask, ctr_of, pred_kp_of, use_ctr, n_cls, use_ctr_clus_flter, gt_kps=None, gt_ctrs=None,
                    debug=False, kp_type='farthest', mesh_kps=None, mesh_ctr=None, r_lst=None):
    """Signature of pvn3d_eval_utils_kpls.py:65-158 plus mesh_kps [n_cls,n_kps,3], mesh_ctr [n_cls,3]
    (row = class id) and r_lst.  Returns (pred_cls_ids, pred_pose_lst, pred_kps_lst)."""
    if mesh_kps is None or mesh_ctr is None:
        raise ValueError("mesh_kps / mesh_ctr are required")
    ids, poses, kps = solve_poses(pcld[None], mask[None], ctr_of[None], pred_kp_of[None], mesh_kps, mesh_ctr,
                                  r_lst=r_lst, use_ctr=use_ctr, use_ctr_clus_flter=use_ctr_clus_flter)[0]
    return ids, [p for p in poses], [k for k in kps]
