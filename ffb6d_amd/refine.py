"""ICP pose refinement on the GPU: the step after the keypoint fit (pose.solve_poses), the second column of every published
FFB6D / PVN3D table.  Host side of include/ffb6d_refine.h, which states the algorithm (point-to-point, scene -> model, every
(frame, object) pair of a batch in the same launches); the reference repository has no counterpart -- tests/icp_ref.py is the
numpy restatement the kernels are held against.

    models = refine.PreparedModels(evaluate.ModelPoints(clouds))          # once per model set
    poses, stats = refine.icp_refine(pcld, mask, poses, frame_of, class_of, models, max_iter=10, max_dist=0.02)

The point-to-plane metric needs one normal per model point, prepared with the set, and reaches the noise floor in fewer iterations:

    models = refine.PreparedModels(evaluate.ModelPoints(clouds), normals="estimate")      # or a tensor f32 [total,3]
    poses, stats = refine.icp_refine(pcld, mask, poses, frame_of, class_of, models, max_iter=5, max_dist=0.02, metric="plane")

`icp_refine` and `correspondences` enqueue their kernels on the current stream and return device tensors: nothing is read
back and the stream is never waited for.  There is no CPU fallback: tensors must live on a GPU.
"""
import numpy as np
import torch

from . import _lib
from .ops import _need_gpu, _stream
from .pose import _mask_bits

FORM = 0               # csrc/icp.hip ffb6d_icp_set_form: 0 = scan (default), 1 = pruned, -1 = pruned from 1024 model points on


def set_form(form):
    """0 scan (default) / 1 pruned / -1 automatic; returns the previous setting.  Results do not depend on it."""
    global FORM
    prev, FORM = FORM, int(form)
    _lib.load().ffb6d_icp_set_form(FORM)
    return prev


class PreparedModels:
    """The model clouds of an evaluate.ModelPoints prepared for the search (Morton order, 64-point tiles with their boxes),
    once per model set.  Preparing copies the clouds to the host and back: it waits for the device.
      normals: None (the point metric only; asking such a set for the plane metric raises), "estimate" (from the clouds alone:
        16-neighbour PCA, the rule of include/ffb6d_refine.h) or a tensor f32 [total,3] in the clouds' own order (mesh vertex
        normals), each normalised once; a normal with a non-finite component or of zero length becomes the zero vector.
    `normals` (f32 [total,3]) reads the prepared normals back as a tensor."""

    def __init__(self, models, normals=None):
        _need_gpu(models.pts, models.begin)
        self.models, self.device = models, models.device
        self.n_cls, self.counts = int(models.n_cls), np.asarray(models.counts, np.int64)
        self.total = int(self.counts.sum())
        lib = _lib.load()
        nbytes = lib.ffb6d_icp_prepared_bytes(self.total, self.n_cls)
        self.buf = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            rc = lib.ffb6d_icp_prepare(models.pts.data_ptr() if self.total else None, models.begin.data_ptr(), self.n_cls, self.total,
                                       self.buf.data_ptr(), nbytes, _stream(self.buf))
        _lib.check(rc, "ffb6d_icp_prepare")
        self.normals_buf = None
        if normals is None:
            return
        nb = lib.ffb6d_icp_normals_bytes(self.total)
        self.normals_buf = torch.zeros((nb,), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            if isinstance(normals, str):
                if normals != "estimate":
                    raise ValueError(f"normals must be None, 'estimate' or a tensor [total,3], got {normals!r}")
                rc = lib.ffb6d_icp_estimate_normals_f32(models.pts.data_ptr() if self.total else None, models.begin.data_ptr(), self.n_cls,
                                                        self.total, self.normals_buf.data_ptr(), nb, _stream(self.buf))
                _lib.check(rc, "ffb6d_icp_estimate_normals_f32")
            else:
                given = normals if torch.is_tensor(normals) else torch.as_tensor(np.asarray(normals, np.float32))
                if tuple(given.shape) != (self.total, 3):
                    raise ValueError(f"normals must be [{self.total},3] (one per model point, the clouds' own order), got {tuple(given.shape)}")
                given = given.to(device=self.device, dtype=torch.float32).contiguous()
                rc = lib.ffb6d_icp_set_normals(given.data_ptr() if self.total else None, self.total, self.normals_buf.data_ptr(), nb,
                                               _stream(self.buf))
                _lib.check(rc, "ffb6d_icp_set_normals")

    @property
    def normals(self):
        """the prepared normals f32 [total,3] (a view of the buffer), or None"""
        if self.normals_buf is None:
            return None
        return self.normals_buf.view(torch.float32)[:4 * self.total].view(self.total, 4)[:, :3]


def estimate_normals(models):
    """One unit normal per model point of an evaluate.ModelPoints, from the clouds alone: the 16-neighbour PCA rule of
    include/ffb6d_refine.h (exact search, double covariance, sign by the largest component) -> f32 [total,3] on the device, the
    zero vector where a class has fewer than three points or a neighbourhood lies on a line.  Once per model set: it waits for
    the device."""
    _need_gpu(models.pts, models.begin)
    total = int(np.asarray(models.counts, np.int64).sum())
    lib = _lib.load()
    nb = lib.ffb6d_icp_normals_bytes(total)
    buf = torch.zeros((nb,), dtype=torch.uint8, device=models.device)
    with torch.cuda.device(models.device):
        rc = lib.ffb6d_icp_estimate_normals_f32(models.pts.data_ptr() if total else None, models.begin.data_ptr(), int(models.n_cls), total,
                                                buf.data_ptr(), nb, _stream(buf))
    _lib.check(rc, "ffb6d_icp_estimate_normals_f32")
    return buf.view(torch.float32)[:4 * total].view(total, 4)[:, :3]


def _prepared(models):
    return models if isinstance(models, PreparedModels) else PreparedModels(models)


def _problems(pcld, mask, poses, frame_of, class_of, models, keep):
    """Validates what the host can see and brings every argument into the layout of the C ABI."""
    _need_gpu(pcld, mask)
    for t in (poses, frame_of, class_of, keep):
        if torch.is_tensor(t):
            _need_gpu(t)
    if pcld.dim() != 3 or pcld.shape[2] != 3 or mask.shape != pcld.shape[:2]:
        raise ValueError(f"expected pcld [B,N,3] and mask [B,N], got {tuple(pcld.shape)} / {tuple(mask.shape)}")
    dev = pcld.device
    if models.device != dev:
        raise ValueError(f"models live on {models.device}, the cloud on {dev}")
    B = pcld.shape[0]
    for name, ids, hi in (("frame_of", frame_of, B), ("class_of", class_of, models.n_cls)):
        if not torch.is_tensor(ids):                            # host-visible ids are checked here; device ids that are no index
            a = np.asarray(ids).reshape(-1)                     # give a problem without pairs (include/ffb6d_refine.h)
            if len(a) and (a.min() < 0 or a.max() >= hi):
                raise ValueError(f"{name} outside [0, {hi})")
    as_i32 = lambda x: (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, np.int32).reshape(-1))).to(       # noqa: E731
        device=dev, dtype=torch.int32).reshape(-1).contiguous()
    frame_of, class_of = as_i32(frame_of), as_i32(class_of)
    P = int(frame_of.shape[0])
    poses = poses if torch.is_tensor(poses) else torch.as_tensor(np.asarray(poses, np.float64))
    poses = poses.to(device=dev, dtype=torch.float64).reshape(-1, 3, 4).contiguous()
    if int(class_of.shape[0]) != P or int(poses.shape[0]) != P:
        raise ValueError(f"{P} frames / {int(class_of.shape[0])} classes / {int(poses.shape[0])} poses")
    if keep is not None:
        if keep.shape != mask.shape:
            raise ValueError(f"keep {tuple(keep.shape)} does not match mask {tuple(mask.shape)}")
        keep = keep.to(torch.uint8).contiguous()
    return pcld.contiguous().float(), mask.contiguous(), poses, frame_of, class_of, keep, P


def _pair_outputs(P, N, dev):                                   # idx, d2, counts
    return (torch.empty((P, N), dtype=torch.int32, device=dev), torch.empty((P, N), dtype=torch.float32, device=dev),
            torch.empty((P,), dtype=torch.int32, device=dev))


def _pose_outputs(P, dev):                                      # T, n_pairs, rms, iters
    return (torch.empty((P, 3, 4), dtype=torch.float64, device=dev), torch.empty((P,), dtype=torch.int32, device=dev),
            torch.empty((P,), dtype=torch.float32, device=dev), torch.empty((P,), dtype=torch.int32, device=dev))


METRICS = ("point", "plane")


def _plane_args(models, metric, min_eig):
    """the normals of a plane call; refuses what the host can see"""
    if metric not in METRICS:
        raise ValueError(f"metric must be 'point' or 'plane', got {metric!r}")
    if metric == "point":
        return None
    if models.normals_buf is None:
        raise ValueError("metric 'plane' needs model normals: PreparedModels(models, normals='estimate' or a tensor [total,3])")
    if not 0.0 <= float(min_eig) < 1.0:
        raise ValueError(f"min_eig must be in [0, 1), got {min_eig}")
    return models.normals_buf


def _workspace(nbytes, dev):
    return torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev), nbytes


def correspondences(pcld, mask, poses, frame_of, class_of, models, max_dist=float("inf"), keep=None):
    """One evaluation of steps 1-3: for the j-th scene point of problem p (the points of pcld[frame_of[p]] with
    mask == class_of[p], and keep != 0 when given, in index order) under poses[p] (f64 [P,3,4], model -> camera)
    -> idx i32 [P,N] (model point within the class; -1 where the pair is gated out or j is beyond the count),
       d2 f32 [P,N] (squared distance to it, kept or not; +inf beyond the count), counts i32 [P]."""
    models = _prepared(models)
    pcld, mask, poses, frame_of, class_of, keep, P = _problems(pcld, mask, poses, frame_of, class_of, models, keep)
    B, N, _ = pcld.shape
    dev = pcld.device
    idx, d2, counts = _pair_outputs(P, N, dev)
    lib = _lib.load()
    ws, wbytes = _workspace(lib.ffb6d_icp_workspace_bytes(P, N), dev)
    with torch.cuda.device(dev), _lib.traced("icp_correspond", 0, (P, N)):
        rc = lib.ffb6d_icp_correspond_f32(models.buf.data_ptr(), models.n_cls, models.total, pcld.data_ptr(), mask.data_ptr(),
                                          _mask_bits(mask), keep.data_ptr() if keep is not None else None, frame_of.data_ptr(),
                                          class_of.data_ptr(), poses.data_ptr(), P, B, N, N, float(max_dist), idx.data_ptr(),
                                          d2.data_ptr(), counts.data_ptr(), ws.data_ptr(), wbytes, _stream(pcld))
    _lib.check(rc, "ffb6d_icp_correspond_f32")
    return idx, d2, counts


def icp_refine(pcld, mask, poses, frame_of, class_of, models, max_iter=10, max_dist=0.02, tol=0.0, min_pairs=3, keep=None, metric="point",
               min_eig=1e-6):
    """The whole loop for P problems: pcld f32 [B,N,3], mask int32|int64 [B,N], poses [P,3,4] (model -> camera), frame_of /
    class_of [P], models a PreparedModels (or an evaluate.ModelPoints, prepared on the spot: that waits for the device).
      max_dist: gate in metres (inf keeps every pair); tol: early stop when an update moves no corner of the model's bounding
      box by more than this many metres (0 = always max_iter iterations); min_pairs: fewer kept pairs end the problem with
      the pose it has.
      metric: "point" (each scene point is pulled to its model point) or "plane" (to the tangent plane at it, so it may slide along
      the surface: fewer iterations; the models must have been prepared with normals).  min_eig (plane only): directions of the
      6 x 6 system whose eigenvalue is below min_eig times the largest are not moved (planes, spheres, cans keep what the data
      does not determine).
    -> (poses f64 [P,3,4], dict n_pairs i32 [P], rms f32 [P] (of the last iteration made, before its update), iters i32 [P];
    under the plane metric also rms_plane f32 [P], the root of the mean squared point-to-plane distance of those pairs),
    all on the device."""
    models = _prepared(models)
    normals = _plane_args(models, metric, min_eig)
    pcld, mask, poses, frame_of, class_of, keep, P = _problems(pcld, mask, poses, frame_of, class_of, models, keep)
    B, N, _ = pcld.shape
    dev = pcld.device
    T, n_pairs, rms, iters = _pose_outputs(P, dev)
    lib = _lib.load()
    if normals is not None:
        rms_plane = torch.empty((P,), dtype=torch.float32, device=dev)
        ws, wbytes = _workspace(lib.ffb6d_icp_plane_workspace_bytes(P, N), dev)
        with torch.cuda.device(dev), _lib.traced("icp_refine_plane", 0, (P, N, int(max_iter))):
            rc = lib.ffb6d_icp_refine_plane_f32(models.buf.data_ptr(), normals.data_ptr(), models.n_cls, models.total, pcld.data_ptr(),
                                                mask.data_ptr(), _mask_bits(mask), keep.data_ptr() if keep is not None else None,
                                                frame_of.data_ptr(), class_of.data_ptr(), poses.data_ptr(), P, B, N, N, float(max_dist),
                                                int(max_iter), float(tol), int(min_pairs), float(min_eig), T.data_ptr(), n_pairs.data_ptr(),
                                                rms.data_ptr(), rms_plane.data_ptr(), iters.data_ptr(), ws.data_ptr(), wbytes, _stream(pcld))
        _lib.check(rc, "ffb6d_icp_refine_plane_f32")
        return T, dict(n_pairs=n_pairs, rms=rms, iters=iters, rms_plane=rms_plane)
    ws, wbytes = _workspace(lib.ffb6d_icp_workspace_bytes(P, N), dev)
    with torch.cuda.device(dev), _lib.traced("icp_refine", 0, (P, N, int(max_iter))):
        rc = lib.ffb6d_icp_refine_f32(models.buf.data_ptr(), models.n_cls, models.total, pcld.data_ptr(), mask.data_ptr(),
                                      _mask_bits(mask), keep.data_ptr() if keep is not None else None, frame_of.data_ptr(),
                                      class_of.data_ptr(), poses.data_ptr(), P, B, N, N, float(max_dist), int(max_iter), float(tol),
                                      int(min_pairs), T.data_ptr(), n_pairs.data_ptr(), rms.data_ptr(), iters.data_ptr(),
                                      ws.data_ptr(), wbytes, _stream(pcld))
    _lib.check(rc, "ffb6d_icp_refine_f32")
    return T, dict(n_pairs=n_pairs, rms=rms, iters=iters)


# ---- several instances of a class in a frame ---------------------------------------------------------------------------
MODES = {"map": 0, "nearest": 1}


def _instance_problems(pcld, mask, inst, poses, frame_of, class_of, inst_of, models, mode, keep):
    """_problems, and the instance map / the instance ids in the layout of the C ABI"""
    if mode not in MODES:
        raise ValueError(f"mode must be 'map' or 'nearest', got {mode!r}")
    pcld, mask, poses, frame_of, class_of, keep, P = _problems(pcld, mask, poses, frame_of, class_of, models, keep)
    if inst is None:
        if mode == "map":
            raise ValueError("mode 'map' needs the instance map `inst` (u8 [B,N])")
    else:
        _need_gpu(inst)
        if inst.shape != mask.shape or inst.dtype != torch.uint8:
            raise ValueError(f"inst must be uint8 {tuple(mask.shape)}, got {inst.dtype} {tuple(inst.shape)}")
        inst = inst.contiguous()
    if torch.is_tensor(inst_of):
        _need_gpu(inst_of)
    else:
        inst_of = torch.as_tensor(np.asarray(inst_of, np.int32).reshape(-1))
    inst_of = inst_of.to(device=pcld.device, dtype=torch.int32).reshape(-1).contiguous()
    if int(inst_of.shape[0]) != P:
        raise ValueError(f"{P} problems / {int(inst_of.shape[0])} instance ids")
    return pcld, mask, inst, poses, frame_of, class_of, inst_of, keep, P


def correspondences_instances(pcld, mask, inst, poses, frame_of, class_of, inst_of, models, mode="map", max_dist=float("inf"), keep=None):
    """`correspondences` for problems (frame, class, instance) -- the rule is stated in include/ffb6d_refine.h.
      inst u8 [B,N]: the instance map (pose.instance_map; 0 = no instance), inst_of [P] the problems' instance ids;
      mode "map": the scene points of p are the class's points with inst == inst_of[p];
      mode "nearest": they are all points of the class (inst may be None), and the adjacent problems of one (frame, class)
           compete for each: the pair is kept only by the problem whose posed model is nearest.
    -> idx i32 [P,N] (-1 where the pair is gated out, not owned, or j is beyond the count), d2 f32 [P,N] (the problem's own
       smallest distance, owned or not), counts i32 [P], owner i32 [P,N] (index of the owning problem, -1 for none)."""
    models = _prepared(models)
    pcld, mask, inst, poses, frame_of, class_of, inst_of, keep, P = _instance_problems(pcld, mask, inst, poses, frame_of, class_of, inst_of,
                                                                                       models, mode, keep)
    B, N, _ = pcld.shape
    dev = pcld.device
    idx, d2, counts = _pair_outputs(P, N, dev)
    owner = torch.empty((P, N), dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws, wbytes = _workspace(lib.ffb6d_icp_inst_workspace_bytes(P, N, MODES[mode]), dev)
    with torch.cuda.device(dev), _lib.traced("icp_correspond_inst", 0, (P, N)):
        rc = lib.ffb6d_icp_correspond_inst_f32(models.buf.data_ptr(), models.n_cls, models.total, pcld.data_ptr(), mask.data_ptr(),
                                               _mask_bits(mask), keep.data_ptr() if keep is not None else None,
                                               inst.data_ptr() if inst is not None else None, frame_of.data_ptr(), class_of.data_ptr(),
                                               inst_of.data_ptr(), poses.data_ptr(), P, B, N, N, float(max_dist), MODES[mode],
                                               idx.data_ptr(), d2.data_ptr(), counts.data_ptr(), owner.data_ptr(), ws.data_ptr(), wbytes,
                                               _stream(pcld))
    _lib.check(rc, "ffb6d_icp_correspond_inst_f32")
    return idx, d2, counts, owner


def icp_refine_instances(pcld, mask, inst, poses, frame_of, class_of, inst_of, models, mode="map", max_iter=10, max_dist=0.02, tol=0.0,
                         min_pairs=3, keep=None, metric="point", min_eig=1e-6):
    """`icp_refine` for problems (frame, class, instance); inst / inst_of / mode as `correspondences_instances`.  In mode
    "nearest" a problem that has stopped keeps its pose and goes on competing for points until the loop ends.
    -> (poses f64 [P,3,4], dict n_pairs i32 [P], rms f32 [P], iters i32 [P], inst u8 [B,N]: the instance id of the problem that
    kept the point's pair at the end, 0 elsewhere -- in mode "nearest" the refined instance map), all on the device; nothing is
    read back.  metric / min_eig as `icp_refine`; the plane metric adds rms_plane f32 [P]."""
    models = _prepared(models)
    normals = _plane_args(models, metric, min_eig)
    pcld, mask, inst, poses, frame_of, class_of, inst_of, keep, P = _instance_problems(pcld, mask, inst, poses, frame_of, class_of, inst_of,
                                                                                       models, mode, keep)
    B, N, _ = pcld.shape
    dev = pcld.device
    T, n_pairs, rms, iters = _pose_outputs(P, dev)
    inst_out = torch.empty((B, N), dtype=torch.uint8, device=dev)
    lib = _lib.load()
    if normals is not None:
        rms_plane = torch.empty((P,), dtype=torch.float32, device=dev)
        ws, wbytes = _workspace(lib.ffb6d_icp_plane_inst_workspace_bytes(P, N, MODES[mode]), dev)
        with torch.cuda.device(dev), _lib.traced("icp_refine_plane_inst", 0, (P, N, int(max_iter))):
            rc = lib.ffb6d_icp_refine_plane_inst_f32(models.buf.data_ptr(), normals.data_ptr(), models.n_cls, models.total, pcld.data_ptr(),
                                                     mask.data_ptr(), _mask_bits(mask), keep.data_ptr() if keep is not None else None,
                                                     inst.data_ptr() if inst is not None else None, frame_of.data_ptr(),
                                                     class_of.data_ptr(), inst_of.data_ptr(), poses.data_ptr(), P, B, N, N, float(max_dist),
                                                     int(max_iter), float(tol), int(min_pairs), float(min_eig), MODES[mode], T.data_ptr(),
                                                     n_pairs.data_ptr(), rms.data_ptr(), rms_plane.data_ptr(), iters.data_ptr(),
                                                     inst_out.data_ptr(), ws.data_ptr(), wbytes, _stream(pcld))
        _lib.check(rc, "ffb6d_icp_refine_plane_inst_f32")
        return T, dict(n_pairs=n_pairs, rms=rms, iters=iters, inst=inst_out, rms_plane=rms_plane)
    ws, wbytes = _workspace(lib.ffb6d_icp_inst_workspace_bytes(P, N, MODES[mode]), dev)
    with torch.cuda.device(dev), _lib.traced("icp_refine_inst", 0, (P, N, int(max_iter))):
        rc = lib.ffb6d_icp_refine_inst_f32(models.buf.data_ptr(), models.n_cls, models.total, pcld.data_ptr(), mask.data_ptr(),
                                           _mask_bits(mask), keep.data_ptr() if keep is not None else None,
                                           inst.data_ptr() if inst is not None else None, frame_of.data_ptr(), class_of.data_ptr(),
                                           inst_of.data_ptr(), poses.data_ptr(), P, B, N, N, float(max_dist), int(max_iter), float(tol),
                                           int(min_pairs), MODES[mode], T.data_ptr(), n_pairs.data_ptr(), rms.data_ptr(),
                                           iters.data_ptr(), inst_out.data_ptr(), ws.data_ptr(), wbytes, _stream(pcld))
    _lib.check(rc, "ffb6d_icp_refine_inst_f32")
    return T, dict(n_pairs=n_pairs, rms=rms, iters=iters, inst=inst_out)
