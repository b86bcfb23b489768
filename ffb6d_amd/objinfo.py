"""Object info from mesh vertices on the GPU: farthest-point-sampled keypoints, bounding-box corners, centre and radius -- what
the reference's offline tool writes to text files (utils/dataset_tools/gen_obj_info.py:92-117, read back by
Basic_Utils.get_kps / get_ctr) and what pose.solve_poses, train_data.pose_targets, refine.PreparedModels and evaluate take as
arguments.  Host side of include/ffb6d_fps.h, which states the sampling rule (the reference's, quirks included);
tests/fps_ref.py is the numpy restatement the kernels are held against, bit for bit.

    meshes = render.PreparedMeshes([...])                                             # or an evaluate.ModelPoints
    info = objinfo.ObjectInfo.from_points(meshes, n_keypoints=8, n_model_points=2000)
    pose.solve_poses(..., info.mesh_kps, info.mesh_ctr, r_lst=info.r_lst)             # device tensors, by class id
    refine.PreparedModels(info.models)

Everything but ObjectInfo.save_txt enqueues its kernels on the current stream and returns device tensors: nothing is read back
and the stream is never waited for.  There is no CPU fallback: tensors must live on a GPU.
"""
import os

import numpy as np
import torch

from . import _lib
from .evaluate import ModelPoints
from .ops import _need_gpu, _stream
from .render import PreparedMeshes

FORM = 0               # csrc/fps.hip ffb6d_fps_set_form: 0 = automatic (resident up to its capacity, streaming above), 1 = resident, 2 = streaming


def set_form(form):
    """0 automatic (default) / 1 resident / 2 streaming; returns the previous setting.  Results do not depend on it."""
    global FORM
    form = int(form)
    if form not in (0, 1, 2):
        raise ValueError(f"form must be 0 (automatic), 1 (resident) or 2 (streaming), got {form}")
    prev, FORM = FORM, form
    _lib.load().ffb6d_fps_set_form(FORM)
    return prev


def resident_capacity():
    """Points of a set that the resident form holds."""
    return int(_lib.load().ffb6d_fps_resident_capacity())


class _Sets:
    """Point sets in the layout of the C ABI: pts f32 [>= total,3], begin i64 [S+1] on the device, sizes on the host."""
    __slots__ = ("pts", "begin", "S", "total", "max_n", "counts", "single", "device")


def _sets(points):
    """A ModelPoints, a PreparedMeshes (its vertices), a device tensor [N,3] or [S,N,3], or host data (numpy / lists, checked
    for non-finite values and uploaded) of those shapes.  A CPU tensor is refused, as everywhere in the library."""
    s = _Sets()
    s.single = False
    if isinstance(points, ModelPoints):
        s.pts, s.begin, s.counts = points.pts, points.begin, np.asarray(points.counts, np.int64)
    elif isinstance(points, PreparedMeshes):
        s.pts, s.begin, s.counts = points.verts, points.vert_begin, np.asarray(points.n_verts, np.int64)
    else:
        if torch.is_tensor(points):
            shape, dtype = tuple(points.shape), points.dtype
        else:
            points = np.asarray(points)
            shape, dtype = points.shape, points.dtype
        if len(shape) not in (2, 3) or shape[-1] != 3:
            raise ValueError(f"points must be [N,3] or [S,N,3], got {tuple(shape)}")
        if len(shape) == 3 and shape[0] < 1:
            raise ValueError(f"points must hold at least one set, got {tuple(shape)}")
        if torch.is_tensor(points):
            if not dtype.is_floating_point:
                raise TypeError(f"points must be floating point, got {dtype}")
            _need_gpu(points)
            pts = points.detach().to(torch.float32)
        else:
            if points.dtype.kind != "f":
                raise TypeError(f"points must be floating point, got {dtype}")
            host = np.ascontiguousarray(points, np.float32)
            if not np.isfinite(host).all():
                raise ValueError("points holds values that are not finite")
            if not torch.cuda.is_available():
                raise _lib.FFB6DNativeError("ffb6d_amd.objinfo runs on the GPU only; there is no CPU fallback")
            pts = torch.from_numpy(host).cuda()
        s.single = len(shape) == 2
        S, N = (1, shape[0]) if s.single else shape[:2]
        s.pts = pts.reshape(-1, 3).contiguous()
        s.counts = np.full(S, N, np.int64)
        s.begin = torch.arange(S + 1, dtype=torch.int64, device=s.pts.device) * N             # made on the device: no copy to wait for
    _need_gpu(s.pts, s.begin)
    s.S, s.total, s.max_n = len(s.counts), int(s.counts.sum()), int(s.counts.max())
    s.device = s.pts.device
    return s


def _start(start, s):
    """"center" -> None (the reference's init_center mode); an int or [S] integers -> i32 [S] on the device."""
    if isinstance(start, str):
        if start != "center":
            raise ValueError(f'start must be an index, [S] indices or "center", got {start!r}')
        return None
    if torch.is_tensor(start):
        if start.dtype.is_floating_point or start.numel() != s.S:
            raise ValueError(f"start must hold {s.S} integers, got {start.dtype} {tuple(start.shape)}")
        _need_gpu(start)
        return start.to(device=s.device, dtype=torch.int32).reshape(-1).contiguous()
    a = np.asarray(start)
    if a.dtype.kind not in "iu" or a.size not in (1, s.S):
        raise ValueError(f"start must be an index or {s.S} of them, got {a.dtype} {a.shape}")
    one = a.size == 1
    a = np.broadcast_to(a.reshape(-1), (s.S,)).astype(np.int64)
    if (a < 0).any() or ((a >= s.counts) & (s.counts > 0)).any():          # an empty set has no first pick to name
        raise ValueError("start names no point of its set")
    if one:                                                                # a fill on the device: no copy to wait for
        return torch.full((s.S,), int(a[0]), dtype=torch.int32, device=s.device)
    return torch.from_numpy(a.astype(np.int32)).to(s.device)


def _samples(m, what="m"):
    if int(m) != m or int(m) < 1:
        raise ValueError(f"{what} must be an integer of at least 1, got {m}")
    return int(m)


def _fps(s, m, start, want_dist):
    m = _samples(m)
    if s.max_n >= 1 << 31:
        raise ValueError(f"{s.max_n} points in a set, at most 2^31 - 1")
    start = _start(start, s)
    dev = s.device
    idx = torch.empty((s.S, m), dtype=torch.int32, device=dev)
    out = torch.empty((s.S, m, 3), dtype=torch.float32, device=dev)
    dist = torch.empty((s.S, m), dtype=torch.float32, device=dev) if want_dist else None
    lib = _lib.load()
    lib.ffb6d_fps_set_form(FORM)
    wbytes = lib.ffb6d_fps_workspace_bytes(s.S, s.max_n, m)
    ws = torch.empty((max(wbytes, 1),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _lib.traced("fps", 16 * s.total * m, (s.S, s.max_n, m)):
        rc = lib.ffb6d_fps_f32(s.pts.data_ptr(), s.begin.data_ptr(), s.S, s.total, s.max_n, m,
                               start.data_ptr() if start is not None else None, idx.data_ptr(), out.data_ptr(),
                               dist.data_ptr() if want_dist else None, ws.data_ptr(), wbytes, _stream(idx))
    _lib.check(rc, "ffb6d_fps_f32")
    return idx, out, dist


def farthest_point_sampling(points, m, start=0, return_dist=False):
    """m farthest-point samples of every set (include/ffb6d_fps.h states the rule: the reference's
    fps/src/farthest_point_sampling.cpp, index sequences identical to it).
      points: an evaluate.ModelPoints, a render.PreparedMeshes (its vertices), a device tensor [N,3] or a dense batch [S,N,3];
              host arrays of those shapes are checked for non-finite values and uploaded.
      start:  the first pick -- an index, [S] indices (host or device) -- or "center": the reference's init_center mode, whose
              first pick is the point farthest from the centre of the bounding box.  The reference's own default start is
              `rand() % n` seeded from the clock; hand such an index in to replay it.
    Returns (idx i32 [S,m] indices within the set, pts f32 [S,m,3]) on the device, and with return_dist also dist f32 [S,m]:
    the squared distance to the earlier picks that each pick was chosen by.  An empty set gives idx -1 and zeros.  For an
    [N,3] input the results are [m], [m,3] (, [m]): fps_utils.farthest_point_sampling(pts, sn, init_center)'s result plus the
    indices.  With m above the number of distinct points the picks go on with index 0, as the reference's do."""
    m = _samples(m)                                          # what the host can judge is judged before anything touches the device
    if isinstance(start, str) and start != "center":
        raise ValueError(f'start must be an index, [S] indices or "center", got {start!r}')
    s = _sets(points)
    idx, out, dist = _fps(s, m, start, return_dist)
    if s.single:
        idx, out, dist = idx[0], out[0], dist[0] if return_dist else None
    return (idx, out, dist) if return_dist else (idx, out)


def box_info(points):
    """Bounding-box statistics of every set (dataset_tools/utils.py:89-115): corners f32 [S,8,3] in get_3D_bbox's order, ctr f32
    [S,3] = (max + min) / 2, radius f32 [S] = half the box diagonal; zeros for an empty set.  `points` as in
    farthest_point_sampling; for an [N,3] input the results are [8,3], [3] and a scalar tensor."""
    s = _sets(points)
    dev = s.device
    corners = torch.empty((s.S, 8, 3), dtype=torch.float32, device=dev)
    ctr = torch.empty((s.S, 3), dtype=torch.float32, device=dev)
    radius = torch.empty((s.S,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _lib.traced("box_info", 12 * s.total, (s.S, s.total)):
        rc = _lib.load().ffb6d_box_info_f32(s.pts.data_ptr(), s.begin.data_ptr(), s.S, s.total, corners.data_ptr(), ctr.data_ptr(),
                                            radius.data_ptr(), _stream(corners))
    _lib.check(rc, "ffb6d_box_info_f32")
    return (corners[0], ctr[0], radius[0]) if s.single else (corners, ctr, radius)


def _model_points(s, n_model_points, start):
    """evaluate.ModelPoints of min(n_c, n_model_points) points per class in FPS order, assembled on the device.  A class with no
    more points than asked for keeps all of them, once each: its picks in the order of their first appearance (with duplicate
    points the picks fall back to index 0 before every index has been named), then the indices not picked, ascending."""
    m = min(_samples(n_model_points, "n_model_points"), max(s.max_n, 1))
    idx, out, _ = _fps(s, m, start, False)
    parts = []
    begin = np.concatenate([[0], np.cumsum(s.counts)])
    for c, n in enumerate(s.counts):
        n = int(n)
        if n > m:
            parts.append(out[c])
        elif n > 0:
            picks = idx[c].long()
            first = torch.full((n,), m, dtype=torch.int64, device=s.device)
            first.scatter_reduce_(0, picks, torch.arange(m, device=s.device), "amin")
            rest = m + torch.arange(n, device=s.device)
            order = torch.argsort(torch.where(first < m, first, rest))
            parts.append(s.pts[int(begin[c]):int(begin[c]) + n][order])
    models = ModelPoints.__new__(ModelPoints)
    models.n_cls, models.counts = s.S, np.minimum(s.counts, m).astype(np.int64)
    models.max_points, models.device = int(models.counts.max()), s.device
    models.pts = torch.cat(parts) if parts else torch.zeros((0, 3), dtype=torch.float32, device=s.device)
    models.begin = torch.from_numpy(np.concatenate([[0], np.cumsum(models.counts)]).astype(np.int64)).to(s.device)
    return models


class ObjectInfo:
    """What gen_obj_info.py computes per object, for a whole object set at once and by class id (row 0 = the background class
    of a PreparedMeshes: zeros), on the device:
      mesh_kps f32 [n_cls,n_kps,3], mesh_ctr f32 [n_cls,3]: as pose.solve_poses, pose.cal_frame_poses, train_data.pose_targets
        and train_data.assemble_training_batch take them;
      corners f32 [n_cls,8,3], radius f32 [n_cls]; r_lst f32 [n_cls-1] = radius[1:], the reference's r_lst[cls_id - 1];
      kps_idx i32 [n_cls,n_kps]: the keypoints' vertex indices within their class (-1 for an empty class);
      models: an evaluate.ModelPoints of the FPS subset of n_model_points per class (refine.PreparedModels and evaluate take
        it as it is), None when n_model_points is None."""

    def __init__(self, mesh_kps, mesh_ctr, corners, radius, kps_idx=None, models=None):
        self.mesh_kps, self.mesh_ctr, self.corners, self.radius = mesh_kps, mesh_ctr, corners, radius
        self.kps_idx, self.models = kps_idx, models
        self.r_lst = radius[1:]
        self.n_cls, self.n_kps = int(mesh_kps.shape[0]), int(mesh_kps.shape[1])

    @classmethod
    def from_points(cls, points, n_keypoints=8, n_model_points=None, start="center"):
        """points: a render.PreparedMeshes or an evaluate.ModelPoints.  start="center" (the reference's init_center mode) is a
        deliberate departure from gen_obj_info.py, whose call leaves the start to `rand() % n` seeded from the clock: the same
        mesh gives the same keypoints on every run.  Three launches (keypoints, box, model clouds) and no read-back."""
        if not isinstance(points, (PreparedMeshes, ModelPoints)):
            raise TypeError(f"points must be a render.PreparedMeshes or an evaluate.ModelPoints, got {type(points).__name__}")
        n_keypoints = _samples(n_keypoints, "n_keypoints")
        if n_model_points is not None:
            _samples(n_model_points, "n_model_points")
        s = _sets(points)
        idx, kps, _ = _fps(s, n_keypoints, start, False)
        corners, ctr, radius = box_info(points)
        models = _model_points(s, n_model_points, start) if n_model_points is not None else None
        return cls(kps, ctr, corners, radius, idx, models)

    def save_txt(self, directory, names):
        """Writes <name>_fps.txt, <name>_corners.txt, <name>_center.txt and <name>_radius.txt per class, in the format of
        gen_obj_info.py:98-117 (one point per line, three numbers separated by blanks; the radius alone on its line), so that
        Basic_Utils.get_kps(kp_pth=) / get_ctr(ctr_pth=) read them with np.loadtxt.  names: a list by class id (None = skip
        the class) or a dict {class id: name}.  The only call here that copies to the host (and waits for the device)."""
        if isinstance(names, dict):
            names = [names.get(c) for c in range(self.n_cls)]
        if len(names) != self.n_cls:
            raise ValueError(f"{len(names)} names for {self.n_cls} classes")
        kps, ctr = self.mesh_kps.cpu().numpy(), self.mesh_ctr.cpu().numpy()
        corners, radius = self.corners.cpu().numpy(), self.radius.cpu().numpy()
        os.makedirs(directory, exist_ok=True)
        written = []
        for c, name in enumerate(names):
            if name is None:
                continue
            for suffix, rows in (("fps", kps[c]), ("corners", corners[c]), ("center", ctr[c][None]), ("radius", radius[c].reshape(1, 1))):
                path = os.path.join(directory, f"{name}_{suffix}.txt")
                with open(path, "w") as of:
                    for row in rows:
                        print(*row, file=of)                 # numpy scalars print their shortest round-trip form, as the reference's do
                written.append(path)
        return written
