"""Object info from mesh vertices on the GPU: farthest-point-sampled keypoints, bounding-box corners, centre and radius -- what
the reference's offline tool writes to text files (utils/dataset_tools/gen_obj_info.py:92-117, read back by
Basic_Utils.get_kps / get_ctr) and what pose.solve_poses, train_data.pose_targets, refine.PreparedModels and evaluate take as
arguments.  Host side of include/ffb6d_fps.h, which states the sampling rule (the reference's, quirks included);
tests/fps_ref.py is the numpy restatement the kernels are held against, bit for bit.

    meshes = render.PreparedMeshes([...])                                             # or an evaluate.ModelPoints
    info = objinfo.ObjectInfo.from_points(meshes, n_keypoints=8, n_model_points=2000)
    pose.solve_poses(..., info.mesh_kps, info.mesh_ctr, r_lst=info.r_lst)             # device tensors, by class id
    refine.PreparedModels(info.models)

The reference's default keypoints (use_orbfps, common.py:71-73,129-131) are texture-aware: FPS over ORB corners of a few rendered
views, lifted into the object frame (gen_obj_info.py:119-125, rgbd_rnder_sift_kp3ds.py).  include/ffb6d_orb.h states the detector
(the published ORB detector in integers -- not OpenCV's bits) and the lift; tests/orb_ref.py restates them:

    info = objinfo.ObjectInfo.from_meshes(meshes, n_keypoints=8)                      # mesh_kps = FPS of the textured points
    info.n_found                                                                      # i32 [n_cls]: lifted points per class

Everything but ObjectInfo.save_txt enqueues its kernels on the current stream and returns device tensors: nothing is read back
and the stream is never waited for.  There is no CPU fallback: tensors must live on a GPU.
"""
import os

import numpy as np
import torch

from . import _lib
from .evaluate import ModelPoints
from .ops import _need_gpu, _stream
from .render import MAX_INSTANCES, PreparedMeshes, _prepared, render

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
    """A ModelPoints, a PreparedMeshes (its vertices), a TexturedPoints, a device tensor [N,3] or [S,N,3], or host data (numpy / lists, checked
    for non-finite values and uploaded) of those shapes.  A CPU tensor is refused, as everywhere in the library."""
    s = _Sets()
    s.single = False
    if isinstance(points, ModelPoints):
        s.pts, s.begin, s.counts = points.pts, points.begin, np.asarray(points.counts, np.int64)
    elif isinstance(points, PreparedMeshes):
        s.pts, s.begin, s.counts = points.verts, points.vert_begin, np.asarray(points.n_verts, np.int64)
    elif isinstance(points, TexturedPoints):                 # sizes live on the device: the host knows their bound alone
        s.pts, s.begin, s.counts = points.pts, points.begin, np.full(points.S, points.max_n, np.int64)
        s.S, s.total, s.max_n, s.device = points.S, int(points.pts.shape[0]), points.max_n, points.pts.device
        return s
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

# ---- texture-aware keypoints: view poses, the ORB detector, the lift (include/ffb6d_orb.h) ---------------------------------------
SPHERE_SCALE = 0.18 / 0.035        # the camera sphere's radius per object radius (rgbd_rnder_sift_kp3ds.py:148: r / 0.035 * 0.18)
DEFAULT_K = ((700.0, 0.0, 320.0), (0.0, 700.0, 240.0), (0.0, 0.0, 1.0))              # rgbd_rnder_sift_kp3ds.py:197
CHUNK_FRAMES = 32                  # frames rendered and searched at a time: their key image and candidate lists stay near 200 MB


def _unit_views(n1, n2):
    """R f64 [V,3,3], t f64 [V,3]: the object -> camera pose of every view for a camera sphere of radius 1.  Restates
    PoseUtils.CameraPositions, getCameraPose and get_o2c_pose_cv (dataset_tools/utils.py:225-255,353-395) with the identity
    object pose; the rotations do not depend on the sphere's radius and the translations are proportional to it."""
    theta = np.linspace(0.1, np.pi, n1 + 1)[:-1]
    phi = np.linspace(0, 2 * np.pi, n2 + 1)[:-1]
    flip = np.diag([1.0, -1.0, -1.0])                        # Blender camera -> computer-vision camera
    Rs, ts = [], []
    for th in theta:
        for ph in phi:
            loc = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
            z = loc / np.linalg.norm(loc)
            x = -np.cross(z, np.array([0.0, 0.0, 1.0]))
            x = x / np.linalg.norm(x)
            y = np.cross(z, x)
            y = y / np.linalg.norm(y)
            w2b = np.array([x, y, z])                        # the transpose of the camera pose's rotation
            Rs.append(flip @ w2b)
            ts.append(flip @ (-1 * w2b @ loc))
    return np.array(Rs), np.array(ts)


def view_poses(radius, n1=3, n2=3):
    """Object -> camera poses f64 [S,V,3,4] of the V = n1 * n2 views the reference renders an object of bounding-box radius
    `radius` from (rgbd_rnder_sift_kp3ds.py:138-156): cameras on a sphere of radius `radius * 0.18 / 0.035` looking at the
    origin, n1 polar angles from 0.1 rad by n2 azimuths.  radius: a number or [S] host values -> a numpy array; a device tensor
    [S] (box_info's) -> a device tensor, scaled on the device with nothing read back."""
    n1, n2 = _samples(n1, "n1"), _samples(n2, "n2")
    R, t = _unit_views(n1, n2)
    if torch.is_tensor(radius):
        _need_gpu(radius)
        dev = radius.device
        sph = radius.detach().reshape(-1).to(torch.float64) * SPHERE_SCALE
        poses = torch.empty((sph.shape[0], n1 * n2, 3, 4), dtype=torch.float64, device=dev)
        poses[..., :3] = torch.from_numpy(R).to(dev)
        poses[..., 3] = sph[:, None, None] * torch.from_numpy(t).to(dev)
        return poses
    sph = np.asarray(radius, np.float64).reshape(-1) * SPHERE_SCALE
    if not (np.isfinite(sph).all() and (sph >= 0).all()):
        raise ValueError("radius must be finite and not negative")
    poses = np.empty((len(sph), n1 * n2, 3, 4))
    poses[..., :3] = R
    poses[..., 3] = sph[:, None, None] * t
    return poses


def orb_quotas(n_features=500, n_levels=8):
    """Keypoints kept per pyramid level, as ORB shares n_features out (in double): i32 [n_levels] host values."""
    n_features, n_levels = int(n_features), int(n_levels)
    if n_features < 1 or not 1 <= n_levels <= 8:
        raise ValueError(f"n_features must be at least 1 and n_levels 1 .. 8, got {n_features}, {n_levels}")
    f = 1.0 / 1.2
    n = n_features * (1.0 - f) / (1.0 - f ** n_levels)
    out, total = [], 0
    for _ in range(n_levels - 1):
        out.append(int(round(n)))                            # round half to even
        total += out[-1]
        n *= f
    out.append(max(n_features - total, 0))
    return np.asarray(out, np.int32)


def _detector(n_features, n_levels, fast_threshold, edge):
    quota = orb_quotas(n_features, n_levels)
    fast_threshold, edge = int(fast_threshold), int(edge)
    if not 0 <= fast_threshold <= 255:
        raise ValueError(f"fast_threshold must be 0 .. 255, got {fast_threshold}")
    if not 4 <= edge <= 4096:
        raise ValueError(f"edge must be 4 .. 4096, got {edge}")
    return quota, int(n_levels), fast_threshold, edge


def _orb_detect(rgb, quota, n_levels, fast_threshold, edge):
    F, _, H, W = (int(v) for v in rgb.shape)
    Q = int(quota.sum())
    dev = rgb.device
    count = torch.empty((F,), dtype=torch.int32, device=dev)
    kps = torch.empty((F, Q, 5), dtype=torch.int32, device=dev)
    resp = torch.empty((F, Q), dtype=torch.int64, device=dev)
    lib = _lib.load()
    wbytes = lib.ffb6d_orb_workspace_bytes(F, H, W, n_levels)
    ws = torch.empty((max(wbytes, 1),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _lib.traced("orb_detect", 4 * F * H * W, (F, H, W, n_levels)):
        rc = lib.ffb6d_orb_detect_u8(rgb.data_ptr(), F, H, W, n_levels, fast_threshold, edge, quota.ctypes.data, count.data_ptr(),
                                     kps.data_ptr(), resp.data_ptr(), ws.data_ptr(), wbytes, _stream(kps))
    _lib.check(rc, "ffb6d_orb_detect_u8")
    return count, kps, resp


def orb_detect(rgb, n_features=500, n_levels=8, fast_threshold=20, edge=31):
    """The detector of include/ffb6d_orb.h on rgb u8 [F,3,H,W] frames (render's layout) on the device: FAST-9 corners on a 1.2x
    pyramid of n_levels levels, strict 8-neighbour maxima above fast_threshold at least `edge` pixels inside a level, ranked by
    an integer Harris response, the best orb_quotas(n_features, n_levels)[l] of level l kept.  It is the published ORB
    detector, not OpenCV's implementation: cv2.ORB's keypoints are not reproduced bit for bit.
    Returns (count i32 [F], kps i32 [F,Q,5] rows (x, y, level, X, Y) with (X, Y) the pixel of the full frame, resp i64 [F,Q]);
    Q = n_features unless the quotas round above it; rows past count[f] hold -1 / 0.  Nothing is read back."""
    if not torch.is_tensor(rgb) or rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[1] != 3:
        raise TypeError("rgb must be a uint8 device tensor [F,3,H,W]")
    _need_gpu(rgb)
    return _orb_detect(rgb.contiguous(), *_detector(n_features, n_levels, fast_threshold, edge))


class TexturedPoints:
    """The lifted ORB points of S objects in the layout of the C ABI: pts f32 [S*max_n,3] (zeros past the last point), begin i64
    [S+1] and n_found i32 [S] on the device; max_n = V*Q is the bound the host knows.  farthest_point_sampling takes it."""
    __slots__ = ("pts", "begin", "n_found", "S", "max_n")

    def __init__(self, pts, begin, n_found, max_n):
        self.pts, self.begin, self.n_found, self.S, self.max_n = pts, begin, n_found, int(n_found.shape[0]), int(max_n)


def textured_points(meshes, K=DEFAULT_K, H=480, W=640, n1=3, n2=3, min_pixels=500, n_features=500, n_levels=8, fast_threshold=20,
                    edge=31, radius=None):
    """The texture-aware 3-D points of every class of a mesh set (rgbd_rnder_sift_kp3ds.py:138-166): each object is rendered
    from view_poses(its box radius, n1, n2) with the intrinsics K (host data [3,3]), orb_detect runs on the frames, and the
    detected pixels are lifted through the rendered depth into the object frame (include/ffb6d_orb.h states the lift).  A view
    that shows fewer than min_pixels pixels of the object contributes nothing.  Frames are made and searched CHUNK_FRAMES at a
    time.  Returns a TexturedPoints by class id (class 0, the background, and classes without faces are empty sets); look at
    its n_found before trusting what is sampled from it.  Nothing is read back."""
    meshes = _prepared(meshes)
    n1, n2 = _samples(n1, "n1"), _samples(n2, "n2")
    H, W, V, S = int(H), int(W), n1 * n2, meshes.n_cls
    if V > MAX_INSTANCES:
        raise ValueError(f"{V} views per object, at most {MAX_INSTANCES}")
    if torch.is_tensor(K):
        raise TypeError("K must be host data [3,3]")
    K = np.asarray(K, np.float64)
    if K.shape != (3, 3) or not np.isfinite(K).all() or K[0, 0] == 0 or K[1, 1] == 0:
        raise ValueError("K must be a finite [3,3] matrix with focal lengths that are not zero")
    quota, n_levels, fast_threshold, edge = _detector(n_features, n_levels, fast_threshold, edge)
    Q = int(quota.sum())
    dev = meshes.device
    if radius is None:
        radius = box_info(meshes)[2]
    poses = view_poses(radius, n1, n2)
    slot_pts = torch.empty((S * V, Q, 3), dtype=torch.float32, device=dev)
    slot_ok = torch.empty((S * V, Q), dtype=torch.int32, device=dev)
    lib = _lib.load()
    step = max(1, min(MAX_INSTANCES, CHUNK_FRAMES) // V)
    for s0 in range(0, S, step):
        s1 = min(s0 + step, S)
        F = (s1 - s0) * V
        frame_of = torch.arange(F, dtype=torch.int32, device=dev)
        class_of = torch.arange(s0, s1, dtype=torch.int32, device=dev).repeat_interleave(V)
        T = poses[s0:s1].reshape(F, 3, 4).contiguous()
        out = render(meshes, T, frame_of, class_of, K, F, H, W, outputs=("rgb", "depth", "visible"))
        count, kps, _ = _orb_detect(out["rgb"], quota, n_levels, fast_threshold, edge)
        with torch.cuda.device(dev), _lib.traced("orb_lift", 20 * F * Q, (F, Q)):
            rc = lib.ffb6d_orb_lift_f32(kps.data_ptr(), count.data_ptr(), out["depth"].data_ptr(), out["visible"].data_ptr(), T.data_ptr(),
                                        F, Q, H, W, K[0, 0], K[1, 1], K[0, 2], K[1, 2], int(min_pixels), slot_pts[s0 * V:].data_ptr(),
                                        slot_ok[s0 * V:].data_ptr(), _stream(kps))
        _lib.check(rc, "ffb6d_orb_lift_f32")
    pts = torch.empty((S * V * Q, 3), dtype=torch.float32, device=dev)
    begin = torch.empty((S + 1,), dtype=torch.int64, device=dev)
    n_found = torch.empty((S,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev), _lib.traced("orb_compact", 32 * S * V * Q, (S, V, Q)):
        rc = lib.ffb6d_orb_compact_f32(slot_pts.data_ptr(), slot_ok.data_ptr(), S, V, Q, pts.data_ptr(), begin.data_ptr(),
                                       n_found.data_ptr(), _stream(pts))
    _lib.check(rc, "ffb6d_orb_compact_f32")
    return TexturedPoints(pts, begin, n_found, V * Q)


class ObjectInfo:
    """What gen_obj_info.py computes per object, for a whole object set at once and by class id (row 0 = the background class
    of a PreparedMeshes: zeros), on the device:
      mesh_kps f32 [n_cls,n_kps,3], mesh_ctr f32 [n_cls,3]: as pose.solve_poses, pose.cal_frame_poses, train_data.pose_targets
        and train_data.assemble_training_batch take them;
      corners f32 [n_cls,8,3], radius f32 [n_cls]; r_lst f32 [n_cls-1] = radius[1:], the reference's r_lst[cls_id - 1];
      kps_idx i32 [n_cls,n_kps]: the keypoints' vertex indices within their class (-1 for an empty class);
      models: an evaluate.ModelPoints of the FPS subset of n_model_points per class (refine.PreparedModels and evaluate take
        it as it is), None when n_model_points is None.  With model_normals=True, models.normals holds one estimated unit
        normal per model point (f32 [total,3]; refine.estimate_normals, the 16-neighbour rule of include/ffb6d_refine.h), so
        refine.PreparedModels(info.models, normals=info.models.normals) serves the point-to-plane metric; None otherwise.
    Built by from_meshes, mesh_kps holds the texture-aware keypoints (the reference's use_orbfps) and kps_idx is None; then also
      fps_kps f32 [n_cls,n_kps,3]: the plain FPS keypoints of the vertices; n_found i32 [n_cls]: the lifted ORB points per class;
      textured: the TexturedPoints they were sampled from.  All three are None otherwise."""

    def __init__(self, mesh_kps, mesh_ctr, corners, radius, kps_idx=None, models=None):
        self.mesh_kps, self.mesh_ctr, self.corners, self.radius = mesh_kps, mesh_ctr, corners, radius
        self.kps_idx, self.models = kps_idx, models
        self.r_lst = radius[1:]
        self.n_cls, self.n_kps = int(mesh_kps.shape[0]), int(mesh_kps.shape[1])
        self.fps_kps = self.n_found = self.textured = None

    @classmethod
    def from_points(cls, points, n_keypoints=8, n_model_points=None, start="center", model_normals=False):
        """points: a render.PreparedMeshes or an evaluate.ModelPoints.  start="center" (the reference's init_center mode) is a
        deliberate departure from gen_obj_info.py, whose call leaves the start to `rand() % n` seeded from the clock: the same
        mesh gives the same keypoints on every run.  Three launches (keypoints, box, model clouds) and no read-back.
        model_normals=True (needs n_model_points) also estimates the normals of the model clouds; that once waits for the device."""
        if not isinstance(points, (PreparedMeshes, ModelPoints)):
            raise TypeError(f"points must be a render.PreparedMeshes or an evaluate.ModelPoints, got {type(points).__name__}")
        n_keypoints = _samples(n_keypoints, "n_keypoints")
        if n_model_points is not None:
            _samples(n_model_points, "n_model_points")
        s = _sets(points)
        idx, kps, _ = _fps(s, n_keypoints, start, False)
        corners, ctr, radius = box_info(points)
        if model_normals and n_model_points is None:
            raise ValueError("model_normals needs n_model_points: the normals belong to the model clouds")
        models = _model_points(s, n_model_points, start) if n_model_points is not None else None
        if models is not None:
            models.normals = None
            if model_normals:
                from .refine import estimate_normals
                models.normals = estimate_normals(models)
        return cls(kps, ctr, corners, radius, idx, models)

    @classmethod
    def from_meshes(cls, meshes, n_keypoints=8, n_model_points=None, keypoints="orb_fps", start="center", model_normals=False, **views):
        """Everything from_points gives, with mesh_kps = the FPS of the meshes' textured_points: what gen_obj_info.py writes as
        <name>_ORB_fps.txt and what use_orbfps selects downstream.  meshes: a render.PreparedMeshes or the list it takes;
        **views: textured_points' arguments (K, H, W, n1, n2, min_pixels, n_features, n_levels, fast_threshold, edge).
        keypoints="fps" keeps the vertex keypoints (from_points' result).  The detector is the published ORB detector stated in
        include/ffb6d_orb.h, not OpenCV's: a checkpoint trained on the reference's keypoint files must keep using those files.
        A class with no lifted point gets the empty-set result of the FPS rule, zeros -- there is no fallback to the vertex
        keypoints: look at n_found (a device tensor, nothing is read back here) before using mesh_kps."""
        if keypoints not in ("orb_fps", "fps"):
            raise ValueError(f'keypoints must be "orb_fps" or "fps", got {keypoints!r}')
        meshes = _prepared(meshes)
        info = cls.from_points(meshes, n_keypoints, n_model_points, start, model_normals)
        if keypoints == "fps":
            return info
        tex = textured_points(meshes, radius=info.radius, **views)
        _, kps, _ = _fps(_sets(tex), n_keypoints, start, False)
        info.fps_kps, info.mesh_kps, info.kps_idx = info.mesh_kps, kps, None
        info.n_found, info.textured = tex.n_found, tex
        return info

    def save_txt(self, directory, names):
        """Writes <name>_fps.txt, <name>_corners.txt, <name>_center.txt and <name>_radius.txt per class, in the format of
        gen_obj_info.py:98-117 (one point per line, three numbers separated by blanks; the radius alone on its line), so that
        Basic_Utils.get_kps(kp_pth=) / get_ctr(ctr_pth=) read them with np.loadtxt.  names: a list by class id (None = skip
        the class) or a dict {class id: name}.  The only call here that copies to the host (and waits for the device).
        With texture-aware keypoints (from_meshes) <name>_fps.txt holds the vertex keypoints, and two more files hold mesh_kps:
        <name>_ORB_fps.txt (gen_obj_info.py:122) and <name>_<n_kps>_kps.txt, the name Basic_Utils.get_kps reads with use_orbfps
        (common.py:73,131)."""
        if isinstance(names, dict):
            names = [names.get(c) for c in range(self.n_cls)]
        if len(names) != self.n_cls:
            raise ValueError(f"{len(names)} names for {self.n_cls} classes")
        kps, ctr = self.mesh_kps.cpu().numpy(), self.mesh_ctr.cpu().numpy()
        orb = None
        if self.fps_kps is not None:
            orb, kps = kps, self.fps_kps.cpu().numpy()
        corners, radius = self.corners.cpu().numpy(), self.radius.cpu().numpy()
        os.makedirs(directory, exist_ok=True)
        written = []
        for c, name in enumerate(names):
            if name is None:
                continue
            files = [("fps", kps[c]), ("corners", corners[c]), ("center", ctr[c][None]), ("radius", radius[c].reshape(1, 1))]
            if orb is not None:
                files += [("ORB_fps", orb[c]), (f"{self.n_kps}_kps", orb[c])]
            for suffix, rows in files:
                path = os.path.join(directory, f"{name}_{suffix}.txt")
                with open(path, "w") as of:
                    for row in rows:
                        print(*row, file=of)                 # numpy scalars print their shortest round-trip form, as the reference's do
                written.append(path)
        return written
