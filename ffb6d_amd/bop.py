"""The BOP pose errors on the GPU: VSD (visible surface discrepancy), MSSD and MSPD (maximum symmetry-aware surface /
projection distance) and the average recall built from the three -- the numbers LM-O and YCB-V results are ranked by, next to the
ADD / ADD-S of ffb6d_amd.evaluate.  Host side of include/ffb6d_bop.h, which states the arithmetic in full; there is no BOP
toolkit to port, tests/bop_ref.py is the numpy restatement the kernels are held against, bit for bit.

    syms = bop.SymmetrySets([None, bop.symmetry_transforms(continuous=[((0, 0, 1), (0, 0, 0))]), ...])     # once, by class id
    mssd, mspd = bop.mssd_mspd(est_RT, gt_RT, class_of, frame_of, K, models, syms)                         # metres, pixels
    err, counts = bop.vsd(depth_test, est_RT, gt_RT, class_of, frame_of, K, meshes, diameters)             # [Q, n_tau]
    ev = bop.BOPEval(models, meshes, syms, diameters); ev.add_batch(...); ev.cal_ar()

BOPEval scores rows that are one estimate against its own ground truth.  A scene with several instances and several scored
estimates per object goes through the host side of include/ffb6d_bop_scene.h (restated by tests/bop_scene_ref.py):

    info = bop.instance_info(depth_test, gt_RT, gt_class, gt_frame, K, meshes)        # px counts, boxes, visib_fract per instance
    groups = bop.pair_rows(est_class, est_frame, gt_class, gt_frame)                  # host: (frame, class) groups and their pairs
    est_gt, gt_est = bop.match(err, score, groups, thr)                               # greedy by score, per error column and threshold
    ev = bop.BOPSceneEval(models, meshes, syms, diameters); ev.add_batch(...); ev.cal_ar()

The distance, visibility and matching calls enqueue their kernels on the current stream and return device tensors; nothing is
read back.  There is no CPU fallback: they are computed by the HIP library on a GPU, only the recall arithmetic is plain numpy
(like cal_auc) and the grouping of pair_rows is host bookkeeping on the ids.

Out of scope: BOP JSON / CSV input and output, the datasets' symmetry tables (models_info.json: the caller supplies the
transforms), and rendering each distinct pose once for VSD when a group has more than one pair: the E_g x T_g pairs of a group go
through `vsd` as independent rows, each rendering its two poses again.  Nothing here claims the bytes of the BOP toolkit's files.
"""
import math

import numpy as np
import torch

from . import _lib
from . import render as _render
from .ops import _need_gpu, _stream

MAX_TAUS = 16                                        # FFB6D_BOP_MAX_TAUS
MAX_ROWS = 65535                                     # rows of one library call (a grid dimension); the wrappers split larger batches
VSD_TAUS = np.arange(0.05, 0.51, 0.05)               # BOP19: 10 misalignment tolerances, fractions of the diameter
VSD_DELTA = 0.015                                    # BOP19: 15 mm visibility tolerance
VSD_THRESHOLDS = np.arange(0.05, 0.51, 0.05)         # correct when e < theta
MSSD_THRESHOLDS = np.arange(0.05, 0.51, 0.05)        # correct when e < theta * diameter
MSPD_THRESHOLDS = np.arange(5, 51, 5)                # correct when e < theta * (W / 640) pixels
CHUNK_PIXELS = 1 << 25                               # pixels rendered per vsd chunk: a key image of 256 MiB


def _numpy(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _as_Rt(s):
    if isinstance(s, (tuple, list)) and len(s) == 2:
        R, t = np.asarray(s[0], np.float64).reshape(3, 3), np.asarray(s[1], np.float64).reshape(3)
    else:
        m = np.asarray(s, np.float64).reshape(4, 4)
        R, t = m[:3, :3], m[:3, 3]
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        raise ValueError("a symmetry transform holds values that are not finite")
    return np.array(R), np.array(t)


def _is_identity(R, t):
    return np.array_equal(R, np.eye(3)) and not t.any()


def symmetry_transforms(discrete=(), continuous=(), max_disc_step=0.01):
    """The symmetry set of one object as a list of (R [3,3], t [3]) float64, model frame, identity first.  This is the project's
    own statement of the BOP rule (there is no toolkit here to compare with):
      discrete: 4 x 4 matrices (or (R, t) pairs); continuous: (axis, offset) pairs, a rotation by any angle about the line
      through `offset` along `axis`, discretised into n = ceil(pi / max_disc_step) steps of 2 pi i / n, i = 0 .. n-1, with
      R = Rodrigues(axis, angle) and t = offset - R @ offset.
    The result is every product (continuous after discrete: R = Rc Rd, t = Rc td + tc) of a continuous transform, or the identity
    when there is none, with the identity or a discrete transform; the identity comes first and exact copies of it are removed."""
    disc = [(np.eye(3), np.zeros(3))] + [_as_Rt(d) for d in discrete]
    cont = []
    for axis, offset in continuous:
        a, off = np.asarray(axis, np.float64).reshape(3), np.asarray(offset, np.float64).reshape(3)
        norm = np.linalg.norm(a)
        if not (norm > 0 and np.isfinite(off).all()) or not max_disc_step > 0:
            raise ValueError(f"bad continuous symmetry: axis {axis}, offset {offset}, max_disc_step {max_disc_step}")
        a = a / norm
        Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        n = int(math.ceil(math.pi / max_disc_step))
        for i in range(n):
            ang = 2.0 * math.pi * i / n
            R = np.eye(3) + math.sin(ang) * Kx + (1.0 - math.cos(ang)) * (Kx @ Kx)
            cont.append((R, off - R @ off))
    if not cont:
        cont = [(np.eye(3), np.zeros(3))]
    out = [(np.eye(3), np.zeros(3))]
    for Rd, td in disc:
        for Rc, tc in cont:
            R, t = Rc @ Rd, Rc @ td + tc
            if not _is_identity(R, t):
                out.append((R, t))
    return out


class SymmetrySets:
    """The symmetry transforms of every class, uploaded once: `transforms` is a list (index = class id) or a dict {class id: ...}
    of None (no symmetry) or a list of (R, t) pairs / 4 x 4 matrices, as symmetry_transforms returns them.  The identity is always
    entry 0 of a class (added when missing, exact copies of it removed).  Holds sym_R f64 [Stot,3,3], sym_t f64 [Stot,3] and
    begin i64 [n_cls+1] on `device`, and the host lists in `sets`."""

    def __init__(self, transforms, device=None, n_cls=None):
        if isinstance(transforms, dict):
            n = max([int(k) for k in transforms] + [-1]) + 1
            transforms = [transforms.get(c) for c in range(max(n, n_cls or 0))]
        transforms = list(transforms) + [None] * max(0, (n_cls or 0) - len(transforms))
        self.sets = []
        for tr in transforms:
            rest = [s for s in (_as_Rt(s) for s in (tr if tr is not None else [])) if not _is_identity(*s)]
            self.sets.append([(np.eye(3), np.zeros(3))] + rest)
        self.n_cls = len(self.sets)
        if self.n_cls == 0:
            raise ValueError("SymmetrySets needs at least one class")
        self.counts = np.array([len(s) for s in self.sets], np.int64)
        self.Stot, self.max_syms = int(self.counts.sum()), int(self.counts.max())
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        flat = [s for cls in self.sets for s in cls]
        self.sym_R = torch.from_numpy(np.stack([R for R, _ in flat])).to(self.device)
        self.sym_t = torch.from_numpy(np.stack([t for _, t in flat])).to(self.device)
        self.begin = torch.from_numpy(np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)).to(self.device)


def _device_array(x, dev, dtype, np_dtype):
    if torch.is_tensor(x):
        _need_gpu(x)
        return x.detach().to(device=dev, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np_dtype))).to(dev)


def _rows(est_RT, gt_RT, class_of, frame_of, K, dev):
    """-> est, gt f64 [Q,3,4], class_of, frame_of i32 [Q], K f64 [B,3,3] on dev"""
    est = _device_array(est_RT, dev, torch.float64, np.float64).reshape(-1, 3, 4)
    gt = _device_array(gt_RT, dev, torch.float64, np.float64).reshape(-1, 3, 4)
    cls = _device_array(class_of, dev, torch.int32, np.int32).reshape(-1)
    frm = _device_array(frame_of, dev, torch.int32, np.int32).reshape(-1)
    Kd = _device_array(K, dev, torch.float64, np.float64)
    if Kd.dim() == 2:
        Kd = Kd.unsqueeze(0)
    Kd = Kd.contiguous()
    if Kd.dim() != 3 or tuple(Kd.shape[1:]) != (3, 3) or Kd.shape[0] == 0:
        raise ValueError(f"K must be [3,3] or [B,3,3], got {tuple(Kd.shape)}")
    Q = int(cls.shape[0])
    if not (int(frm.shape[0]) == int(est.shape[0]) == int(gt.shape[0]) == Q):
        raise ValueError(f"{int(est.shape[0])} estimated / {int(gt.shape[0])} ground-truth poses for {Q} class ids and "
                         f"{int(frm.shape[0])} frame ids")
    return est, gt, cls, frm, Kd


def mssd2_mspd2(est_RT, gt_RT, class_of, frame_of, K, models, syms, outputs=("mssd", "mspd")):
    """The kernel's own outputs: the SQUARED errors as device float64 [Q] (None for an output that was not asked for)."""
    dev = models.device
    if models.n_cls != syms.n_cls:
        raise ValueError(f"{models.n_cls} classes of model points, {syms.n_cls} of symmetries")
    if not outputs or any(o not in ("mssd", "mspd") for o in outputs):
        raise ValueError(f"outputs must name 'mssd' and / or 'mspd', got {outputs}")
    _need_gpu(models.pts, syms.sym_R)
    est, gt, cls, frm, Kd = _rows(est_RT, gt_RT, class_of, frame_of, K, dev)
    Q = int(cls.shape[0])
    out = {o: torch.empty((Q,), dtype=torch.float64, device=dev) for o in outputs}
    lib = _lib.load()
    for q0 in range(0, Q, MAX_ROWS):                                             # the library takes MAX_ROWS rows a call
        n = min(MAX_ROWS, Q - q0)
        ptr = lambda o: out[o][q0:].data_ptr() if o in out else None                                                        # noqa: E731
        wbytes = lib.ffb6d_bop_mssd_mspd_workspace_bytes(n, models.max_points, syms.max_syms)
        ws = torch.empty((max(wbytes, 1),), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev), _lib.traced("bop_mssd_mspd", 0, (n, models.max_points, syms.max_syms)):
            rc = lib.ffb6d_bop_mssd_mspd_f64(models.pts.data_ptr(), models.begin.data_ptr(), models.n_cls, int(models.counts.sum()),
                                             models.max_points, syms.sym_R.data_ptr(), syms.sym_t.data_ptr(), syms.begin.data_ptr(),
                                             syms.Stot, syms.max_syms, cls[q0:].data_ptr(), frm[q0:].data_ptr(), est[q0:].data_ptr(),
                                             gt[q0:].data_ptr(), n, Kd.data_ptr(), int(Kd.shape[0]), ptr("mssd"), ptr("mspd"),
                                             ws.data_ptr(), wbytes, _stream(ws))
        _lib.check(rc, "ffb6d_bop_mssd_mspd_f64")
    return out.get("mssd"), out.get("mspd")


def mssd_mspd(est_RT, gt_RT, class_of, frame_of, K, models, syms):
    """MSSD and MSPD of Q (estimated, ground-truth) pose pairs in one call:
      est_RT, gt_RT [Q,3,4] (model -> camera; used as float64), class_of [Q] class ids into `models` (an evaluate.ModelPoints: BOP
      scores the mesh vertices) and `syms` (a SymmetrySets), frame_of [Q] into K ([B,3,3], or [3,3] for one camera): host data
      (uploaded) or device tensors.
    Returns device float64 tensors mssd [Q] in the models' unit (metres) and mspd [Q] in pixels: torch.sqrt of the kernel's squared
    errors.  A row whose class has no points, whose class or frame id is out of range or whose poses are not finite gives NaN;
    a point at or behind the camera plane under either pose makes the row's MSPD +inf.  A library call takes MAX_ROWS = 65535
    rows (a grid dimension); larger batches are split here."""
    s2, p2 = mssd2_mspd2(est_RT, gt_RT, class_of, frame_of, K, models, syms)
    return torch.sqrt(s2), torch.sqrt(p2)


def _taus(taus):
    t = np.ascontiguousarray(np.asarray(taus, np.float32).reshape(-1))
    if not 1 <= len(t) <= MAX_TAUS:
        raise ValueError(f"{len(t)} taus, between 1 and {MAX_TAUS} are taken")
    return t


def _taus_device(taus, dev):
    """taus on the device: host data is checked and uploaded; a float32 device tensor (vsd uploads once for all its chunks) is used as it is"""
    if torch.is_tensor(taus) and taus.is_cuda:
        if taus.dtype != torch.float32 or taus.dim() != 1 or not taus.is_contiguous() or not 1 <= int(taus.shape[0]) <= MAX_TAUS:
            raise ValueError(f"device taus must be a contiguous float32 [1..{MAX_TAUS}] tensor, got {taus.dtype} {tuple(taus.shape)}")
        return taus.to(dev)
    return torch.from_numpy(_taus(_numpy(taus))).to(dev)


def vsd_compare(depth_test, depth_est, depth_gt, class_of, frame_of, K, diameters, delta=VSD_DELTA, taus=VSD_TAUS, out=None):
    """The VSD kernel alone, on depth images that exist already: depth_test f32 [B,H,W], depth_est / depth_gt f32 [Q,H,W] (row q's
    model rendered alone under its two poses), device tensors; class_of / frame_of i32 [Q], K f64 [B,3,3], diameters f32 [n_cls]
    on the same device; taus: host data, or a float32 device tensor (no upload).  Q <= 65535.
    -> (vsd f64 [Q, n_tau], counts i32 [Q, 2 + n_tau]); `out`: that pair, to be written in place."""
    _need_gpu(depth_test, depth_est, depth_gt, class_of, frame_of, K, diameters)
    for name, t, dt in (("depth_test", depth_test, torch.float32), ("depth_est", depth_est, torch.float32), ("depth_gt", depth_gt, torch.float32),
                        ("class_of", class_of, torch.int32), ("frame_of", frame_of, torch.int32), ("K", K, torch.float64),
                        ("diameters", diameters, torch.float32)):
        if t.dtype != dt or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous {dt} tensor, got {t.dtype}")
    dev = depth_test.device
    B, H, W = (int(v) for v in depth_test.shape)
    Q = int(class_of.shape[0])
    if tuple(depth_est.shape) != (Q, H, W) or tuple(depth_gt.shape) != (Q, H, W) or int(frame_of.shape[0]) != Q or tuple(K.shape) != (B, 3, 3):
        raise ValueError(f"depth_est {tuple(depth_est.shape)} / depth_gt {tuple(depth_gt.shape)} / K {tuple(K.shape)} for {Q} rows and "
                         f"depth_test {tuple(depth_test.shape)}")
    tau = _taus_device(taus, dev)
    n_tau = int(tau.shape[0])
    err, counts = out if out is not None else (torch.empty((Q, n_tau), dtype=torch.float64, device=dev),
                                               torch.empty((Q, 2 + n_tau), dtype=torch.int32, device=dev))
    lib = _lib.load()
    wbytes = lib.ffb6d_bop_vsd_workspace_bytes(Q, H, W)
    ws = torch.empty((max(wbytes, 1),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _lib.traced("bop_vsd", 12 * Q * H * W, (Q, H, W, n_tau)):
        rc = lib.ffb6d_bop_vsd_f32(depth_test.data_ptr(), depth_est.data_ptr(), depth_gt.data_ptr(), class_of.data_ptr(), frame_of.data_ptr(),
                                   Q, K.data_ptr(), B, H, W, diameters.data_ptr(), int(diameters.shape[0]), float(delta), tau.data_ptr(),
                                   n_tau, counts.data_ptr(), err.data_ptr(), ws.data_ptr(), wbytes, _stream(ws))
    _lib.check(rc, "ffb6d_bop_vsd_f32")
    return err, counts


def render_pairs(meshes, est, gt, cls, frm, Kd, H, W):
    """Rows' models rendered alone under both poses -> depth_est, depth_gt f32 [n,H,W] (device tensors in, device tensors out)."""
    n = int(cls.shape[0])
    Kq = Kd[frm.clamp(0, Kd.shape[0] - 1).long()]                               # a frame id out of range renders with some camera: the row is NaN anyway
    frames = torch.arange(2 * n, dtype=torch.int32, device=cls.device)
    depth = _render.render(meshes, torch.cat([est, gt]), frames, torch.cat([cls, cls]), torch.cat([Kq, Kq]), 2 * n, H, W,
                           outputs=("depth",))["depth"]
    return depth[:n], depth[n:]


def rows_per_chunk(H, W):
    """Rows `vsd` renders and compares at a time: two frames per row, at most render.MAX_INSTANCES instances and CHUNK_PIXELS pixels
    per render call (the renderer's key image takes 8 bytes per pixel: 256 MiB), at least one row."""
    return max(1, min(_render.MAX_INSTANCES, CHUNK_PIXELS // (H * W)) // 2)


def vsd(depth_test, est_RT, gt_RT, class_of, frame_of, K, meshes, diameters, delta=VSD_DELTA, taus=VSD_TAUS, chunk_rows=None):
    """VSD of Q (estimated, ground-truth) pose pairs against the measured depth of their frames:
      depth_test [B,H,W] metres (0, negative or not finite = no measurement), est_RT / gt_RT [Q,3,4], class_of [Q] into `meshes`
      (a render.PreparedMeshes, or the list it takes) and `diameters` ([n_cls], the models' unit), frame_of [Q] into depth_test and
      K ([B,3,3] or [3,3]); delta: the visibility tolerance; taus: 1 to 16 misalignment tolerances as fractions of the diameter.
    Each row's model is drawn alone under its two poses through render.render(..., outputs=("depth",)) -- 2 frames per row -- and
    the three images are compared by the VSD kernel.  Rows go through in chunks of rows_per_chunk(H, W) = max(1, min(1024,
    2^25 / (H W)) / 2) (or chunk_rows if smaller): at most render.MAX_INSTANCES = 1024 instances per render call, and at most 2^25
    pixels, so that the renderer's 8-byte key image stays within 256 MiB (54 rows of 480 x 640).  Results do not depend on it.
    Returns device tensors vsd f64 [Q, n_tau] and counts i32 [Q, 2 + n_tau] = [n_union, n_inter, cost_0 ..] per row; a row whose class
    or frame id is out of range gives NaN and counts of 0, a row without any visible pixel 1.0."""
    meshes = _render._prepared(meshes)
    dev = meshes.device
    test = _device_array(depth_test, dev, torch.float32, np.float32)
    if test.dim() != 3:
        raise ValueError(f"depth_test must be [B,H,W], got {tuple(test.shape)}")
    B, H, W = (int(v) for v in test.shape)
    est, gt, cls, frm, Kd = _rows(est_RT, gt_RT, class_of, frame_of, K, dev)
    if Kd.shape[0] == 1 and B > 1:
        Kd = Kd.expand(B, 3, 3).contiguous()
    if int(Kd.shape[0]) != B:
        raise ValueError(f"K must be [3,3] or [{B},3,3], got {tuple(Kd.shape)}")
    diam = _device_array(diameters, dev, torch.float32, np.float32).reshape(-1)
    if int(diam.shape[0]) != meshes.n_cls:
        raise ValueError(f"{int(diam.shape[0])} diameters for {meshes.n_cls} classes")
    Q = int(cls.shape[0])
    tau = _taus_device(taus, dev)                                                # one upload for all the chunks
    n_tau = int(tau.shape[0])
    err = torch.empty((Q, n_tau), dtype=torch.float64, device=dev)
    counts = torch.empty((Q, 2 + n_tau), dtype=torch.int32, device=dev)
    step = rows_per_chunk(H, W) if chunk_rows is None else max(1, min(int(chunk_rows), rows_per_chunk(H, W)))
    for q0 in range(0, Q, step):
        q1 = min(Q, q0 + step)
        d_est, d_gt = render_pairs(meshes, est[q0:q1], gt[q0:q1], cls[q0:q1], frm[q0:q1], Kd, H, W)
        vsd_compare(test, d_est, d_gt, cls[q0:q1], frm[q0:q1], Kd, diam, delta, tau, out=(err[q0:q1], counts[q0:q1]))
    return err, counts


# ---- instance visibility and matching (include/ffb6d_bop_scene.h) -----------------------------------------------------------
MAX_GROUP = 64                                       # FFB6D_BOP_MAX_GROUP: estimates, and instances, of one (frame, class)
MAX_MATCH_COLS = MAX_MATCH_THRS = 16
INFO_INTS = 12                                       # px_count_all, _valid, _visib, _support, bbox_obj xywh, bbox_visib xywh


def visib_compare(depth_test, depth_obj, frame_of, K, delta=VSD_DELTA, masks=False, out=None):
    """The visibility kernel alone, on depth images that exist already: depth_test f32 [B,H,W], depth_obj f32 [Q,H,W] (row q's
    model rendered alone under its pose), frame_of i32 [Q], K f64 [B,3,3]: contiguous device tensors.  Q <= 65535.
    -> (info i32 [Q,12], visib_fract f64 [Q], mask_visib u8 [Q,H,W] or None); `out`: that triple, to be written in place (its mask
    entry decides whether masks are written)."""
    _need_gpu(depth_test, depth_obj, frame_of, K)
    for name, t, dt in (("depth_test", depth_test, torch.float32), ("depth_obj", depth_obj, torch.float32), ("frame_of", frame_of, torch.int32),
                        ("K", K, torch.float64)):
        if t.dtype != dt or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous {dt} tensor, got {t.dtype}")
    dev = depth_test.device
    B, H, W = (int(v) for v in depth_test.shape)
    Q = int(frame_of.shape[0])
    if tuple(depth_obj.shape) != (Q, H, W) or tuple(K.shape) != (B, 3, 3):
        raise ValueError(f"depth_obj {tuple(depth_obj.shape)} / K {tuple(K.shape)} for {Q} rows and depth_test {tuple(depth_test.shape)}")
    if out is not None:
        info, fract, mask = out
    else:
        info = torch.empty((Q, INFO_INTS), dtype=torch.int32, device=dev)
        fract = torch.empty((Q,), dtype=torch.float64, device=dev)
        mask = torch.empty((Q, H, W), dtype=torch.uint8, device=dev) if masks else None
    lib = _lib.load()
    wbytes = lib.ffb6d_bop_visib_workspace_bytes(Q, H, W)
    ws = torch.empty((max(wbytes, 1),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _lib.traced("bop_visib", (8 + (mask is not None)) * Q * H * W, (Q, H, W, mask is not None)):
        rc = lib.ffb6d_bop_visib_f32(depth_test.data_ptr(), depth_obj.data_ptr(), frame_of.data_ptr(), Q, K.data_ptr(), B, H, W, float(delta),
                                     info.data_ptr(), fract.data_ptr(), mask.data_ptr() if mask is not None else None, ws.data_ptr(),
                                     wbytes, _stream(ws))
    _lib.check(rc, "ffb6d_bop_visib_f32")
    return info, fract, mask


def instance_info(depth_test, RT, class_of, frame_of, K, meshes, delta=VSD_DELTA, masks=False, chunk_rows=None):
    """What BOP publishes per ground-truth instance (scene_gt_info), and the plausibility figures of an estimated pose: each row's
    model is drawn ALONE under RT[q] through render.render(..., outputs=("depth",)) and compared with the measured depth of its
    frame by the visibility kernel.  depth_test [B,H,W] metres, RT [Q,3,4], class_of [Q] into `meshes`, frame_of [Q] into depth_test
    and K ([B,3,3] or [3,3]): host data (uploaded) or device tensors.  One frame per row: 2 * rows_per_chunk(H, W) rows a chunk (or
    chunk_rows if smaller) under the renderer's two bounds; results do not depend on it.
    -> dict of device tensors px_count_all, px_count_valid, px_count_visib, px_count_support i32 [Q], visib_fract f64 [Q], bbox_obj,
    bbox_visib i32 [Q,4] = x, y, w, h (-1 when empty; bbox_obj covers the part of the silhouette inside the frame) and, with masks,
    mask_visib u8 [Q,H,W].  A row whose frame id is out of range gives counts 0, boxes -1 and a fraction of NaN.  Host class ids out
    of range are refused; device ids are not read back: such a row is rendered with a clamped class and returned like a bad frame."""
    meshes = _render._prepared(meshes)
    dev = meshes.device
    test = _device_array(depth_test, dev, torch.float32, np.float32)
    if test.dim() != 3:
        raise ValueError(f"depth_test must be [B,H,W], got {tuple(test.shape)}")
    B, H, W = (int(v) for v in test.shape)
    if not torch.is_tensor(class_of):
        c = np.asarray(class_of, np.int64).reshape(-1)
        if len(c) and (c.min() < 0 or c.max() >= meshes.n_cls):
            raise ValueError(f"class_of outside [0, {meshes.n_cls})")
    poses = _device_array(RT, dev, torch.float64, np.float64).reshape(-1, 3, 4)
    _, _, cls, frm, Kd = _rows(poses, poses, class_of, frame_of, K, dev)
    if Kd.shape[0] == 1 and B > 1:
        Kd = Kd.expand(B, 3, 3).contiguous()
    if int(Kd.shape[0]) != B:
        raise ValueError(f"K must be [3,3] or [{B},3,3], got {tuple(Kd.shape)}")
    Q = int(cls.shape[0])
    info = torch.empty((Q, INFO_INTS), dtype=torch.int32, device=dev)
    fract = torch.empty((Q,), dtype=torch.float64, device=dev)
    mask = torch.empty((Q, H, W), dtype=torch.uint8, device=dev) if masks else None
    bad_cls = (cls < 0) | (cls >= meshes.n_cls)
    drawn = cls.clamp(0, meshes.n_cls - 1)
    frm = torch.where(bad_cls, torch.full_like(frm, -1), frm)                    # the kernel's bad-frame row: counts 0, boxes -1, NaN
    full = 2 * rows_per_chunk(H, W) if CHUNK_PIXELS // (H * W) >= 2 else 1
    step = full if chunk_rows is None else max(1, min(int(chunk_rows), full))
    for q0 in range(0, Q, step):
        q1 = min(Q, q0 + step)
        n = q1 - q0
        Kq = Kd[frm[q0:q1].clamp(0, B - 1).long()]                               # a frame id out of range renders with some camera: the row is NaN anyway
        depth = _render.render(meshes, poses[q0:q1], torch.arange(n, dtype=torch.int32, device=dev), drawn[q0:q1], Kq, n, H, W,
                               outputs=("depth",))["depth"]
        visib_compare(test, depth, frm[q0:q1].contiguous(), Kd, delta, out=(info[q0:q1], fract[q0:q1], mask[q0:q1] if masks else None))
    out = dict(px_count_all=info[:, 0], px_count_valid=info[:, 1], px_count_visib=info[:, 2], px_count_support=info[:, 3], visib_fract=fract,
               bbox_obj=info[:, 4:8], bbox_visib=info[:, 8:12])
    if masks:
        out["mask_visib"] = mask
    return out


def pair_rows(est_class, est_frame, gt_class, gt_frame):
    """Host bookkeeping on the ids: groups the estimates and the ground-truth instances of a test set by (frame, class) -- groups
    in ascending (frame, class), members in their input order -- and lists every (estimate, instance) pair of every group, ready to
    feed `mssd_mspd` and `vsd` (est_RT[pair_est], gt_RT[pair_gt], group_class[pair_group], group_frame[pair_group]).
    Estimates of a (frame, class) without any instance form a group with T_g = 0, instances without an estimate one with E_g = 0.
    -> dict of numpy arrays: est_begin, gt_begin i32 [G+1], pair_begin i64 [G+1]; group_frame, group_class i64 [G];
    est_order i64 [Etot] / gt_order i64 [Gtot]: input index of the member at each grouped position (the order of `match`'s score
    argument and of its outputs' rows); est_group, gt_group i64: the group at each grouped position; pair_est, pair_gt i64 [Npairs]:
    INPUT indices of each pair's estimate and instance, pair_group i64 [Npairs]."""
    ec, ef = np.asarray(est_class, np.int64).reshape(-1), np.asarray(est_frame, np.int64).reshape(-1)
    gc, gf = np.asarray(gt_class, np.int64).reshape(-1), np.asarray(gt_frame, np.int64).reshape(-1)
    if len(ec) != len(ef) or len(gc) != len(gf):
        raise ValueError(f"{len(ec)} / {len(ef)} estimate class / frame ids, {len(gc)} / {len(gf)} ground-truth ones")
    keys = np.unique(np.stack([np.concatenate([ef, gf]), np.concatenate([ec, gc])], 1), axis=0).reshape(-1, 2)      # sorted by (frame, class)
    G = len(keys)
    index = {(int(f), int(c)): g for g, (f, c) in enumerate(keys)}
    eg = np.array([index[(int(f), int(c))] for f, c in zip(ef, ec)], np.int64).reshape(-1)
    gg = np.array([index[(int(f), int(c))] for f, c in zip(gf, gc)], np.int64).reshape(-1)
    est_order, gt_order = np.argsort(eg, kind="stable"), np.argsort(gg, kind="stable")
    E, T = np.bincount(eg, minlength=G), np.bincount(gg, minlength=G)
    est_begin = np.concatenate([[0], np.cumsum(E)]).astype(np.int32)
    gt_begin = np.concatenate([[0], np.cumsum(T)]).astype(np.int32)
    pair_begin = np.concatenate([[0], np.cumsum(E.astype(np.int64) * T)]).astype(np.int64)
    pair_est, pair_gt, pair_group = np.zeros(int(pair_begin[-1]), np.int64), np.zeros(int(pair_begin[-1]), np.int64), np.zeros(int(pair_begin[-1]), np.int64)
    for g in range(G):
        e = est_order[est_begin[g]:est_begin[g + 1]]
        t = gt_order[gt_begin[g]:gt_begin[g + 1]]
        pair_est[pair_begin[g]:pair_begin[g + 1]] = np.repeat(e, len(t))
        pair_gt[pair_begin[g]:pair_begin[g + 1]] = np.tile(t, len(e))
        pair_group[pair_begin[g]:pair_begin[g + 1]] = g
    return dict(est_begin=est_begin, gt_begin=gt_begin, pair_begin=pair_begin, group_frame=keys[:, 0].copy(), group_class=keys[:, 1].copy(),
                est_order=est_order, gt_order=gt_order, est_group=eg[est_order], gt_group=gg[gt_order], pair_est=pair_est, pair_gt=pair_gt,
                pair_group=pair_group)


def _group_tables(groups, dev):
    """The three begin tables of `groups` on dev, uploaded once per dict and device"""
    cache = groups.setdefault("_device", {})
    if dev not in cache:
        cache[dev] = tuple(torch.from_numpy(np.ascontiguousarray(groups[k], dt)).to(dev)
                           for k, dt in (("est_begin", np.int32), ("gt_begin", np.int32), ("pair_begin", np.int64)))
    return cache[dev]


def match(err, score, groups, thr, max_ests=None):
    """Greedy matching of scored estimates to ground-truth instances, the rule of include/ffb6d_bop_scene.h, for every group and
    every configuration (error column, threshold) in one launch:
      err f64 [Npairs] or [Npairs, n_col]: the pair rows of `pair_rows` as `mssd_mspd` / `vsd` score them; score f32 [Etot] in the
      grouped order (score_in[groups["est_order"]]); thr f64 [G] or [G, n_thr] per-group thresholds; max_ests i32 [G] or None: only
      the best max_ests[g] estimates of a group are considered (0: all).  Host data (uploaded) or device tensors; `groups`: the dict
      of pair_rows (its begin tables are checked on the host by ffb6d_bop_match_check, then uploaded once and kept in the dict).
    -> (est_gt i32 [Etot, n_col, n_thr], gt_est i32 [Gtot, n_col, n_thr]) device tensors of LOCAL indices within the group, -1 = none."""
    est_begin, gt_begin, pair_begin = (np.ascontiguousarray(groups[k], dt) for k, dt in (("est_begin", np.int32), ("gt_begin", np.int32),
                                                                                       ("pair_begin", np.int64)))
    G = len(est_begin) - 1
    if G < 0 or len(gt_begin) != G + 1 or len(pair_begin) != G + 1:
        raise ValueError(f"begin tables of {len(est_begin)}, {len(gt_begin)} and {len(pair_begin)} entries")
    Etot, Gtot, Npairs = int(est_begin[-1]), int(gt_begin[-1]), int(pair_begin[-1])
    shape = lambda x: tuple(x.shape) if torch.is_tensor(x) else np.shape(x)                                                # noqa: E731
    es, ts = shape(err), shape(thr)
    es, ts = es + (1,) * (len(es) == 1), ts + (1,) * (len(ts) == 1)
    if len(es) != 2 or len(ts) != 2 or es[0] != Npairs or ts[0] != G:
        raise ValueError(f"err {shape(err)} for {Npairs} pairs, thr {shape(thr)} for {G} groups")
    n_col, n_thr = int(es[1]), int(ts[1])
    host_max = None
    if max_ests is not None and not torch.is_tensor(max_ests):
        host_max = np.ascontiguousarray(np.asarray(max_ests, np.int32).reshape(-1))
    if max_ests is not None and int(np.prod(shape(max_ests))) != G:
        raise ValueError(f"max_ests {shape(max_ests)} for {G} groups")
    lib = _lib.load()                                                            # the host check comes before any upload
    _lib.check(lib.ffb6d_bop_match_check(est_begin.ctypes.data, gt_begin.ctypes.data, pair_begin.ctypes.data,
                                         host_max.ctypes.data if host_max is not None else None, G, Etot, Gtot, Npairs, n_col, n_thr),
               "ffb6d_bop_match_check")
    dev = err.device if torch.is_tensor(err) and err.is_cuda else torch.device("cuda", torch.cuda.current_device())
    errd = _device_array(err, dev, torch.float64, np.float64).reshape(Npairs, n_col)
    thrd = _device_array(thr, dev, torch.float64, np.float64).reshape(G, n_thr)
    sc = _device_array(score, dev, torch.float32, np.float32).reshape(-1)
    if int(sc.shape[0]) != Etot:
        raise ValueError(f"{int(sc.shape[0])} scores for {Etot} estimates")
    if max_ests is not None:
        max_ests = _device_array(max_ests, dev, torch.int32, np.int32).reshape(-1)
    eb, gb, pb = _group_tables(groups, dev)
    est_gt = torch.empty((Etot, n_col, n_thr), dtype=torch.int32, device=dev)
    gt_est = torch.empty((Gtot, n_col, n_thr), dtype=torch.int32, device=dev)
    _need_gpu(est_gt)
    with torch.cuda.device(dev), _lib.traced("bop_match", 0, (G, Etot, Gtot, n_col, n_thr)):
        rc = lib.ffb6d_bop_match_f64(eb.data_ptr(), gb.data_ptr(), pb.data_ptr(), G, Etot, Gtot, Npairs, errd.data_ptr(), n_col, sc.data_ptr(),
                                     thrd.data_ptr(), n_thr, max_ests.data_ptr() if max_ests is not None else None, est_gt.data_ptr(),
                                     gt_est.data_ptr(), None, 0, _stream(est_gt))
    _lib.check(rc, "ffb6d_bop_match_f64")
    return est_gt, gt_est


# ---- recall (host, numpy) ---------------------------------------------------------------------------------------------------
def recall(errors, thresholds):
    """Fraction of (estimate, threshold) pairs with error < threshold.  errors [N] (or [N,k]: k error values per estimate, each
    compared with every threshold -- VSD's taus); thresholds [T], or [N,T] for per-estimate thresholds.  A missing estimate is an
    infinite error; NaN counts as a miss; no estimates give 0."""
    e = np.asarray(errors, np.float64)
    th = np.asarray(thresholds, np.float64)
    if e.size == 0:
        return 0.0
    e = e.reshape(len(e), -1)
    th = th.reshape(1, -1) if th.ndim <= 1 else th.reshape(len(e), -1)
    return float((e[:, :, None] < th[:, None, :]).mean())


def average_recall(vsd_err, mssd, mspd, diameters, width=640):
    """The BOP19 numbers of N estimates: vsd_err [N, 10] (the 10 VSD_TAUS), mssd [N] and diameters [N] in one unit, mspd [N] pixels,
    width: the image width (MSPD thresholds scale with width / 640; a scalar or [N]).
      AR_VSD:  e < theta,             theta in 0.05 .. 0.5, averaged over the thresholds and the 10 taus
      AR_MSSD: e < theta * diameter,  theta in 0.05 .. 0.5
      AR_MSPD: e < theta * (W / 640), theta in 5 .. 50 pixels
    -> dict(ar_vsd, ar_mssd, ar_mspd, ar = their mean, n)."""
    mssd, mspd = np.asarray(mssd, np.float64).reshape(-1), np.asarray(mspd, np.float64).reshape(-1)
    n = len(mssd)
    diam = np.broadcast_to(np.asarray(diameters, np.float64).reshape(-1), (n,))
    scale = np.broadcast_to(np.asarray(width, np.float64).reshape(-1), (n,)) / 640.0
    vsd_err = np.asarray(vsd_err, np.float64)
    ar_vsd = recall(vsd_err.reshape(n, vsd_err.size // max(n, 1)), VSD_THRESHOLDS)
    ar_mssd = recall(mssd, diam[:, None] * MSSD_THRESHOLDS[None, :])
    ar_mspd = recall(mspd, scale[:, None] * MSPD_THRESHOLDS[None, :].astype(np.float64))
    return dict(ar_vsd=ar_vsd, ar_mssd=ar_mssd, ar_mspd=ar_mspd, ar=(ar_vsd + ar_mssd + ar_mspd) / 3.0, n=n)


class BOPEval:
    """Accumulates the three errors of a test run and summarises them, like evaluate.TorchEval does for ADD(-S).
    models: evaluate.ModelPoints (the mesh vertices), meshes: render.PreparedMeshes, syms: SymmetrySets, diameters [n_cls]: all
    indexed by class id.  Errors stay on the device, one set of tensors per scored batch, until a summary is asked for."""

    def __init__(self, models, meshes, syms, diameters, delta=VSD_DELTA):
        self.models, self.meshes, self.syms = models, _render._prepared(meshes), syms
        self.diameters = np.asarray(_numpy(diameters), np.float64).reshape(-1)
        self.n_cls = models.n_cls
        if not (self.meshes.n_cls == syms.n_cls == len(self.diameters) == self.n_cls):
            raise ValueError("models, meshes, syms and diameters must cover the same classes")
        self.delta = delta
        self._diam_dev = torch.from_numpy(self.diameters.astype(np.float32)).to(self.meshes.device)
        self._pending = []
        self.cls_ids, self.widths = np.zeros(0, np.int64), np.zeros(0)
        self.vsd, self.mssd, self.mspd = np.zeros((0, len(VSD_TAUS))), np.zeros(0), np.zeros(0)

    def add_batch(self, depth_test, est_RT, gt_RT, class_of, frame_of, K, found=None):
        """Scores Q rows (the arguments of `vsd` and `mssd_mspd`); class_of is host data.  found [Q] bool: False marks a ground-truth
        instance without an estimate -- its est_RT is ignored and its three errors are infinite."""
        cls = np.asarray(_numpy(class_of), np.int64).reshape(-1)
        if len(cls) == 0:
            return
        if cls.min() < 0 or cls.max() >= self.n_cls:
            raise ValueError(f"class_of outside [0, {self.n_cls})")
        dev = self.meshes.device
        est = _device_array(est_RT, dev, torch.float64, np.float64).reshape(-1, 3, 4)
        gt = _device_array(gt_RT, dev, torch.float64, np.float64).reshape(-1, 3, 4)
        miss = None
        if found is not None:
            miss = ~_device_array(found, dev, torch.bool, np.bool_).reshape(-1)
            est = torch.where(miss[:, None, None], gt, est)
        mssd, mspd = mssd_mspd(est, gt, cls, frame_of, K, self.models, self.syms)
        err, _ = vsd(depth_test, est, gt, cls, frame_of, K, self.meshes, self._diam_dev, self.delta, VSD_TAUS)
        if miss is not None:
            inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
            mssd, mspd, err = torch.where(miss, inf, mssd), torch.where(miss, inf, mspd), torch.where(miss[:, None], inf, err)
        self._pending.append((cls, int(depth_test.shape[-1]), err, mssd, mspd))

    def _flush(self):
        for cls, width, err, mssd, mspd in self._pending:
            self.cls_ids = np.concatenate([self.cls_ids, cls])
            self.widths = np.concatenate([self.widths, np.full(len(cls), float(width))])
            self.vsd = np.concatenate([self.vsd, err.cpu().numpy()])
            self.mssd = np.concatenate([self.mssd, mssd.cpu().numpy()])
            self.mspd = np.concatenate([self.mspd, mspd.cpu().numpy()])
        self._pending = []

    def cal_ar(self):
        """-> dict(ar, ar_vsd, ar_mssd, ar_mspd, n: over every scored row; ar_lst, ar_vsd_lst, ar_mssd_lst, ar_mspd_lst, n_lst: per
        class id, index 0 = all objects as in TorchEval.cal_auc; classes without rows count as 0)."""
        self._flush()
        diam = self.diameters[self.cls_ids]
        out = average_recall(self.vsd, self.mssd, self.mspd, diam, self.widths)
        table = [out] + [None] * (self.n_cls - 1)
        for c in range(1, self.n_cls):
            m = self.cls_ids == c
            table[c] = average_recall(self.vsd[m], self.mssd[m], self.mspd[m], diam[m], self.widths[m])
        out = dict(out)
        for k in ("ar", "ar_vsd", "ar_mssd", "ar_mspd", "n"):
            out[k + "_lst"] = [t[k] for t in table]
        return out


class BOPSceneEval:
    """BOP19 recall of a test run with several ground-truth instances and several scored estimates per (frame, object): the
    instances' visibility decides which of them are targets (visib_fract >= min_visib), every (estimate, instance) pair of a
    (frame, class) group is scored by the three error functions, and estimates are matched to instances greedily by score, once
    per error function and threshold (include/ffb6d_bop_scene.h).  Arguments as BOPEval.  The matchings and the valid mask stay on
    the device, one set of tensors per batch, until a summary is asked for."""

    def __init__(self, models, meshes, syms, diameters, delta=VSD_DELTA, min_visib=0.1):
        self.models, self.meshes, self.syms = models, _render._prepared(meshes), syms
        self.diameters = np.asarray(_numpy(diameters), np.float64).reshape(-1)
        self.n_cls = models.n_cls
        if not (self.meshes.n_cls == syms.n_cls == len(self.diameters) == self.n_cls):
            raise ValueError("models, meshes, syms and diameters must cover the same classes")
        self.delta, self.min_visib = delta, min_visib
        self._diam_dev = torch.from_numpy(self.diameters.astype(np.float32)).to(self.meshes.device)
        self._pending = []
        self._hits = {k: np.zeros(0, np.int64) for k in ("vsd", "mssd", "mspd")}      # per instance: configurations in which it was matched
        self._configs = {k: 0 for k in self._hits}
        self._considered = {k: 0 for k in self._hits}
        self.cls_ids, self.valid = np.zeros(0, np.int64), np.zeros(0, bool)

    def add_batch(self, depth_test, K, est_RT, est_class, est_frame, est_score, gt_RT, gt_class, gt_frame):
        """One batch of frames: depth_test [B,H,W], K [B,3,3] or [3,3]; E estimates est_RT [E,3,4] with est_class / est_frame [E]
        (host ids) and est_score [E], or None for px_count_support / max(px_count_all, 1) of each estimate's render against the
        measured depth; T ground-truth instances gt_RT [T,3,4], gt_class / gt_frame [T] (host ids).  Each group may hold at most
        MAX_GROUP = 64 estimates and 64 instances.  max_ests of a group is its number of valid targets (BOP19's rule), computed
        on the device.
        -> the batch's matchings: dict(groups: the dict of pair_rows; valid bool [T] and score f32 [E] in grouped order, visib_fract f64
        [T] in input order; est_gt / gt_est: {"vsd", "mssd", "mspd"} -> the tensors of `match`), device tensors; None without instances."""
        ec, ef = np.asarray(_numpy(est_class), np.int64).reshape(-1), np.asarray(_numpy(est_frame), np.int64).reshape(-1)
        gc, gf = np.asarray(_numpy(gt_class), np.int64).reshape(-1), np.asarray(_numpy(gt_frame), np.int64).reshape(-1)
        for c in (ec, gc):
            if len(c) and (c.min() < 0 or c.max() >= self.n_cls):
                raise ValueError(f"class ids outside [0, {self.n_cls})")
        if len(gc) == 0:
            return None
        dev = self.meshes.device
        W = int(depth_test.shape[-1])
        est = _device_array(est_RT, dev, torch.float64, np.float64).reshape(-1, 3, 4)
        gt = _device_array(gt_RT, dev, torch.float64, np.float64).reshape(-1, 3, 4)
        groups = pair_rows(ec, ef, gc, gf)
        idx = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                                                   # noqa: E731
        fract = instance_info(depth_test, gt, gc, gf, K, self.meshes, self.delta)["visib_fract"]
        valid = fract[idx(groups["gt_order"])] >= self.min_visib                                                            # grouped order; NaN: not a target
        if est_score is None:
            info = instance_info(depth_test, est, ec, ef, K, self.meshes, self.delta)
            score = (info["px_count_support"].double() / info["px_count_all"].clamp(min=1).double()).float()
        else:
            score = _device_array(est_score, dev, torch.float32, np.float32).reshape(-1)
        score = score[idx(groups["est_order"])]
        total = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(valid.long(), 0)])
        gb = idx(groups["gt_begin"].astype(np.int64))
        n_valid = (total[gb[1:]] - total[gb[:-1]]).int()                                                                    # valid targets per group
        E = idx(np.diff(groups["est_begin"]).astype(np.int32))
        considered = torch.minimum(E, n_valid).sum()                                                                        # a group without targets considers nothing
        pe, pg = idx(groups["pair_est"]), idx(groups["pair_gt"])
        pcls, pfrm = groups["group_class"][groups["pair_group"]], groups["group_frame"][groups["pair_group"]]
        mssd, mspd = mssd_mspd(est[pe], gt[pg], pcls, pfrm, K, self.models, self.syms)
        err, _ = vsd(depth_test, est[pe], gt[pg], pcls, pfrm, K, self.meshes, self._diam_dev, self.delta, VSD_TAUS)
        G = len(groups["group_class"])
        thr = dict(mssd=self.diameters[groups["group_class"]][:, None] * MSSD_THRESHOLDS[None, :],
                   mspd=(np.full(G, float(W)) / 640.0)[:, None] * MSPD_THRESHOLDS[None, :].astype(np.float64),
                   vsd=np.broadcast_to(np.asarray(VSD_THRESHOLDS, np.float64)[None, :], (G, len(VSD_THRESHOLDS))))
        matched = {k: match(e, score, groups, thr[k], n_valid) for k, e in (("vsd", err), ("mssd", mssd), ("mspd", mspd))}
        gt_est = {k: m[1] for k, m in matched.items()}
        self._pending.append((gc[groups["gt_order"]], valid, considered, gt_est))
        return dict(groups=groups, valid=valid, visib_fract=fract, score=score, est_gt={k: m[0] for k, m in matched.items()}, gt_est=gt_est)

    def _flush(self):
        for cls, valid, considered, gt_est in self._pending:
            v = valid.cpu().numpy()
            self.cls_ids, self.valid = np.concatenate([self.cls_ids, cls]), np.concatenate([self.valid, v])
            for k, m in gt_est.items():
                n_cfg = int(m.shape[1] * m.shape[2])
                if self._configs[k] not in (0, n_cfg):
                    raise ValueError(f"{k}: batches of {self._configs[k]} and {n_cfg} configurations")
                self._configs[k] = n_cfg
                self._hits[k] = np.concatenate([self._hits[k], (m >= 0).sum((1, 2)).cpu().numpy().astype(np.int64)])
                self._considered[k] += int(considered) * n_cfg
        self._pending = []

    def _recalls(self, sel):
        n = int(sel.sum())
        out = {"ar_" + k: (float(self._hits[k][sel].sum()) / float(self._configs[k] * n) if n else 0.0) for k in ("vsd", "mssd", "mspd")}
        out.update(ar=(out["ar_vsd"] + out["ar_mssd"] + out["ar_mspd"]) / 3.0, n=n)
        return out

    def cal_ar(self):
        """-> the dict of BOPEval.cal_ar (ar, ar_vsd, ar_mssd, ar_mspd, n and their per-class `_lst` forms, index 0 = all objects),
        every recall pooled: the matched valid targets summed over the configurations (10 x 10 for VSD, 10 for MSSD and MSPD),
        divided by (configurations x valid targets); n counts the valid targets.  With one estimate per instance and every instance
        valid this is BOPEval.cal_ar() of the same rows exactly.  Also n_targets, n_ignored (instances below min_visib) and, per
        error function, precision_* = matched valid targets / considered estimates (min(E_g, valid targets of g), summed over the
        groups and configurations: a match to an ignored instance counts on neither side)."""
        self._flush()
        out = self._recalls(self.valid)
        table = [out] + [self._recalls(self.valid & (self.cls_ids == c)) for c in range(1, self.n_cls)]
        out = dict(out)
        for k in ("ar", "ar_vsd", "ar_mssd", "ar_mspd", "n"):
            out[k + "_lst"] = [t[k] for t in table]
        out.update(n_targets=int(self.valid.sum()), n_ignored=int((~self.valid).sum()))
        for k in ("vsd", "mssd", "mspd"):
            out["precision_" + k] = float(self._hits[k][self.valid].sum()) / float(self._considered[k]) if self._considered[k] else 0.0
        return out
