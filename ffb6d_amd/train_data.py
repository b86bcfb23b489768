"""Training samples on the device: the arithmetic of the training half of the reference's `Dataset.get_item`, batched, over
the C ABI of include/ffb6d_train.h.

    pose_targets            get_pose_gt_info + labels_pt   ycb_dataset.py:240,348-386, linemod_dataset.py:287,398-436
    pose_targets_instances  the same per instance          several instances of one class in a frame, found through the renderer's
                                                           instance image (no counterpart in the reference); votes_from_targets
    draw_noise_params       rgb_add_noise's host draws     ycb_dataset.py:107-143, linemod_dataset.py:142-164
    motion_blur_taps        linear_motion_blur's kernel    ycb_dataset.py:88-105 (cv2.line restated)
    rgb_add_noise           rgb_add_noise on the device    HSV, sharpen, motion blur, Gaussian blur, Gaussian noise
    add_real_back           add_real_back                  ycb_dataset.py:145-163, linemod_dataset.py:166-186
    draw_jitter_params      ColorJitter's host draws       transforms.ColorJitter(0.2, 0.2, 0.2, 0.05), ycb_dataset.py:34
    color_jitter            self.trancolor on the device   ycb_dataset.py:190-193, linemod_dataset.py:221-223
    assemble_training_batch color_jitter at decode time, the order of ycb_dataset.py:198-204 / linemod_dataset.py:241-249, then
                            inputs.assemble_inputs and pose_targets

Randomness.  Stage decisions and scalar parameters are drawn on the host from a numpy RandomState in the reference's exact
order, so a frame gets the reference's decisions and parameters up to and including the noise sigma.  The per-pixel normals
come from a counter-based generator on the device (include/ffb6d_train.h), which replaces the reference's
`rng.randn(480, 640, 3)`: the one draw the reference takes after it (YCB's "extra noise" decision) is taken from the same
RandomState and is therefore distribution-equivalent, not draw-identical.

OpenCV is not available where this package is built: the HSV round trip, filter2D / GaussianBlur and cv2.line are restated
from OpenCV's published algorithms and pinned against those restatements (tests/train_data_ref.py), not against cv2.
Pillow is available there, and torchvision's PIL ColorJitter is a thin layer over it: color_jitter is pinned to Pillow's own
bytes (tests/golden/color_jitter.npz, tests/color_jitter_ref.py).  Its planes are R, G, B in that order, whereas plane 0 plays
OpenCV's "B" in rgb_add_noise; both are the same array, as in the reference.
There is no CPU fallback: CPU tensors raise FFB6DNativeError.
"""

import numpy as np
import torch

from . import _lib
from . import inputs as _inputs

MAX_TAPS, MAX_HALO = 32, 15
# ffb6d_stencil_frame_t of include/ffb6d_train.h (all fields 4 bytes wide: no padding)
STENCIL_FRAME = np.dtype([("n_taps", "<i4"), ("halo", "<i4"), ("sigma", "<f4"), ("extra_sigma", "<f4"),
                          ("dy", "<i4", MAX_TAPS), ("dx", "<i4", MAX_TAPS), ("w", "<f4", MAX_TAPS)])
# ffb6d_jitter_frame_t of include/ffb6d_train.h
JITTER_FRAME = np.dtype([("n_ops", "<i4"), ("op", "<i4", 4), ("alpha", "<f4", 4), ("hue_shift", "<i4")])
JITTER_OPS = ("brightness", "contrast", "saturation", "hue")       # FFB6D_JITTER_*; torchvision's fn_idx
FLAVOURS = ("ycb", "linemod")
EXTRA_NOISE_SIGMA = 7.0                     # ycb_dataset.py:141


def _gpu(*ts):
    for t in ts:
        if not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.FFB6DNativeError("ffb6d_amd.train_data runs on the GPU only (got a CPU tensor); there is no CPU fallback")


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _host_or_device(x, dev, dtype):
    """numpy / list / CPU tensor -> (host numpy copy, device tensor); device tensor -> (None, tensor)."""
    if torch.is_tensor(x) and x.is_cuda:
        return None, x.to(dtype).contiguous()
    a = np.asarray(x.detach().numpy() if torch.is_tensor(x) else x)
    return a, torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------------
# pose targets
# ---------------------------------------------------------------------------------------------------------------------
def pose_targets(cld, choose, label_img, cls_ids, RTs, mesh_kps, mesh_ctr):
    """Targets of B frames (include/ffb6d_train.h states every formula):
      cld f32 [B,N,3] (device); choose [B,N] or [B,1,N] int32 / int64 (device); label_img [B,H,W] uint8 / int32 (device);
      cls_ids [B,O] or [B,O,1] class id per object slot, 0 = empty; RTs [B,O,3,4] float64 / float32;
      mesh_kps [n_cls,K,3], mesh_ctr [n_cls,3] indexed by class id (pose.solve_poses' convention).
    cls_ids, RTs and the meshes may be host data (numpy, lists, CPU tensors; uploaded) or device tensors.  Host class ids
    outside [0, n_cls) raise ValueError before anything is launched; device ids are not read back (the kernel treats an id
    outside [1, n_cls) as an empty slot).
    Returns a dict with the reference's keys: labels i32 [B,N], kp_targ_ofst f32 [B,N,K,3] and ctr_targ_ofst f32 [B,N,3]
    (POINT MINUS KEYPOINT, as np.add(cld, -1.0*kp)), kp_3ds f32 [B,O,K,3], ctr_3ds f32 [B,O,3], RTs f32 [B,O,3,4],
    cls_ids i32 [B,O,1]."""
    _gpu(cld, choose, label_img)
    dev = cld.device
    if cld.dim() != 3 or cld.shape[2] != 3 or cld.dtype != torch.float32:
        raise TypeError(f"cld must be float32 [B,N,3], got {cld.dtype} {tuple(cld.shape)}")
    B, N = int(cld.shape[0]), int(cld.shape[1])
    ch = choose.reshape(B, -1) if choose.dim() == 3 else choose
    if ch.dtype not in (torch.int32, torch.int64) or tuple(ch.shape) != (B, N):
        raise TypeError(f"choose must be int32 / int64 [B,N] = [{B},{N}], got {choose.dtype} {tuple(choose.shape)}")
    if label_img.dtype not in (torch.uint8, torch.int32) or label_img.dim() != 3 or label_img.shape[0] != B:
        raise TypeError(f"label_img must be uint8 / int32 [B,H,W], got {label_img.dtype} {tuple(label_img.shape)}")
    HW = int(label_img.shape[1]) * int(label_img.shape[2])
    _, kps = _host_or_device(mesh_kps, dev, torch.float32)
    _, ctr = _host_or_device(mesh_ctr, dev, torch.float32)
    if kps.dim() != 3 or kps.shape[2] != 3 or tuple(ctr.shape) != (kps.shape[0], 3):
        raise ValueError(f"mesh_kps must be [n_cls,K,3] and mesh_ctr [n_cls,3], got {tuple(kps.shape)}, {tuple(ctr.shape)}")
    n_cls, K = int(kps.shape[0]), int(kps.shape[1])
    if torch.is_tensor(RTs) and RTs.is_cuda:
        rts = RTs.contiguous()
    else:
        a = np.asarray(RTs.detach().numpy() if torch.is_tensor(RTs) else RTs)
        rts = torch.from_numpy(np.ascontiguousarray(a if a.dtype in (np.float32, np.float64) else a.astype(np.float64))).to(dev)
    if rts.dtype not in (torch.float32, torch.float64) or rts.dim() != 4 or rts.shape[0] != B or tuple(rts.shape[2:]) != (3, 4):
        raise TypeError(f"RTs must be float64 / float32 [B,O,3,4], got {rts.dtype} {tuple(rts.shape)}")
    O = int(rts.shape[1])
    if torch.is_tensor(cls_ids) and cls_ids.is_cuda:
        if cls_ids.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"cls_ids must be an integer tensor, got {cls_ids.dtype}")
        ids = cls_ids.reshape(B, -1).to(torch.int32).contiguous()
    else:
        a = np.asarray(cls_ids.detach().numpy() if torch.is_tensor(cls_ids) else cls_ids)
        if a.dtype.kind not in "iu":
            raise TypeError(f"cls_ids must hold integers, got {a.dtype}")
        a = a.reshape(B, -1)
        bad = (a < 0) | (a >= n_cls)
        if bad.any():
            b, o = map(int, np.argwhere(bad)[0])
            raise ValueError(f"cls_ids[{b},{o}] = {int(a[b, o])} outside [0, {n_cls})")
        ids = torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    if tuple(ids.shape) != (B, O):
        raise ValueError(f"cls_ids has {tuple(ids.shape)} slots, RTs {O} per frame")
    if not (1 <= K <= 64 and 1 <= O <= 64 and O * (K + 1) <= 1024):
        raise ValueError(f"K = {K}, O = {O} outside the kernel's limits (include/ffb6d_train.h)")
    ch, lab, c = ch.contiguous(), label_img.contiguous(), cld.contiguous()
    out = dict(labels=torch.empty((B, N), dtype=torch.int32, device=dev),
               kp_targ_ofst=torch.empty((B, N, K, 3), dtype=torch.float32, device=dev),
               ctr_targ_ofst=torch.empty((B, N, 3), dtype=torch.float32, device=dev),
               kp_3ds=torch.empty((B, O, K, 3), dtype=torch.float32, device=dev),
               ctr_3ds=torch.empty((B, O, 3), dtype=torch.float32, device=dev),
               RTs=torch.empty((B, O, 3, 4), dtype=torch.float32, device=dev),
               cls_ids=torch.empty((B, O, 1), dtype=torch.int32, device=dev))
    lib = _lib.load()
    with torch.cuda.device(dev), _lib.traced("pose_targets", 4 * B * N * (3 * K + 8), (B, N, K, O)):
        rc = lib.ffb6d_pose_targets(c.data_ptr(), ch.data_ptr(), int(ch.dtype == torch.int64), lab.data_ptr(),
                                    int(lab.dtype == torch.uint8), ids.data_ptr(), rts.data_ptr(), int(rts.dtype == torch.float64),
                                    kps.data_ptr(), ctr.data_ptr(), n_cls, B, N, HW, O, K, out["labels"].data_ptr(),
                                    out["kp_targ_ofst"].data_ptr(), out["ctr_targ_ofst"].data_ptr(), out["kp_3ds"].data_ptr(),
                                    out["ctr_3ds"].data_ptr(), out["RTs"].data_ptr(), out["cls_ids"].data_ptr(), _stream(c))
    _lib.check(rc, "ffb6d_pose_targets")
    return out


def _instance_ids(x, name, hi, dev):
    """frame_of / class_of: host ids (checked against [0, hi)) or a device tensor (not read back) -> int32 [I] on dev."""
    if torch.is_tensor(x) and x.is_cuda:
        if x.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{name} must be an integer tensor, got {x.dtype}")
        return x.reshape(-1).to(torch.int32).contiguous()
    a = np.asarray(x.detach().numpy() if torch.is_tensor(x) else x)
    if a.size and a.dtype.kind not in "iu":
        raise TypeError(f"{name} must hold integers, got {a.dtype}")
    a = a.reshape(-1)
    bad = (a < 0) | (a >= hi)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(f"{name}[{i}] = {int(a[i])} outside [0, {hi})")
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)


def pose_targets_instances(cld, choose, inst_img, frame_of, class_of, poses, mesh_kps, mesh_ctr):
    """Targets of B frames per INSTANCE (include/ffb6d_train.h, ffb6d_pose_targets_inst, states the rule): a point's object is
    the instance that owns its pixel in the renderer's `inst` image, so several instances of one class in a frame keep their
    own keypoints, where pose_targets gives them all the last slot's.
      cld f32 [B,N,3] (device); choose [B,N] or [B,1,N] int32 / int64 (device); inst_img int32 [B,H,W] (device): the global
      instance index per pixel, negative = none (render.render(..., outputs=("inst",)));
      frame_of / class_of [I], poses [I,3,4] float64: render's own instance list; mesh_kps [n_cls,K,3], mesh_ctr [n_cls,3].
    The instance list and the meshes may be host data (uploaded) or device tensors.  Host frame ids outside [0, B) and class
    ids outside [0, n_cls) raise ValueError before anything is launched; device ids are not read back (the kernel gives such
    an instance zero rows and no point).  At most render.MAX_INSTANCES = 1024 instances, 64 keypoints.
    Returns a dict of device tensors: labels i32 [B,N] (class), inst_of_point i32 [B,N] (-1 = none), kp_targ_ofst f32
    [B,N,K,3] and ctr_targ_ofst f32 [B,N,3] (POINT MINUS KEYPOINT), kp_3ds f32 [I,K,3], ctr_3ds f32 [I,3], n_points i32 [I]
    (sampled points owned by each instance).  Two launches, no read-back."""
    _gpu(cld, choose, inst_img)
    dev = cld.device
    if cld.dim() != 3 or cld.shape[2] != 3 or cld.dtype != torch.float32:
        raise TypeError(f"cld must be float32 [B,N,3], got {cld.dtype} {tuple(cld.shape)}")
    B, N = int(cld.shape[0]), int(cld.shape[1])
    ch = choose.reshape(B, -1) if choose.dim() == 3 else choose
    if ch.dtype not in (torch.int32, torch.int64) or tuple(ch.shape) != (B, N):
        raise TypeError(f"choose must be int32 / int64 [B,N] = [{B},{N}], got {choose.dtype} {tuple(choose.shape)}")
    if inst_img.dtype != torch.int32 or inst_img.dim() != 3 or inst_img.shape[0] != B:
        raise TypeError(f"inst_img must be int32 [B,H,W], got {inst_img.dtype} {tuple(inst_img.shape)}")
    HW = int(inst_img.shape[1]) * int(inst_img.shape[2])
    _, kps = _host_or_device(mesh_kps, dev, torch.float32)
    _, ctr = _host_or_device(mesh_ctr, dev, torch.float32)
    if kps.dim() != 3 or kps.shape[2] != 3 or tuple(ctr.shape) != (kps.shape[0], 3):
        raise ValueError(f"mesh_kps must be [n_cls,K,3] and mesh_ctr [n_cls,3], got {tuple(kps.shape)}, {tuple(ctr.shape)}")
    n_cls, K = int(kps.shape[0]), int(kps.shape[1])
    frm = _instance_ids(frame_of, "frame_of", B, dev)
    cls = _instance_ids(class_of, "class_of", n_cls, dev)
    n_inst = int(frm.shape[0])
    _, rts = _host_or_device(poses, dev, torch.float64)
    rts = rts.reshape(-1, 3, 4)
    if int(cls.shape[0]) != n_inst or int(rts.shape[0]) != n_inst:
        raise ValueError(f"{n_inst} frames / {int(cls.shape[0])} classes / {int(rts.shape[0])} poses")
    if not (1 <= K <= 64 and n_inst <= 1024):
        raise ValueError(f"K = {K}, I = {n_inst} outside the kernel's limits (include/ffb6d_train.h)")
    ch, img, c = ch.contiguous(), inst_img.contiguous(), cld.contiguous()
    out = dict(labels=torch.empty((B, N), dtype=torch.int32, device=dev),
               inst_of_point=torch.empty((B, N), dtype=torch.int32, device=dev),
               kp_targ_ofst=torch.empty((B, N, K, 3), dtype=torch.float32, device=dev),
               ctr_targ_ofst=torch.empty((B, N, 3), dtype=torch.float32, device=dev),
               kp_3ds=torch.empty((n_inst, K, 3), dtype=torch.float32, device=dev),
               ctr_3ds=torch.empty((n_inst, 3), dtype=torch.float32, device=dev),
               n_points=torch.empty((n_inst,), dtype=torch.int32, device=dev))
    lib = _lib.load()
    need = int(lib.ffb6d_pose_targets_inst_workspace_bytes(n_inst, K))
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _lib.traced("pose_targets_inst", 4 * B * N * (3 * K + 9), (B, N, K, n_inst)):
        rc = lib.ffb6d_pose_targets_inst(c.data_ptr(), ch.data_ptr(), int(ch.dtype == torch.int64), img.data_ptr(), frm.data_ptr(),
                                         cls.data_ptr(), rts.data_ptr(), kps.data_ptr(), ctr.data_ptr(), n_cls, B, N, HW, n_inst, K,
                                         out["labels"].data_ptr(), out["inst_of_point"].data_ptr(), out["kp_targ_ofst"].data_ptr(),
                                         out["ctr_targ_ofst"].data_ptr(), out["kp_3ds"].data_ptr(), out["ctr_3ds"].data_ptr(),
                                         out["n_points"].data_ptr(), ws.data_ptr(), need, _stream(c))
    _lib.check(rc, "ffb6d_pose_targets_inst")
    return out


def votes_from_targets(targets):
    """The targets of pose_targets / pose_targets_instances in the layout of the network's heads: (ctr_of f32 [B,1,N,3], kp_of
    f32 [B,K,N,3]), the offsets a perfect network would emit.  Targets are POINT MINUS KEYPOINT and the solver votes
    `pcld - offset` (pose.vote_sets; pvn3d_eval_utils_kpls.py:84,125: `pcld - ctr_of[0]`, `pcld - pred_kp_of`), so these votes
    land on the posed keypoints up to one float rounding each way."""
    kp, ctr = targets["kp_targ_ofst"], targets["ctr_targ_ofst"]
    return ctr.unsqueeze(1).contiguous(), kp.permute(0, 2, 1, 3).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# host side of rgb_add_noise: parameter draws and tap lists
# ---------------------------------------------------------------------------------------------------------------------
def _rand_range(rng, lo, hi):
    return rng.rand() * (hi - lo) + lo                                  # ycb_dataset.py:79-80


def draw_noise_params(rng, flavour="ycb"):
    """The decisions and scalar parameters of one rgb_add_noise call, drawn from `rng` (a numpy RandomState) in the
    reference's order (ycb_dataset.py:107-143, linemod_dataset.py:142-164).  Returns a dict:
      hsv (fs, fv) or None; sharpen centre weight or None (YCB only); motion (angle, length) or None;
      gauss (ksize, sigma) or None; noise_sigma (YCB: randint(15) or randint(25); LineMOD: 0);
      extra_noise (YCB: the rand() > 0.8 taken after the noise -- see the module docstring; LineMOD: False)."""
    if flavour not in FLAVOURS:
        raise ValueError(f"flavour must be one of {FLAVOURS}")
    ycb = flavour == "ycb"
    p = dict(hsv=None, sharpen=None, motion=None, gauss=None, noise_sigma=0, extra_noise=False)
    if rng.rand() > 0:
        if ycb:
            p["hsv"] = (_rand_range(rng, 1.25, 1.45), _rand_range(rng, 1.15, 1.35))
        else:
            p["hsv"] = (_rand_range(rng, 1 - 0.25, 1 + .25), _rand_range(rng, 1 - .15, 1 + .15))
    if ycb and rng.rand() > .8:
        p["sharpen"] = rng.rand() * 3 + 9
    if rng.rand() > 0.8:
        r_angle = int(rng.rand() * 360)
        r_len = int(rng.rand() * 15) + 1
        p["motion"] = (r_angle, r_len)
    if rng.rand() > 0.8:
        if rng.rand() > 0.2:
            p["gauss"] = (3, rng.rand())
        else:
            p["gauss"] = (5, rng.rand())
    if ycb:
        if rng.rand() > 0.2:
            p["noise_sigma"] = int(rng.randint(15))
        else:
            p["noise_sigma"] = int(rng.randint(25))
        p["extra_noise"] = bool(rng.rand() > 0.8)
    return p


def _clip_line(w, h, p1, p2):
    """cv::clipLine(Size, Point&, Point&) (drawing.cpp): -> (inside, p1, p2)."""
    x1, y1 = p1
    x2, y2 = p2
    right, bottom = w - 1, h - 1
    if w <= 0 or h <= 0:
        return False, p1, p2
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * (x2 - x1) / (y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * (x2 - x1) / (y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * (y2 - y1) / (x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * (y2 - y1) / (x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, (x1, y1), (x2, y2)


def cv_line_points(w, h, p1, p2):
    """The pixels cv2.line(img, p1, p2, color) sets on a w x h image with thickness 1, LINE_8, shift 0: clipLine, then
    LineIterator's 8-connected Bresenham walk from left to right (drawing.cpp).  Points are (x, y)."""
    ok, (x1, y1), (x2, y2) = _clip_line(w, h, tuple(p1), tuple(p2))
    if not ok:
        return []
    if x2 - x1 < 0:                                                     # leftToRight
        x1, y1, x2, y2 = x2, y2, x1, y1
    dx, dy = x2 - x1, y2 - y1
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    steep = dy > dx
    if steep:
        dx, dy = dy, dx
    err, plus, minus = dx - (dy + dy), dx + dx, -(dy + dy)
    x, y, pts = x1, y1, []
    for _ in range(dx + 1):
        pts.append((x, y))
        diag = err < 0
        err += minus + (plus if diag else 0)
        if steep:
            y += sy
            x += 1 if diag else 0
        else:
            x += 1
            y += sy if diag else 0
    return pts


def motion_blur_taps(angle, length):
    """linear_motion_blur's kernel (ycb_dataset.py:88-105) as a tap list: (dy int [T], dx int [T], w float64 [T]) in
    row-major order of the a x a kernel's non-zero entries, offsets relative to the anchor a // 2 (filter2D's default).
    a <= 0 returns the identity."""
    rad = np.deg2rad(angle)
    dx = np.cos(rad)
    dy = np.sin(rad)
    a = int(max(list(map(abs, (dx, dy)))) * length * 2)
    if a <= 0:
        return np.zeros(1, np.int64), np.zeros(1, np.int64), np.ones(1)
    kern = np.zeros((a, a))
    cx, cy = a // 2, a // 2
    ex, ey = list(map(int, (dx * length + cx, dy * length + cy)))
    for x, y in cv_line_points(a, a, (cx, cy), (ex, ey)):
        kern[y, x] = 1.0
    s = kern.sum()
    if s == 0:
        kern[cx, cy] = 1.0
    else:
        kern /= s
    return _kernel_taps(kern)


def _kernel_taps(kern):
    ii, jj = np.nonzero(kern)                                           # row-major
    return ii - kern.shape[0] // 2, jj - kern.shape[1] // 2, kern[ii, jj]


def sharpen_taps(centre):
    """ycb_dataset.py:118-122: -1 everywhere, `centre` in the middle, normalised by the sum."""
    kern = -np.ones((3, 3))
    kern[1, 1] = centre
    kern /= kern.sum()
    return _kernel_taps(kern)


def gaussian_taps(ksize, sigma):
    """cv2.GaussianBlur(img, (ksize, ksize), sigma) as one 2-D tap list: getGaussianKernel's float64 taps
    (exp(-x^2 / (2 sigma^2)) normalised, sigma <= 0 -> 0.3 ((ksize - 1) / 2 - 1) + 0.8), outer product."""
    if sigma <= 0:
        sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
    x = np.arange(ksize) - (ksize - 1) * 0.5
    k = np.exp(-0.5 / (sigma * sigma) * x * x)
    k = k / k.sum()
    return _kernel_taps(np.outer(k, k))


def _stage_taps(p, stage):
    if stage == "sharpen" and p.get("sharpen") is not None:
        return sharpen_taps(p["sharpen"])
    if stage == "motion" and p.get("motion") is not None:
        return motion_blur_taps(*p["motion"])
    if stage == "gauss" and p.get("gauss") is not None:
        return gaussian_taps(*p["gauss"])
    return None


def _fill_frame(rec, taps):
    if taps is None:
        return
    dy, dx, w = taps
    keep = w != 0
    dy, dx, w = dy[keep], dx[keep], w[keep]
    n = len(w)
    if n > MAX_TAPS or (n and max(np.abs(dy).max(), np.abs(dx).max()) > MAX_HALO):
        raise ValueError(f"{n} taps / offsets beyond {MAX_HALO}: outside the stencil kernel's limits")
    rec["n_taps"] = n
    rec["halo"] = int(max(np.abs(dy).max(), np.abs(dx).max())) if n else 0
    rec["dy"][:n], rec["dx"][:n], rec["w"][:n] = dy, dx, w.astype(np.float32)


def _u8_images(rgb):
    _gpu(rgb)
    if rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[1] != 3:
        raise TypeError(f"rgb must be uint8 [B,3,H,W], got {rgb.dtype} {tuple(rgb.shape)}")
    return rgb.contiguous()


def rgb_add_noise(rgb, params, seed):
    """rgb_add_noise of B frames on the device.  rgb uint8 [B,3,H,W] (the layout assemble_inputs takes; plane 0 plays
    OpenCV's "B", as the reference's RGB array does); params: one dict per frame (draw_noise_params, or built by hand), None
    = the frame passes unchanged; seed: 64-bit key of the per-pixel normals.  Stages in the reference's order: HSV, sharpen,
    motion blur, Gaussian blur, then the noise fused into the last filter pass.  Returns a new uint8 tensor."""
    x = _u8_images(rgb)
    B, _, H, W = x.shape
    if len(params) != B:
        raise ValueError(f"{len(params)} parameter sets for {B} frames")
    params = [p or {} for p in params]
    dev = x.device
    stages = [s for s in ("sharpen", "motion", "gauss") if any(p.get(s) is not None for p in params)]
    noisy = any(p.get("noise_sigma", 0) > 0 or p.get("extra_noise") for p in params)
    if noisy and not stages:
        stages = ["copy"]
    hsv = any(p.get("hsv") is not None for p in params)
    # one upload: fs_fv f64 [B,2], then one ffb6d_stencil_frame_t [B] per pass
    fs_fv = np.full((B, 2), -1.0)
    for b, p in enumerate(params):
        if p.get("hsv") is not None:
            fs_fv[b] = p["hsv"]
    frames = np.zeros((len(stages), B), STENCIL_FRAME)
    for i, s in enumerate(stages):
        for b, p in enumerate(params):
            _fill_frame(frames[i, b], _stage_taps(p, s))
            if i == len(stages) - 1:
                frames[i, b]["sigma"] = float(p.get("noise_sigma", 0))
                frames[i, b]["extra_sigma"] = EXTRA_NOISE_SIGMA if p.get("extra_noise") else 0.0
    blob = np.concatenate([fs_fv.view(np.uint8).reshape(-1), frames.view(np.uint8).reshape(-1)])
    dblob = torch.from_numpy(blob).to(dev)
    lib = _lib.load()
    bufs = [torch.empty_like(x), torch.empty_like(x)]                  # ping-pong
    cur, nxt = x, 0
    with torch.cuda.device(dev):
        if hsv:
            with _lib.traced("rgb_hsv", 2 * x.numel(), (B, H, W)):
                rc = lib.ffb6d_rgb_hsv_jitter(cur.data_ptr(), dblob.data_ptr(), bufs[nxt].data_ptr(), B, H, W, _stream(x))
            _lib.check(rc, "ffb6d_rgb_hsv_jitter")
            cur, nxt = bufs[nxt], 1 - nxt
        for i, s in enumerate(stages):
            ptr = dblob.data_ptr() + 16 * B + i * B * STENCIL_FRAME.itemsize
            with _lib.traced("rgb_stencil", 2 * x.numel(), (B, H, W, s)):
                rc = lib.ffb6d_rgb_stencil(cur.data_ptr(), ptr, int(seed) & 0xFFFFFFFFFFFFFFFF, bufs[nxt].data_ptr(), B, H, W,
                                           _stream(x))
            _lib.check(rc, "ffb6d_rgb_stencil")
            cur, nxt = bufs[nxt], 1 - nxt
    return cur.clone() if cur is x else cur


# ---------------------------------------------------------------------------------------------------------------------
# ColorJitter
# ---------------------------------------------------------------------------------------------------------------------
def draw_jitter_params(generator, brightness=0.2, contrast=0.2, saturation=0.2, hue=0.05):
    """The host draws of one frame's ColorJitter from a torch.Generator (CPU): randperm(4) gives the order, then one uniform
    draw each from [1 - b, 1 + b] (floored at 0), [1 - c, 1 + c], [1 - s, 1 + s] and [-h, h]; the defaults are the reference's
    transforms.ColorJitter(0.2, 0.2, 0.2, 0.05).  An amplitude of None or 0 leaves the operation out.  torchvision is not
    available where this package is built, so this is distribution-equivalent to ColorJitter.get_params, not draw-identical to
    any torchvision release; color_jitter takes explicit orders and factors, so a caller with torchvision can pass its own.
    Returns dict(order=(...), brightness=, contrast=, saturation=, hue=) with the keys of the operations that are on."""
    p = dict(order=tuple(int(i) for i in torch.randperm(4, generator=generator)))
    for key, amp in zip(JITTER_OPS, (brightness, contrast, saturation, hue)):
        if not amp:
            continue
        if amp < 0 or (key == "hue" and amp > 0.5):
            raise ValueError(f"{key} amplitude {amp} outside its range")
        lo, hi = (-amp, amp) if key == "hue" else (max(0.0, 1.0 - amp), 1.0 + amp)
        p[key] = lo + (hi - lo) * float(torch.rand(1, generator=generator, dtype=torch.float64))
    return p


def jitter_records(params):
    """One ffb6d_jitter_frame_t per frame from the per-frame dicts of color_jitter (host side, numpy)."""
    rec = np.zeros(len(params), JITTER_FRAME)
    for b, p in enumerate(params):
        if p is None:
            continue
        order = p.get("order", (0, 1, 2, 3))
        if len(order) > 4:
            raise ValueError(f"frame {b}: order {tuple(order)} holds more than four operations")
        n = 0
        for o in order:
            op = int(o)
            if not 0 <= op < 4:
                raise ValueError(f"frame {b}: unknown operation {o!r} in order")
            val = p.get(JITTER_OPS[op])
            if val is None:
                continue
            if op == 3:
                if not -0.5 <= float(val) <= 0.5:
                    raise ValueError(f"frame {b}: hue {val} outside [-0.5, 0.5]")
                rec[b]["hue_shift"] = int(float(val) * 255.0) % 256     # truncated toward zero, then np.uint8's wrap-around
            else:
                rec[b]["alpha"][n] = np.float32(val)
            rec[b]["op"][n] = op
            n += 1
        rec[b]["n_ops"] = n
    return rec


def color_jitter(rgb, params):
    """torchvision's PIL ColorJitter of B frames on the device, byte for byte (include/ffb6d_train.h states the rule).
    rgb uint8 [B,3,H,W], planes R, G, B; params: one entry per frame, dict(order=(...), brightness=, contrast=, saturation=,
    hue=): `order` lists the operations (0 brightness, 1 contrast, 2 saturation, 3 hue: torchvision's ids) as they are applied, an
    operation whose key is missing or None is skipped, and an entry of None passes the frame unchanged (draw_jitter_params
    makes such dicts).  A repeated operation, a negative or non-finite factor or a hue outside [-0.5, 0.5] raises before
    anything is launched.  One upload carries the records; two launches do the batch.  Returns a new uint8 tensor."""
    x = _u8_images(rgb)
    B, _, H, W = x.shape
    if len(params) != B:
        raise ValueError(f"{len(params)} parameter sets for {B} frames")
    rec = jitter_records(params)
    lib = _lib.load()
    _lib.check(lib.ffb6d_jitter_frames_check(rec.ctypes.data, B), "ffb6d_jitter_frames_check")
    out = torch.empty_like(x)
    if x.numel() == 0:
        return out
    dev = x.device
    contrast = int(sum(1 in r["op"][:r["n_ops"]] for r in rec))
    need = int(lib.ffb6d_color_jitter_workspace_bytes(B, H, W))
    # records and workspace in one buffer: the records behind the workspace, which is a multiple of 256 bytes
    buf = torch.empty(need + rec.nbytes, dtype=torch.uint8, device=dev)
    buf[need:].copy_(torch.from_numpy(rec.view(np.uint8).reshape(-1)), non_blocking=False)
    with torch.cuda.device(dev), _lib.traced("color_jitter", 3 * H * W * (2 * B + contrast), (B, H, W)):
        rc = lib.ffb6d_color_jitter_u8(x.data_ptr(), buf.data_ptr() + need, out.data_ptr(), B, H, W, buf.data_ptr(), need,
                                       _stream(x))
    _lib.check(rc, "ffb6d_color_jitter_u8")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# background compositing
# ---------------------------------------------------------------------------------------------------------------------
def _mask_u8_or_i32(t, name, B, H, W):
    if t.dtype not in (torch.uint8, torch.int32) or tuple(t.shape) != (B, H, W):
        raise TypeError(f"{name} must be uint8 / int32 [{B},{H},{W}], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def add_real_back(rgb, depth, label, back_rgb, back_depth, back_label, flavour="ycb", composite_rgb=None):
    """add_real_back of B frames in one launch (include/ffb6d_train.h):
      rgb uint8 [B,3,H,W], depth float32 [B,H,W], label [B,H,W] (the synthetic frame's own labels, uint8 / int32);
      back_rgb uint8 [B,3,H,W], back_depth float32 [B,H,W] (the real frame's, cast to float32 like the reference),
      back_label [B,H,W]: YCB the real frame's label image (background where <= 0), LineMOD its mask[...,0] (< 255);
      composite_rgb: None, or one flag per frame (LineMOD composites RGB with probability 0.6, linemod_dataset.py:179).
    Returns (rgb uint8 [B,3,H,W], depth float32 [B,H,W]): rgb = label <= 0 ? back_rgb * keep_back : rgb,
    depth = depth > 1e-6 ? depth : back_depth * keep_back."""
    if flavour not in FLAVOURS:
        raise ValueError(f"flavour must be one of {FLAVOURS}")
    x = _u8_images(rgb)
    _gpu(depth, label, back_rgb, back_depth, back_label)
    B, _, H, W = x.shape
    bk = _u8_images(back_rgb)
    if tuple(bk.shape) != tuple(x.shape):
        raise ValueError(f"back_rgb {tuple(bk.shape)} != rgb {tuple(x.shape)}")
    lab = _mask_u8_or_i32(label, "label", B, H, W)
    bm = _mask_u8_or_i32(back_label, "back_label", B, H, W)
    d, bd = depth.float().contiguous(), back_depth.float().contiguous()
    if tuple(d.shape) != (B, H, W) or tuple(bd.shape) != (B, H, W):
        raise ValueError("depth and back_depth must be [B,H,W]")
    flags = None
    if composite_rgb is not None:
        flags = (composite_rgb if torch.is_tensor(composite_rgb) else torch.as_tensor(np.asarray(composite_rgb, bool)))
        flags = flags.to(device=x.device, dtype=torch.uint8).reshape(-1).contiguous()
        if flags.numel() != B:
            raise ValueError(f"{flags.numel()} composite_rgb flags for {B} frames")
    out_rgb, out_d = torch.empty_like(x), torch.empty_like(d)
    lib = _lib.load()
    with torch.cuda.device(x.device), _lib.traced("add_real_back", 14 * B * H * W, (B, H, W)):
        rc = lib.ffb6d_add_real_back(x.data_ptr(), lab.data_ptr(), int(lab.dtype == torch.uint8), d.data_ptr(), bk.data_ptr(),
                                     bd.data_ptr(), bm.data_ptr(), int(bm.dtype == torch.uint8), FLAVOURS.index(flavour),
                                     flags.data_ptr() if flags is not None else None, out_rgb.data_ptr(), out_d.data_ptr(),
                                     B, H * W, _stream(x))
    _lib.check(rc, "ffb6d_add_real_back")
    return out_rgb, out_d


# ---------------------------------------------------------------------------------------------------------------------
# the whole sample
# ---------------------------------------------------------------------------------------------------------------------
def _sub(t, idx):
    return t.index_select(0, idx)


def assemble_training_batch(rgb, depth, label_img, K, n_points, cls_ids, RTs, mesh_kps, mesh_ctr, cam_scale=1.0,
                            normals=None, synthetic=None, noise_params=None, back=None, second_noise_params=None,
                            flavour="ycb", composite_rgb=None, fill_missing=False, depth_to_mm=1.0, seed=None,
                            aug_seed=None, generator=None, index_dtype=torch.int64, jitter_params=None, instances=None):
    """Decoded training frames -> the network's inputs plus the loss's targets, all on the device.
      rgb uint8 [B,3,H,W], depth float32 [B,H,W] (raw units, metres = depth / cam_scale), label_img [B,H,W] uint8 / int32,
      K intrinsics, n_points; cls_ids / RTs / mesh_kps / mesh_ctr as in pose_targets.
      jitter_params: None, or one color_jitter entry per frame (None = that frame unchanged), applied first, to real and
        synthetic frames alike: the reference jitters at decode time (ycb_dataset.py:190-193, linemod_dataset.py:221-223).
      synthetic: per-frame flags (host); for those frames, in the reference's order (ycb_dataset.py:198-204,
        linemod_dataset.py:243-249): rgb_add_noise with noise_params[b], add_real_back with back = dict(rgb=, depth=, label=)
        (the real frames, one per synthetic frame, in order) and composite_rgb, then rgb_add_noise again with
        second_noise_params[b] (None: skipped; the reference draws rand() > 0.8 for it).  Parameter lists are indexed by
        frame, entries of non-synthetic frames are ignored.
      fill_missing: inputs.fill_missing(depth, cam_scale) afterwards (YCB, ycb_dataset.py:204).
      normals: [B,3,H,W] float32, or None = inputs.depth_normal(depth * depth_to_mm, fx, fy) (YCB: depth_to_mm = 0.1).
      instances: None, or dict(inst_img=, frame_of=, class_of=, poses=) as pose_targets_instances takes them (what
        render_synthetic(..., return_inst=True) drew from): frames with several instances of one class.  The targets then come
        from pose_targets_instances; cls_ids and RTs are not used (pass None), and label_img stays the class image, which
        the compositing reads.  add_real_back pastes the real frame only where that label is background and leaves label_img
        itself alone, so the pixels an instance owns are the same before and after it: inst_img passes through untouched.
    Then the unchanged inputs.assemble_inputs (seed / generator: its sampling key; min_points=0) and pose_targets.
    Returns the input dict plus labels, rgb_labels, RTs, kp_3ds, ctr_3ds, cls_ids, kp_targ_ofst, ctr_targ_ofst.
    With `instances`: the input dict plus labels, rgb_labels, kp_targ_ofst, ctr_targ_ofst, kp_3ds [I,K,3], ctr_3ds [I,3] (per
    instance, not per slot), inst_labels i32 [B,N] (the instance of each point, -1 = none), n_points_inst i32 [I], and the
    ground truth in the form bop.BOPSceneEval.add_batch takes: gt_RT f64 [I,3,4], gt_class / gt_frame i32 [I]."""
    _gpu(rgb, depth, label_img)
    B = int(rgb.shape[0])
    dev = rgb.device
    if jitter_params is not None:
        rgb = color_jitter(rgb, jitter_params)
    syn = [] if synthetic is None else [b for b in range(B) if bool(synthetic[b])]
    if syn:
        if aug_seed is None:
            aug_seed = _inputs._seed(None, generator)
        idx = torch.tensor(syn, dtype=torch.int64, device=dev)
        srgb, sdep = _sub(rgb, idx), _sub(depth.float(), idx)
        if noise_params is not None:
            srgb = rgb_add_noise(srgb, [noise_params[b] for b in syn], aug_seed)
        if back is not None:
            flags = None if composite_rgb is None else [bool(composite_rgb[b]) for b in syn]
            srgb, sdep = add_real_back(srgb, sdep, _sub(label_img, idx), back["rgb"], back["depth"], back["label"], flavour, flags)
        if second_noise_params is not None:
            srgb = rgb_add_noise(srgb, [second_noise_params[b] for b in syn], int(aug_seed) ^ 0x5851F42D4C957F2D)
        rgb, depth = rgb.index_copy(0, idx, srgb), depth.float().index_copy(0, idx, sdep)
    if fill_missing:
        depth = _inputs.fill_missing(depth, cam_scale)
    if normals is None:
        Kn = np.asarray(K.cpu() if torch.is_tensor(K) else K, np.float64)
        if Kn.ndim == 3 and not (Kn == Kn[:1]).all():
            normals = torch.cat([_inputs.depth_normal(depth[b:b + 1] * depth_to_mm, Kn[b, 0, 0], Kn[b, 1, 1]) for b in range(B)])
        else:
            Kb = Kn.reshape(-1, 3, 3)[0]
            normals = _inputs.depth_normal(depth * depth_to_mm, Kb[0, 0], Kb[1, 1])
    inp = _inputs.assemble_inputs(rgb, depth, normals, K, n_points, cam_scale=cam_scale, generator=generator,
                                  index_dtype=index_dtype, seed=seed, min_points=0)
    out = dict(inp)
    if instances is None:
        out.update(pose_targets(inp["cld_xyz0"], inp["choose"], label_img, cls_ids, RTs, mesh_kps, mesh_ctr))
    else:
        n_cls = len(mesh_kps)
        gt_frame = _instance_ids(instances["frame_of"], "frame_of", B, dev)
        gt_class = _instance_ids(instances["class_of"], "class_of", n_cls, dev)
        _, gt_RT = _host_or_device(instances["poses"], dev, torch.float64)
        gt_RT = gt_RT.reshape(-1, 3, 4)
        tg = pose_targets_instances(inp["cld_xyz0"], inp["choose"], instances["inst_img"], gt_frame, gt_class, gt_RT, mesh_kps,
                                    mesh_ctr)
        out.update(tg, inst_labels=tg["inst_of_point"], n_points_inst=tg["n_points"], gt_RT=gt_RT, gt_class=gt_class,
                   gt_frame=gt_frame)
        del out["inst_of_point"], out["n_points"]
    out["rgb_labels"] = label_img.to(torch.int32)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# synthetic frames from meshes and poses
# ---------------------------------------------------------------------------------------------------------------------
def render_synthetic(meshes, poses, frame_of, class_of, K, B, H, W, depth_scale=1.0, min_visible=0, return_inst=False):
    """The synthetic frames the reference reads from renders/ ("render": one instance per frame) and fuse/ ("fuse": several,
    occluding one another; linemod_dataset.py:209-249), drawn on the device from meshes and poses (ffb6d_amd/render.py):
      meshes: a render.PreparedMeshes (or its list); poses [I,3,4] (model -> camera, metres), frame_of / class_of [I], K.
    Returns (rgb uint8 [B,3,H,W], depth float32 [B,H,W] = metres * depth_scale (the raw units of a sensor whose cam_scale is
    depth_scale), label int32 [B,H,W] (class id, 0 = background), ok bool [I] = the instance owns at least min_visible pixels;
    the reference discards renders below 500, rgbd_rnder_sift_kp3ds.py:80): the rgb / depth / label_img that
    assemble_training_batch(..., synthetic=...) takes.
    return_inst=True appends a fifth value, inst int32 [B,H,W]: the index into poses / frame_of / class_of of the instance that
    owns each pixel, -1 = none -- the inst_img of pose_targets_instances and of assemble_training_batch(..., instances=...)."""
    from . import render as _render
    outputs = ("rgb", "depth", "label", "visible") + (("inst",) if return_inst else ())
    out = _render.render(meshes, poses, frame_of, class_of, K, B, H, W, outputs=outputs)
    depth = out["depth"] if depth_scale == 1.0 else out["depth"] * float(depth_scale)
    ret = (out["rgb"], depth, out["label"], out["visible"] >= int(min_visible))
    return ret + (out["inst"],) if return_inst else ret
