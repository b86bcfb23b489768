"""Posed, vertex-coloured triangle meshes -> rgb / depth / label frames on the GPU: the synthetic frames that the reference
reads from disk (linemod_dataset.py:55-103,209-249, made by an external z-buffer library, rgbd_rnder_sift_kp3ds.py:38-105).
Host side of include/ffb6d_render.h, which states the algorithm; the reference carries no rasteriser source --
tests/render_ref.py is the numpy restatement the kernels are held against, bit for bit.

    meshes = render.PreparedMeshes([None, dict(xyz=..., rgb=..., faces=...), ...])        # once per object set, by class id
    out = render.render(meshes, poses, frame_of, class_of, K, B, H, W)                    # rgb, depth, label on the device

`render` enqueues its kernels on the current stream and returns device tensors: nothing is read back and the stream is never
waited for.  There is no CPU fallback: tensors must live on a GPU.
"""
import numpy as np
import torch

from . import _lib
from .ops import _need_gpu, _stream

FORM = 0               # csrc/render.hip ffb6d_render_set_form: 0 = a lane per triangle (default), 1 = a wavefront per triangle, -1 = by box area
MAX_INSTANCES, MAX_FACES = 1024, 1 << 22
OUTPUTS = {"rgb": torch.uint8, "depth": torch.float32, "label": torch.int32, "inst": torch.int32, "face": torch.int32,
           "visible": torch.int32}


def set_form(form):
    """0 lane per triangle (default) / 1 wavefront per triangle / -1 automatic; returns the previous setting.  Results do not
    depend on it."""
    global FORM
    prev, FORM = FORM, int(form)
    _lib.load().ffb6d_render_set_form(FORM)
    return prev


def _numpy(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _host(x, dtype, width, what):
    a = np.ascontiguousarray(_numpy(x), dtype).reshape(-1, width)
    if a.dtype.kind == "f" and not np.isfinite(a).all():
        raise ValueError(f"{what} holds values that are not finite")
    return a


class PreparedMeshes:
    """A mesh set on the device, once per object set.  meshes: list indexed by class id of None (no such object; class 0 is
    the background label) or dict(xyz=[V,3] metres, rgb=[V,3] uint8, faces=[F,3] vertex indices within the mesh).  Host data
    is validated (indices in range, fewer than 2^22 faces per class) and uploaded; preparing waits for nothing but the copies."""

    def __init__(self, meshes, device=None):
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.FFB6DNativeError("ffb6d_amd.render runs on the GPU only; there is no CPU fallback")
        verts, colors, faces, nv, nf = [], [], [], [], []
        for c, m in enumerate(meshes):
            if m is None:
                nv.append(0)
                nf.append(0)
                continue
            xyz, rgb, fc = _host(m["xyz"], np.float32, 3, f"meshes[{c}]['xyz']"), _numpy(m["rgb"]), _numpy(m["faces"])
            if rgb.dtype != np.uint8 or rgb.shape != xyz.shape:
                raise TypeError(f"meshes[{c}]['rgb'] must be uint8 {xyz.shape}, got {rgb.dtype} {rgb.shape}")
            if fc.dtype.kind not in "iu" or fc.ndim != 2 or fc.shape[1] != 3:
                raise TypeError(f"meshes[{c}]['faces'] must be integers [F,3], got {fc.dtype} {fc.shape}")
            if len(fc) > MAX_FACES:
                raise ValueError(f"meshes[{c}] has {len(fc)} faces, at most 2^22 per class")
            if len(fc) and (fc.min() < 0 or fc.max() >= len(xyz)):
                raise ValueError(f"meshes[{c}]['faces'] names vertices outside [0, {len(xyz)})")
            verts.append(xyz)
            colors.append(np.ascontiguousarray(rgb))
            faces.append(np.ascontiguousarray(fc, np.int32))
            nv.append(len(xyz))
            nf.append(len(fc))
        self.n_cls = len(meshes)
        if self.n_cls == 0:
            raise ValueError("an empty mesh set")
        self.n_verts, self.n_faces = np.asarray(nv, np.int64), np.asarray(nf, np.int64)
        self.Vtot, self.Ftot = int(self.n_verts.sum()), int(self.n_faces.sum())
        self.max_verts, self.max_faces = int(self.n_verts.max()), int(self.n_faces.max())
        # one spare row each, so that an empty set still has an address
        up = lambda parts, dt: torch.from_numpy(np.concatenate(parts + [np.zeros((1, 3), dt)])).to(self.device)      # noqa: E731
        self.verts, self.colors, self.faces = up(verts, np.float32), up(colors, np.uint8), up(faces, np.int32)
        self.vert_begin = torch.from_numpy(np.concatenate([[0], np.cumsum(self.n_verts)]).astype(np.int64)).to(self.device)
        self.face_begin = torch.from_numpy(np.concatenate([[0], np.cumsum(self.n_faces)]).astype(np.int64)).to(self.device)


def _prepared(meshes):
    return meshes if isinstance(meshes, PreparedMeshes) else PreparedMeshes(meshes)


def _device_array(x, dev, dtype, np_dtype):
    if torch.is_tensor(x):
        _need_gpu(x)
        return x.to(device=dev, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np_dtype))).to(dev)


def render(meshes, poses, frame_of, class_of, K, B, H, W, z_near=1e-3, outputs=("rgb", "depth", "label")):
    """Draws I instances into B frames of H x W (include/ffb6d_render.h states every formula):
      meshes: a PreparedMeshes (or the list it takes, prepared on the spot); poses [I,3,4] (model -> camera), frame_of /
      class_of [I], K [3,3] or [B,3,3]: host data (uploaded) or device tensors; z_near > 0: vertices nearer than this drop
      their triangles (there is no clipping).
      outputs: any of "rgb" u8 [B,3,H,W], "depth" f32 [B,H,W] (0 = nothing drawn), "label" i32 [B,H,W] (class id, 0 = nothing),
      "inst" i32 [B,H,W] (owning instance, -1 = none), "face" i32 [B,H,W] (face within the class), "visible" i32 [I] (pixels
      owned).
    Host-visible ids outside their range raise ValueError; device ids are not read back (such an instance draws nothing).
    Returns a dict of device tensors."""
    for t in (poses, frame_of, class_of, K):
        if torch.is_tensor(t):
            _need_gpu(t)
    meshes = _prepared(meshes)
    dev = meshes.device
    outputs = tuple(outputs)
    if not outputs or any(o not in OUTPUTS for o in outputs):
        raise ValueError(f"outputs must name some of {tuple(OUTPUTS)}, got {outputs}")
    B, H, W = int(B), int(H), int(W)
    if B <= 0 or H <= 0 or W <= 0 or B * H * W >= 1 << 31:
        raise ValueError(f"bad frame sizes B={B} H={H} W={W} (B*H*W < 2^31)")
    if not z_near > 0:
        raise ValueError(f"z_near must be positive, got {z_near}")
    for name, ids, hi in (("frame_of", frame_of, B), ("class_of", class_of, meshes.n_cls)):
        if not torch.is_tensor(ids):
            a = np.asarray(ids).reshape(-1)
            if len(a) and (a.min() < 0 or a.max() >= hi):
                raise ValueError(f"{name} outside [0, {hi})")
    frame_of = _device_array(frame_of, dev, torch.int32, np.int32).reshape(-1)
    class_of = _device_array(class_of, dev, torch.int32, np.int32).reshape(-1)
    poses = _device_array(poses, dev, torch.float64, np.float64).reshape(-1, 3, 4)
    Kd = _device_array(K, dev, torch.float64, np.float64)
    if Kd.dim() == 2:
        Kd = Kd.unsqueeze(0).expand(B, 3, 3)
    Kd = Kd.contiguous()
    if tuple(Kd.shape) != (B, 3, 3):
        raise ValueError(f"K must be [3,3] or [{B},3,3], got {tuple(Kd.shape)}")
    n_inst = int(frame_of.shape[0])
    if int(class_of.shape[0]) != n_inst or int(poses.shape[0]) != n_inst:
        raise ValueError(f"{n_inst} frames / {int(class_of.shape[0])} classes / {int(poses.shape[0])} poses")
    if n_inst > MAX_INSTANCES:
        raise ValueError(f"{n_inst} instances, at most {MAX_INSTANCES} per call")
    shapes = {"rgb": (B, 3, H, W), "visible": (n_inst,)}
    out = {o: torch.empty(shapes.get(o, (B, H, W)), dtype=OUTPUTS[o], device=dev) for o in outputs}
    ptr = lambda o: out[o].data_ptr() if o in out else None                                                                 # noqa: E731
    lib = _lib.load()
    wbytes = lib.ffb6d_render_workspace_bytes(n_inst, meshes.max_verts, B, H, W)
    ws = torch.empty((max(wbytes, 1),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _lib.traced("render", 8 * B * H * W, (n_inst, B, H, W)):
        rc = lib.ffb6d_render_f32(meshes.verts.data_ptr(), meshes.colors.data_ptr(), meshes.faces.data_ptr(), meshes.vert_begin.data_ptr(),
                                  meshes.face_begin.data_ptr(), meshes.n_cls, meshes.Vtot, meshes.Ftot, meshes.max_verts, meshes.max_faces,
                                  frame_of.data_ptr(), class_of.data_ptr(), poses.data_ptr(), n_inst, Kd.data_ptr(), B, H, W, float(z_near),
                                  ptr("rgb"), ptr("depth"), ptr("label"), ptr("inst"), ptr("face"), ptr("visible"), ws.data_ptr(), wbytes,
                                  _stream(ws))
    _lib.check(rc, "ffb6d_render_f32")
    return out
