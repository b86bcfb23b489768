"""Seeded synthetic RGB-D frames and synthetic weights (numpy only, no GPU, no dataset).

There is no network or dataset on the build/bench machines, so every test, golden vector
and benchmark runs on frames generated here (SURVEY.md section 8d / BASELINE.md section 3):

  depth   z(y,x) = 1.0 + 0.3*sin(x/37)*cos(y/29) + 0.002*N(0,1) metres, 5 % of pixels
          zeroed (invalid depth); the noise keeps point-to-point distances tie-free
  xyz     back-projection with the LineMOD intrinsics exactly as `dpt_2_pcld`
          (ffb6d/datasets/linemod/linemod_dataset.py:188-199; float64 maths, cast to f32
          where the reference casts: knn.pyx:95-96, linemod_dataset.py:325)
  choose  the first N entries of a seeded permutation of the valid pixels (the reference
          samples N valid pixels and shuffles them once, linemod_dataset.py:264-282)
  rgb     uint8 uniform noise; normals: normalised N(0,1)^3
  cld_rgb_nrm = [xyz, rgb at the chosen pixels, normals at the chosen pixels]  [9,N]
                (linemod_dataset.py:284-289)

Seeds follow `1000*config + sample`.
"""
import zlib

import numpy as np

LINEMOD_K = np.array([[572.4114, 0.0, 325.2611],
                      [0.0, 573.57043, 242.04899],
                      [0.0, 0.0, 1.0]])  # ffb6d/common.py:144-146


def frame_seed(config, sample):
    return 1000 * int(config) + int(sample)


def make_frame(seed, n_points=12288, height=480, width=640, invalid_frac=0.05, K=LINEMOD_K):
    """One synthetic RGB-D frame as the dataset would hand it over (numpy, CPU).

    Returns dict: rgb u8 [3,H,W]; dpt_xyz f32 [3,H,W]; cld f32 [N,3];
    cld_rgb_nrm f32 [9,N]; choose i32 [1,N].
    """
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[:height, :width]
    z = 1.0 + 0.3 * np.sin(xs / 37.0) * np.cos(ys / 29.0) + 0.002 * rng.standard_normal((height, width))
    dpt = z.astype(np.float32)
    dpt[rng.random_sample((height, width)) < invalid_frac] = 0.0
    # dpt_2_pcld: xmap = row index, ymap = column index (linemod_dataset.py:35-36)
    msk = (dpt > 1e-8).astype(np.float32)
    row = (xs - K[0][2]) * dpt / K[0][0]
    col = (ys - K[1][2]) * dpt / K[1][1]
    dpt_xyz = np.concatenate((row[..., None], col[..., None], dpt[..., None]), axis=2)
    dpt_xyz = (dpt_xyz * msk[:, :, None]).astype(np.float32)  # [H,W,3]

    valid = (dpt.reshape(-1) > 1e-6).nonzero()[0]
    if valid.size < n_points:
        raise ValueError(f"only {valid.size} valid pixels for n_points={n_points}")
    choose = valid[rng.permutation(valid.size)[:n_points]].astype(np.int32)

    rgb = rng.randint(0, 256, size=(height, width, 3)).astype(np.uint8)
    nrm = rng.standard_normal((height, width, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(np.float32)

    cld = dpt_xyz.reshape(-1, 3)[choose, :]
    rgb_pt = rgb.reshape(-1, 3)[choose, :].astype(np.float32)
    nrm_pt = nrm.reshape(-1, 3)[choose, :]
    cld_rgb_nrm = np.concatenate((cld, rgb_pt, nrm_pt), axis=1).transpose(1, 0)
    return dict(
        rgb=np.ascontiguousarray(rgb.transpose(2, 0, 1)),
        dpt_xyz=np.ascontiguousarray(dpt_xyz.transpose(2, 0, 1)),
        cld=np.ascontiguousarray(cld, dtype=np.float32),
        cld_rgb_nrm=np.ascontiguousarray(cld_rgb_nrm, dtype=np.float32),
        choose=choose[None, :].copy(),
    )


def make_targets(seed, cld, n_classes=22, n_kps=8, n_objects=3, radius=0.12):
    """Synthetic training targets of one frame with the dataset's shapes and meaning (linemod_dataset.py:291-297,
    ycb_dataset.py:214-252): `n_objects` spheres of `radius` metres around seeded surface points, each with a class id in
    [1, n_classes) and n_kps keypoints; labels [N] int32 = class of the sphere a point falls in (0 = background; the nearest centre
    wins), kp_targ_ofst [N,n_kps,3] / ctr_targ_ofst [N,1,3] = keypoint / centre minus point for the points of an object, 0 elsewhere.
    Its own random stream (seed + 7919): make_frame's values and the golden fixtures built from them do not change."""
    rng = np.random.RandomState(seed + 7919)
    n = cld.shape[0]
    centres = cld[rng.choice(n, size=n_objects, replace=False)].astype(np.float64)
    classes = rng.choice(np.arange(1, max(n_classes, 2)), size=n_objects, replace=n_classes - 1 < n_objects)
    kps = centres[:, None, :] + 0.05 * rng.standard_normal((n_objects, n_kps, 3))
    d = np.linalg.norm(cld[:, None, :].astype(np.float64) - centres[None], axis=2)          # [N, objects]
    owner = d.argmin(axis=1)
    inside = d[np.arange(n), owner] < radius
    labels = np.where(inside, classes[owner], 0).astype(np.int32)
    kp_targ = np.where(inside[:, None, None], kps[owner] - cld[:, None, :], 0.0).astype(np.float32)
    ctr_targ = np.where(inside[:, None, None], centres[owner][:, None, :] - cld[:, None, :], 0.0).astype(np.float32)
    return dict(labels=labels, kp_targ_ofst=kp_targ, ctr_targ_ofst=ctr_targ)


def make_batch(config, batch_size, **kw):
    """Stack `batch_size` frames with seeds 1000*config + sample."""
    frames = [make_frame(frame_seed(config, s), **kw) for s in range(batch_size)]
    return {k: np.stack([f[k] for f in frames], axis=0) for k in frames[0]}


def strided_grids(dpt_xyz):
    """`sr2dptxyz` of linemod_dataset.py:299-311: xyz image sub-sampled at stride 1,2,4,8,
    pixel (y*s, x*s), flattened to [G_s,3].  dpt_xyz: [3,H,W] or [B,3,H,W]."""
    out = {}
    for s in (1, 2, 4, 8):
        h, w = dpt_xyz.shape[-2] // s, dpt_xyz.shape[-1] // s
        g = dpt_xyz[..., : h * s : s, : w * s : s]
        g = g.reshape(*g.shape[:-2], -1)
        out[s] = np.ascontiguousarray(np.swapaxes(g, -1, -2))
    return out


# ------------------------------------------------------------------------------------
# synthetic weights: deterministic per parameter NAME, so the reference model (golden
# generation, build container) and our modules (GPU box) get identical values without
# shipping a 135 MB checkpoint.
# ------------------------------------------------------------------------------------
def _tensor_seed(name, seed):
    return (zlib.crc32(name.encode("utf-8")) ^ (seed * 2654435761)) & 0x7FFFFFFF


def synth_tensor(name, shape, seed=0):
    """float32/int64 numpy array for state-dict entry `name` (shape from the module).

    The values are chosen so that activations stay O(1)-O(100) through the ~110 layers, as a
    trained network's do: He-normal conv weights, BatchNorm statistics close to identity, a
    small gain on the last BatchNorm of every residual block (otherwise the 16 residual adds
    grow the signal by 2^16 and the softmax poolings see logits of 1e6, which makes the
    network chaotic and every fp32 comparison meaningless), and the two input layers scaled
    for raw 0..255 colour values."""
    rng = np.random.RandomState(_tensor_seed(name, seed))
    shape = tuple(int(s) for s in shape)
    leaf = name.rsplit(".", 1)[-1]
    if leaf == "num_batches_tracked":
        return np.zeros(shape, dtype=np.int64)
    if leaf == "running_var":
        return rng.uniform(0.8, 1.25, size=shape).astype(np.float32)
    if leaf == "running_mean":
        return (0.1 * rng.standard_normal(shape)).astype(np.float32)
    if leaf == "bias":
        return (0.05 * rng.standard_normal(shape)).astype(np.float32)
    if len(shape) <= 1:  # BatchNorm gamma / PReLU slope
        if shape == (1,):
            return np.full(shape, 0.25, dtype=np.float32)
        if name.endswith(".bn2.weight"):          # residual-branch gain
            return rng.uniform(0.1, 0.3, size=shape).astype(np.float32)
        return rng.uniform(0.8, 1.2, size=shape).astype(np.float32)
    fan_in = int(np.prod(shape[1:]))
    w = (rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)).astype(np.float32)
    if name == "cnn_pre_stages.0.weight":          # consumes raw 0..255 rgb
        w *= np.float32(0.01)
    if name == "rndla_pre_stages.conv.weight":     # channels 3..5 of cld_rgb_nrm are raw rgb
        w[:, 3:6] *= np.float32(0.01)
    return w


def synth_state_dict(module, seed=0):
    """Deterministic state dict for a torch module with the reference's key names.
    Entries that alias the same storage (the reference shares `cnn.final` between
    cnn_up_stages[2] and [3], ffb6d.py:86-87) get the values of the first alias."""
    import torch

    out, first_name = {}, {}
    for name, t in module.state_dict().items():
        key = (t.data_ptr(), tuple(t.shape)) if t.numel() > 0 else (name, ())
        src = first_name.setdefault(key, name)
        out[name] = torch.from_numpy(synth_tensor(src, t.shape, seed)).to(t.dtype)
    return out


# parameters that alias one tensor in the reference model: `cnn.final` is registered under
# both cnn_up_stages[2] and cnn_up_stages[3] (ffb6d.py:86-87)
REFERENCE_ALIASES = {
    "cnn_up_stages.3.1.0.weight": "cnn_up_stages.2.0.0.weight",
    "cnn_up_stages.3.1.0.bias": "cnn_up_stages.2.0.0.bias",
}


def synth_state_dict_from_shapes(shapes, seed=0, n_classes=None):
    """Same values as synth_state_dict(reference_model), built from a {name: shape} map
    (tests/golden/state_dict_keys.json) instead of a module.  `n_classes` overrides the
    output width of the segmentation head (the only class-count dependent tensors)."""
    import torch

    out = {}
    for name, shape in shapes.items():
        shape = list(shape)
        if n_classes is not None and name.startswith("rgbd_seg_layer.3.conv."):
            shape[0] = n_classes
        src = REFERENCE_ALIASES.get(name, name)
        a = synth_tensor(src, shape, seed)
        out[name] = torch.from_numpy(a)
    return out


# --------------------------------------------------------------------------------------
# Pose-solver cases: what FFB6D.forward hands to
# cal_frame_poses[_lm] (ffb6d/utils/pvn3d_eval_utils_kpls.py:65-158,220-285), synthesised:
# objects = rigidly placed blobs of the cloud, votes = true offsets + noise + outliers.
# --------------------------------------------------------------------------------------
def random_rotation(rng):
    q = rng.randn(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_pose_case(seed, n_pts=2048, n_obj=2, n_kps=8, n_cls=None, noise=0.004, outliers=0.1,
                   label_noise=0.02, bg_frac=0.3, mesh_seed=None):
    """Returns a dict of numpy arrays:
      pcld f32[N,3], mask i64[N] (0 = background, 1..n_obj), ctr_of f32[1,N,3], kp_of f32[n_kps,N,3]
      mesh_kps f32[n_cls,n_kps,3], mesh_ctr f32[n_cls,3] (row = class id, row 0 unused),
      r_lst f32[n_cls-1] object radii, RT f64[n_cls,3,4] the true poses."""
    rng = np.random.RandomState(seed)
    n_cls = n_cls or n_obj + 1
    mrng = rng if mesh_seed is None else np.random.RandomState(mesh_seed)   # frames of one batch share the meshes
    mesh_kps = (mrng.rand(n_cls, n_kps, 3).astype(np.float32) - 0.5) * 0.2
    mesh_ctr = (mrng.rand(n_cls, 3).astype(np.float32) - 0.5) * 0.02
    r_lst = (0.08 + 0.05 * mrng.rand(n_cls - 1)).astype(np.float32)
    RT = np.zeros((n_cls, 3, 4))
    pcld = np.zeros((n_pts, 3), np.float32)
    mask = np.zeros((n_pts,), np.int64)
    ctr_of = np.zeros((1, n_pts, 3), np.float32)
    kp_of = np.zeros((n_kps, n_pts, 3), np.float32)
    owner = rng.choice(n_obj + 1, size=n_pts, p=[bg_frac] + [(1 - bg_frac) / n_obj] * n_obj)
    for c in range(1, n_obj + 1):
        R = random_rotation(rng)
        t = np.array([0.5 * (c - (n_obj + 1) / 2), 0.1 * rng.randn(), 1.0 + 0.2 * rng.rand()])
        RT[c, :, :3], RT[c, :, 3] = R, t
    for i in range(n_pts):
        c = owner[i]
        if c == 0:
            pcld[i] = [rng.uniform(-1, 1), rng.uniform(-0.6, 0.6), rng.uniform(0.6, 1.6)]
            ctr_of[0, i] = 0.2 * rng.randn(3)
            kp_of[:, i] = 0.2 * rng.randn(n_kps, 3)
            continue
        R, t = RT[c, :, :3], RT[c, :, 3]
        local = rng.randn(3)
        local *= 0.07 * rng.rand() ** (1 / 3) / np.linalg.norm(local)
        p = R @ local + t
        pcld[i] = p
        mask[i] = c
        ctr_of[0, i] = p - (R @ mesh_ctr[c] + t) + noise * rng.randn(3)
        kp_of[:, i] = p[None] - (mesh_kps[c] @ R.T + t) + noise * rng.randn(n_kps, 3)
        if rng.rand() < outliers:
            ctr_of[0, i] += 0.15 * rng.randn(3)
            kp_of[:, i] += 0.15 * rng.randn(n_kps, 3)
    flip = rng.rand(n_pts) < label_noise                      # segmentation mistakes
    mask[flip] = rng.randint(0, n_obj + 1, size=int(flip.sum()))
    return dict(pcld=pcld, mask=mask, ctr_of=ctr_of.astype(np.float32), kp_of=kp_of.astype(np.float32),
                mesh_kps=mesh_kps, mesh_ctr=mesh_ctr, r_lst=r_lst, RT=RT)


# ---- pose evaluation (ADD / ADD-S): model clouds and pose pairs ------------------------------------------------
def model_cloud(seed, n_pts):
    """An object-sized model cloud f32 [n_pts,3] (metres): an anisotropic blob of about 0.1 m."""
    rng = np.random.RandomState(seed)
    return (rng.randn(n_pts, 3) * [0.04, 0.025, 0.015]).astype(np.float32)


def ring_model(seed, n_pts, k):
    """A k-fold rotation-symmetric model f32 [n_pts,3] (n_pts divisible by k): n_pts / k seeded points and their copies
    rotated by multiples of 2 pi / k about z, so rotating the model by `ring_angle(k)` maps it onto itself."""
    rng = np.random.RandomState(seed)
    base = np.stack([0.04 + 0.01 * rng.rand(n_pts // k), 0.002 * rng.randn(n_pts // k), 0.02 * rng.randn(n_pts // k)], 1)
    return np.concatenate([base @ rot_z(j * ring_angle(k)).T for j in range(k)]).astype(np.float32)


def ring_angle(k):
    return 2.0 * np.pi / k


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def eval_pose_pair(seed, kind="near"):
    """(pred f32 [3,4], gt f32 [3,4]) [R|t] pairs: kind = 'near' (a few degrees / centimetres off), 'far' (unrelated
    poses), 'zero' (an all-zero prediction: the reference's undetected object) or 'same' (identical bits)."""
    rng = np.random.RandomState(seed)
    gt = np.zeros((3, 4))
    gt[:, :3], gt[:, 3] = random_rotation(rng), [0.1 * rng.randn(), 0.1 * rng.randn(), 0.8 + 0.4 * rng.rand()]
    if kind == "same":
        pred = gt.copy()
    elif kind == "zero":
        pred = np.zeros((3, 4))
    elif kind == "far":
        pred = np.zeros((3, 4))
        pred[:, :3], pred[:, 3] = random_rotation(rng), gt[:, 3] + 0.2 * rng.randn(3)
    else:
        axis = rng.randn(3)
        axis /= np.linalg.norm(axis)
        a = np.deg2rad(3.0 * rng.rand())
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        dR = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
        pred = np.zeros((3, 4))
        pred[:, :3], pred[:, 3] = dR @ gt[:, :3], gt[:, 3] + 0.01 * rng.randn(3)
    return pred.astype(np.float32), gt.astype(np.float32)


def pose_case_ground_truth(case, extra_seed=None):
    """Ground truth of a make_pose_case frame in the layout of a YCB test batch: cls_ids i64 [n,1], RTs f32 [n,3,4],
    gt_kps f32 [n,n_kps,3] (mesh keypoints under the true pose) for the objects 1..n_obj.  extra_seed: also one object
    of class n_obj + 1 that no prediction has, then a row of class 0 (end of the list) and a row after it that the
    evaluation must not reach."""
    n_obj = int(case["mask"].max())
    RT = case["RT"]
    ids = list(range(1, n_obj + 1))
    RTs = [RT[c] for c in ids]
    kps = [case["mesh_kps"][c] @ RT[c, :, :3].T + RT[c, :, 3] for c in ids]
    if extra_seed is not None:
        _, gt = eval_pose_pair(extra_seed, "near")
        ids += [n_obj + 1, 0, 1]
        RTs += [gt, np.zeros((3, 4)), RT[1]]
        kps += [kps[0] + 0.05, np.zeros_like(kps[0]), kps[0]]
    return (np.asarray(ids, np.int64).reshape(-1, 1), np.asarray(RTs).astype(np.float32),
            np.asarray(kps).astype(np.float32))


# ---- rendering: vertex-coloured triangle meshes ----------------------------------------------------------------
def sphere_mesh(subdiv, radius=0.1, seed=0):
    """An icosphere as a vertex-coloured triangle mesh: dict(xyz f32 [V,3] on the sphere of `radius` metres, rgb u8 [V,3]
    seeded colours, faces i32 [F,3] wound counter-clockwise seen from outside), F = 20 * 4^subdiv, V = 10 * 4^subdiv + 2.
    Every subdivision cuts each triangle into four at its edge midpoints, pushed out to the sphere."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    verts = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
             (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    verts = [np.asarray(v, np.float64) / np.sqrt(1.0 + g * g) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
             (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
             (9, 8, 1)]
    for _ in range(int(subdiv)):
        mid = {}

        def midpoint(a, b):
            key = (a, b) if a < b else (b, a)
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        nxt = []
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nxt
    rng = np.random.RandomState(seed)
    xyz = (np.asarray(verts) * float(radius)).astype(np.float32)
    return dict(xyz=xyz, rgb=rng.randint(0, 256, (len(xyz), 3)).astype(np.uint8), faces=np.asarray(faces, np.int32))


# ---- multi-instance scenes: several posed instances of a few asymmetric objects --------------------------------
def bumpy_mesh(seed, radius=0.05, subdiv=2):
    """An object without any symmetry, so that its pose is unambiguous: the icosphere of `sphere_mesh` scaled unequally along
    its three axes (seeded, the longest half-axis = `radius` metres) with one bump, a seeded direction around which the surface
    is pushed out by up to 35 %.  Same dict as sphere_mesh."""
    rng = np.random.RandomState(seed + 4099)
    m = sphere_mesh(subdiv, 1.0, seed=seed)
    unit = m["xyz"].astype(np.float64)
    scale = np.array([1.0, 0.55 + 0.2 * rng.rand(), 0.35 + 0.15 * rng.rand()])[rng.permutation(3)]
    d = rng.randn(3)
    d /= np.linalg.norm(d)
    bump = 1.0 + 0.35 * np.clip((unit @ d - 0.6) / 0.4, 0.0, 1.0)
    xyz = unit * scale * bump[:, None]
    m["xyz"] = (xyz * (radius / np.linalg.norm(xyz, axis=1).max())).astype(np.float32)
    return m


def make_instance_scene(seed, instances=((1, 1, 1, 2), (1, 1)), n_classes=None, height=120, width=160, n_kps=8, radius=0.08,
                        depth=(0.6, 0.8), bandwidth=0.04, overlap=False, K=None):
    """A seeded scene with several instances of one class in a frame: what render.render / train_data.render_synthetic draw and
    train_data.pose_targets_instances labels.  instances[b] lists the class ids (1 ..) of frame b's instances.
      meshes     list by class id (None for class 0) of bumpy_mesh objects whose longest half-axis is `radius`
      poses f64 [I,3,4], frame_of / class_of i32 [I]: the renderer's instance list, in the order of `instances`
      K f64 [B,3,3]: the LineMOD intrinsics scaled to height x width (or the given [3,3])
      mesh_kps f32 [n_cls,n_kps,3] seeded mesh vertices, mesh_ctr f32 [n_cls,3] the bounding-box centres, r_lst f32 [n_cls-1]
      object radii, diameters f32 [n_cls] (index 0 unused, 1.0).
    Placement (rejection sampling): rotations are uniform, centres lie at `depth` metres; the centres of two instances of a frame
    are at least max(4 * bandwidth, 2 object radii) apart (4 bandwidths of the solver's mean shift, pose.RADIUS, keep their
    centre clusters separate); every instance's bounding sphere projects inside the frame; and unless `overlap`, no two bounding
    spheres of a frame overlap in the image, so that every instance is seen whole."""
    rng = np.random.RandomState(seed)
    B = len(instances)
    n_cls = int(n_classes or max(max(f) for f in instances if len(f)) + 1)
    meshes = [None] + [bumpy_mesh(seed * 31 + c, radius) for c in range(1, n_cls)]
    if K is None:
        K = LINEMOD_K * np.array([[width / 640.0], [height / 480.0], [1.0]])
    K = np.asarray(K, np.float64)
    mesh_kps, mesh_ctr = np.zeros((n_cls, n_kps, 3), np.float32), np.zeros((n_cls, 3), np.float32)
    r_lst, diameters = np.zeros(n_cls - 1, np.float32), np.ones(n_cls, np.float32)
    for c in range(1, n_cls):
        v = meshes[c]["xyz"]
        mesh_kps[c] = v[rng.choice(len(v), n_kps, replace=False)]
        mesh_ctr[c] = (v.min(0) + v.max(0)) / 2
        r_lst[c - 1] = np.linalg.norm(v, axis=1).max()
        diameters[c] = 2 * r_lst[c - 1]
    gap = max(4.0 * bandwidth, 2.0 * radius)
    poses, frame_of, class_of = [], [], []
    for b, classes in enumerate(instances):
        placed = []
        for c in classes:
            for _ in range(10000):
                z = rng.uniform(*depth)
                u, v = rng.uniform(0, width), rng.uniform(0, height)
                t = np.array([(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z])
                r_px = max(K[0, 0], K[1, 1]) * radius / (z - radius)          # the bounding sphere's image radius, from above
                inside = r_px <= u <= width - 1 - r_px and r_px <= v <= height - 1 - r_px
                apart = all(np.linalg.norm(t - q) >= gap for q, _, _ in placed)
                clear = overlap or all(np.hypot(u - uq, v - vq) >= r_px + rq for _, (uq, vq), rq in placed)
                if inside and apart and clear:
                    break
            else:
                raise ValueError(f"frame {b}: no room for {len(classes)} instances of radius {radius} in {height} x {width}")
            placed.append((t, (u, v), r_px))
            T = np.zeros((3, 4))
            T[:, :3], T[:, 3] = random_rotation(rng), t
            poses.append(T)
            frame_of.append(b)
            class_of.append(c)
    return dict(meshes=meshes, poses=np.asarray(poses).reshape(-1, 3, 4), frame_of=np.asarray(frame_of, np.int32),
                class_of=np.asarray(class_of, np.int32), K=np.stack([K] * B), mesh_kps=mesh_kps, mesh_ctr=mesh_ctr, r_lst=r_lst,
                diameters=diameters, B=B, H=int(height), W=int(width))
