"""numpy restatement of ffb6d_pose_targets_inst (include/ffb6d_train.h), written out as loops and in double: the rule the kernels of
csrc/train_inst.hip are held to bit for bit, and the seeded case the CPU (emulator) and GPU tests share.  Test infrastructure only."""
import functools

import numpy as np


def pose_targets_inst_ref(cld, choose, inst_img, frame_of, class_of, poses, mesh_kps, mesh_ctr):
    """cld f32 [B,N,3], choose int [B,N], inst_img i32 [B,HW], frame_of / class_of i32 [I], poses f64 [I,3,4], mesh_kps f32
    [n_cls,K,3], mesh_ctr f32 [n_cls,3] -> dict of the call's seven outputs in their own dtypes."""
    B, N = choose.shape
    HW = inst_img.shape[1]
    n_inst, n_cls, K = len(frame_of), mesh_kps.shape[0], mesh_kps.shape[1]
    kp3d, ctr3d = np.zeros((n_inst, K, 3), np.float64), np.zeros((n_inst, 3), np.float64)
    exists = np.zeros(n_inst, bool)
    for i in range(n_inst):
        c = int(class_of[i])
        exists[i] = 0 <= int(frame_of[i]) < B and 1 <= c < n_cls
        if not exists[i]:
            continue
        rt = poses[i].astype(np.float64)
        for j in range(3):
            for k in range(K):
                m = mesh_kps[c, k].astype(np.float64)
                kp3d[i, k, j] = ((m[0] * rt[j, 0] + m[1] * rt[j, 1]) + m[2] * rt[j, 2]) + rt[j, 3]
            m = mesh_ctr[c].astype(np.float64)
            ctr3d[i, j] = ((m[0] * rt[j, 0] + m[1] * rt[j, 1]) + m[2] * rt[j, 2]) + rt[j, 3]
    labels, inst = np.zeros((B, N), np.int32), np.full((B, N), -1, np.int32)
    kp_t, ctr_t = np.zeros((B, N, K, 3), np.float32), np.zeros((B, N, 3), np.float32)
    n_points = np.zeros(n_inst, np.int32)
    for b in range(B):
        for n in range(N):
            idx = int(choose[b, n])
            if not 0 <= idx < HW:
                continue
            i = int(inst_img[b, idx])
            if not (0 <= i < n_inst and exists[i] and int(frame_of[i]) == b):
                continue
            labels[b, n], inst[b, n] = class_of[i], i
            n_points[i] += 1
            p = cld[b, n].astype(np.float64)
            for j in range(3):
                kp_t[b, n, :, j] = (p[j] - kp3d[i, :, j]).astype(np.float32)        # every k: one double subtraction, one rounding
                ctr_t[b, n, j] = np.float32(p[j] - ctr3d[i, j])
    return dict(labels=labels, inst_of_point=inst, kp_targ_ofst=kp_t, ctr_targ_ofst=ctr_t, kp_3ds=kp3d.astype(np.float32),
                ctr_3ds=ctr3d.astype(np.float32), n_points=n_points)


OUTPUTS = ("labels", "inst_of_point", "kp_targ_ofst", "ctr_targ_ofst", "kp_3ds", "ctr_3ds", "n_points")
B, N, H, W, N_CLS = 3, 1061, 24, 32, 5          # N: no multiple of a workgroup's 128 points, nor of 4


def _rotation(rng):
    q = rng.randn(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_case(n_inst, K, choose_dtype=np.int64, seed=0):
    """The case of the bit-equality tests: B = 3 frames of 24 x 32 pixels, N = 1061 points, n_cls = 5.  With n_inst = 70 the list
    holds an instance that owns no pixel (3), one whose frame_of names another frame than the pixels that carry its index (4),
    one of class 0 (5) and one of class n_cls (6); the instance images hold -1 and indices >= I, choose holds -1 and HW."""
    rng = np.random.RandomState(1000 * n_inst + K + seed)
    HW = H * W
    mesh_kps = ((rng.rand(N_CLS, K, 3) - 0.5) * 0.2).astype(np.float32)
    mesh_ctr = ((rng.rand(N_CLS, 3) - 0.5) * 0.02).astype(np.float32)
    frame_of = rng.randint(0, B, n_inst).astype(np.int32)
    class_of = rng.randint(1, N_CLS, n_inst).astype(np.int32)
    poses = np.zeros((n_inst, 3, 4))
    for i in range(n_inst):
        poses[i, :, :3], poses[i, :, 3] = _rotation(rng), [rng.randn() * 0.3, rng.randn() * 0.3, 0.8 + 0.5 * rng.rand()]
    inst_img = np.full((B, HW), -1, np.int32)
    for b in range(B):
        own = np.nonzero(frame_of == b)[0]
        own = own[own != 3]                                              # instance 3 owns no pixel
        draw = rng.rand(HW)
        if len(own):
            inst_img[b] = np.where(draw < 0.7, own[rng.randint(0, len(own), HW)], -1)
        inst_img[b, draw > 0.97] = n_inst + rng.randint(0, 3)           # an index past the list
        inst_img[b, (draw > 0.94) & (draw <= 0.97)] = -7
    if n_inst > 6:
        class_of[5], class_of[6] = 0, N_CLS
        wrong = (int(frame_of[4]) + 1) % B
        inst_img[wrong, rng.choice(HW, 40, replace=False)] = 4          # painted into another frame than its own
        for i in (5, 6):
            inst_img[frame_of[i], rng.choice(HW, 40, replace=False)] = i
    choose = rng.randint(0, HW, (B, N)).astype(choose_dtype)
    choose[:, 17], choose[:, 500], choose[0, N - 1], choose[2, 0] = -1, HW, HW, -1
    cld = (rng.randn(B, N, 3) * 0.3 + [0, 0, 1.0]).astype(np.float32)
    return dict(cld=cld, choose=choose, inst_img=inst_img, frame_of=frame_of, class_of=class_of, poses=poses, mesh_kps=mesh_kps,
                mesh_ctr=mesh_ctr)


@functools.lru_cache(maxsize=None)
def case_and_reference(n_inst, K):
    """(make_case(n_inst, K), its restated outputs), computed once per process and read-only: the tests share them."""
    c = make_case(n_inst, K)
    ref = pose_targets_inst_ref(**c)
    for a in list(c.values()) + list(ref.values()):
        a.setflags(write=False)
    return c, ref


def one_per_class_case(K=8, seed=0):
    """At most one instance per (frame, class): the same scene as the instance call and as ffb6d_pose_targets take it.
    -> (instance-call arguments, dict(label_img u8 [B,HW], cls_ids i32 [B,O], RTs f64 [B,O,3,4]))."""
    rng = np.random.RandomState(77 + seed)
    HW, O = H * W, N_CLS - 1
    c = make_case(0, K, seed=seed)
    frame_of = np.repeat(np.arange(B), O).astype(np.int32)
    class_of = np.concatenate([rng.permutation(np.arange(1, N_CLS)) for _ in range(B)]).astype(np.int32)
    keep = rng.rand(B * O) < 0.8                                         # some classes are absent from some frames
    frame_of, class_of = frame_of[keep], class_of[keep]
    n_inst = len(frame_of)
    poses = np.zeros((n_inst, 3, 4))
    for i in range(n_inst):
        poses[i, :, :3], poses[i, :, 3] = _rotation(rng), [rng.randn() * 0.3, rng.randn() * 0.3, 0.8 + 0.5 * rng.rand()]
    inst_img = np.full((B, HW), -1, np.int32)
    label_img = np.zeros((B, HW), np.uint8)
    cls_ids, RTs = np.zeros((B, O), np.int32), np.zeros((B, O, 3, 4))
    for b in range(B):
        own = np.nonzero(frame_of == b)[0]
        pick = own[rng.randint(0, len(own), HW)]
        fg = rng.rand(HW) < 0.7
        inst_img[b] = np.where(fg, pick, -1)
        label_img[b] = np.where(fg, class_of[pick], 0)
        cls_ids[b, :len(own)], RTs[b, :len(own)] = class_of[own], poses[own]
    c.update(inst_img=inst_img, frame_of=frame_of, class_of=class_of, poses=poses)
    return c, dict(label_img=label_img, cls_ids=cls_ids, RTs=RTs)


def two_of_a_class_case(K=8):
    """Frame 0 holds two instances of class 2 (and one of class 1): left and right half of the image.
    -> (instance-call arguments, dict(label_img, cls_ids, RTs) with one slot per instance)."""
    rng = np.random.RandomState(5)
    HW = H * W
    c = make_case(0, K)
    frame_of, class_of = np.array([0, 0, 0], np.int32), np.array([2, 1, 2], np.int32)
    poses = np.zeros((3, 3, 4))
    for i in range(3):
        poses[i, :, :3], poses[i, :, 3] = _rotation(rng), [-0.3 + 0.3 * i, 0.05 * i, 1.0]
    inst_img = np.full((B, H, W), -1, np.int32)
    inst_img[0, :, :10], inst_img[0, :, 12:20], inst_img[0, :, 22:] = 0, 1, 2
    inst_img = inst_img.reshape(B, HW)
    label_img = np.where(inst_img >= 0, class_of[np.clip(inst_img, 0, 2)], 0).astype(np.uint8)
    cls_ids, RTs = np.zeros((B, 3), np.int32), np.zeros((B, 3, 3, 4))
    cls_ids[0], RTs[0] = class_of, poses
    c.update(inst_img=inst_img, frame_of=frame_of, class_of=class_of, poses=poses)
    return c, dict(label_img=label_img, cls_ids=cls_ids, RTs=RTs)
