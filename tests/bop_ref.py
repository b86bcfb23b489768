"""numpy restatement of the BOP pose errors stated in include/ffb6d_bop.h (there is no BOP toolkit to port: this file is what
ffb6d_amd/bop.py and csrc/bop_eval.hip are held against, bit for bit).

MSSD / MSPD are float64 with one operation per rounding, component by component in the header's order (no `@`, no dot: numpy
never fuses a multiply with an add, but a matrix product would choose its own order of sums); VSD is np.float32 throughout.
Depth images come from tests/render_ref.py.  Also here: the cases that the emulator and the device tests share."""
import numpy as np

import render_ref
from ffb6d_amd import synth

MAX_TAUS = 16
IDENTITY = (np.eye(3), np.zeros(3))


# ---------------------------------------------------------------------------------------------------------------------
# MSSD / MSPD
# ---------------------------------------------------------------------------------------------------------------------
def transform(T, x, y, z):
    """T: 12 entries (scalars or arrays that broadcast against the points), row-major [R|t]"""
    X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3]
    Y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7]
    Z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11]
    return X, Y, Z


def compose(Tg, Rs, ts):
    """gt pose [3,4] with symmetries Rs [S,3,3], ts [S,3] -> 12 arrays [S,1] (row-major [Rg'|tg'])"""
    out = []
    for i in range(3):
        a0, a1, a2 = Tg[i, 0], Tg[i, 1], Tg[i, 2]
        for j in range(3):
            out.append((a0 * Rs[:, 0, j] + a1 * Rs[:, 1, j]) + a2 * Rs[:, 2, j])
        out.append(((a0 * ts[:, 0] + a1 * ts[:, 1]) + a2 * ts[:, 2]) + Tg[i, 3])
    return [v[:, None] for v in out]


def project(K, X, Y, Z):
    return (K[0, 0] * X) / Z + K[0, 2], (K[1, 1] * Y) / Z + K[1, 2]


def mssd_mspd2_row(pts, syms, Te, Tg, K):
    """Squared MSSD and MSPD of one row.  pts [n,3] (n > 0), syms: list of (R [3,3], t [3]) (empty: the identity alone),
    Te / Tg [3,4] finite, K [3,3]."""
    p = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)
    Te, Tg, K = np.asarray(Te, np.float64), np.asarray(Tg, np.float64), np.asarray(K, np.float64)
    syms = list(syms) if len(syms) else [IDENTITY]
    Rs = np.stack([np.asarray(R, np.float64).reshape(3, 3) for R, _ in syms])
    ts = np.stack([np.asarray(t, np.float64).reshape(3) for _, t in syms])
    x, y, z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    inf = np.float64(np.inf)
    with np.errstate(all="ignore"):
        Xe, Ye, Ze = transform(Te.reshape(-1), x, y, z)
        Xg, Yg, Zg = transform(compose(Tg, Rs, ts), x, y, z)
        dx, dy, dz = Xe - Xg, Ye - Yg, Ze - Zg
        d2 = (dx * dx + dy * dy) + dz * dz
        d2 = np.where(d2 >= 0.0, d2, inf)                                        # a NaN counts as +inf
        ue, ve = project(K, Xe, Ye, Ze)
        ug, vg = project(K, Xg, Yg, Zg)
        du, dv = ue - ug, ve - vg
        p2 = du * du + dv * dv
        p2 = np.where((Ze > 0.0) & (Zg > 0.0) & (p2 >= 0.0), p2, inf)
    return d2.max(axis=1).min(), p2.max(axis=1).min()


def mssd_mspd2(models, syms, class_of, frame_of, est_T, gt_T, K):
    """models: list by class id of [n,3] arrays; syms: list by class id of lists of (R, t); K [B,3,3].
    -> mssd2, mspd2 f64 [Q]; NaN for the rows the header lists."""
    est_T, gt_T = np.asarray(est_T, np.float64).reshape(-1, 3, 4), np.asarray(gt_T, np.float64).reshape(-1, 3, 4)
    K = np.asarray(K, np.float64).reshape(-1, 3, 3)
    Q = len(class_of)
    out = np.full((2, Q), np.nan)
    for q in range(Q):
        c, b = int(class_of[q]), int(frame_of[q])
        if not (0 <= c < len(models) and 0 <= b < len(K)) or len(models[c]) == 0:
            continue
        if not (np.isfinite(est_T[q]).all() and np.isfinite(gt_T[q]).all()):
            continue
        out[:, q] = mssd_mspd2_row(models[c], syms[c], est_T[q], gt_T[q], K[b])
    return out[0], out[1]


def mssd_mspd2_matmul(pts, syms, Te, Tg, K):
    """The same two errors written the way a toolkit would, with float64 matrix products: differs from the header's order only
    in how three-term sums are associated."""
    p = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)
    Te, Tg, K = np.asarray(Te, np.float64), np.asarray(Tg, np.float64), np.asarray(K, np.float64)

    def proj(P):
        uvw = P @ K.T
        return uvw[:, :2] / uvw[:, 2:]

    Pe = p @ Te[:, :3].T + Te[:, 3]
    es, ep = [], []
    for R, t in (list(syms) if len(syms) else [IDENTITY]):
        Pg = p @ (Tg[:, :3] @ np.asarray(R, np.float64)).T + (Tg[:, :3] @ np.asarray(t, np.float64) + Tg[:, 3])
        es.append(np.linalg.norm(Pe - Pg, axis=1).max())
        ep.append(np.linalg.norm(proj(Pe) - proj(Pg), axis=1).max())
    return min(es), min(ep)


# ---------------------------------------------------------------------------------------------------------------------
# VSD
# ---------------------------------------------------------------------------------------------------------------------
def ray_dist(depth, K):
    """f32 [H,W] depth along z -> distance from the camera centre; 0 stays 0"""
    f32 = np.float32
    z = np.asarray(depth, f32)
    fx, fy, cx, cy = f32(K[0, 0]), f32(K[1, 1]), f32(K[0, 2]), f32(K[1, 2])
    H, W = z.shape
    c = np.arange(W, dtype=f32)[None, :]
    r = np.arange(H, dtype=f32)[:, None]
    with np.errstate(all="ignore"):
        X = ((c - cx) * z) / fx
        Y = ((r - cy) * z) / fy
        d = np.sqrt((X * X + Y * Y) + z * z)
    assert d.dtype == f32
    return np.where(z == 0, f32(0), d)


def vsd_row(depth_test, depth_est, depth_gt, K, diameter, delta, taus):
    """One row: -> counts i32 [2 + n_tau], vsd f64 [n_tau]"""
    f32 = np.float32
    t = np.asarray(depth_test, f32)
    with np.errstate(all="ignore"):
        t = np.where(np.isfinite(t) & (t > 0), t, f32(0))
        dt, de, dg = ray_dist(t, K), ray_dist(depth_est, K), ray_dist(depth_gt, K)
        delta = f32(delta)
        vis_gt = (dg > 0) & ((dt == 0) | (dg - dt <= delta))
        vis_est = (de > 0) & ((dt == 0) | (de - dt <= delta) | vis_gt)
        uni, inter = vis_gt | vis_est, vis_gt & vis_est
        e = np.abs(dg - de) / f32(diameter)
    assert e.dtype == f32
    n_union, n_inter = int(uni.sum()), int(inter.sum())
    taus = np.asarray(taus, f32).reshape(-1)
    assert 1 <= len(taus) <= MAX_TAUS
    with np.errstate(all="ignore"):
        cost = [int((inter & (e >= tau)).sum()) for tau in taus]
    counts = np.array([n_union, n_inter] + cost, np.int32)
    if n_union == 0:
        return counts, np.ones(len(taus))
    return counts, np.array([np.float64(c + (n_union - n_inter)) / np.float64(n_union) for c in cost])


def vsd(depth_test, depth_est, depth_gt, class_of, frame_of, K, diameters, delta, taus):
    """depth_test [B,H,W], depth_est / depth_gt [Q,H,W] -> counts i32 [Q, 2+n_tau], vsd f64 [Q, n_tau]; a row whose class or
    frame id is out of range: counts 0, vsd NaN."""
    Q, n_tau = len(class_of), len(np.asarray(taus).reshape(-1))
    K = np.asarray(K, np.float64).reshape(-1, 3, 3)
    counts, out = np.zeros((Q, 2 + n_tau), np.int32), np.full((Q, n_tau), np.nan)
    for q in range(Q):
        c, b = int(class_of[q]), int(frame_of[q])
        if 0 <= c < len(diameters) and 0 <= b < len(K):
            counts[q], out[q] = vsd_row(depth_test[b], depth_est[q], depth_gt[q], K[b], diameters[c], delta, taus)
    return counts, out


def render_alone(meshes, T, class_of, frame_of, K, H, W):
    """Row q's model rendered alone under T[q] with its frame's intrinsics -> f32 [Q,H,W]; rows with bad ids render nothing."""
    K = np.asarray(K, np.float64).reshape(-1, 3, 3)
    Q = len(class_of)
    Kq = np.stack([K[min(max(int(b), 0), len(K) - 1)] for b in frame_of]) if Q else np.zeros((0, 3, 3))
    return render_ref.render(meshes, T, np.arange(Q, dtype=np.int32), class_of, Kq, Q, H, W)["depth"]


# ---------------------------------------------------------------------------------------------------------------------
# shared cases
# ---------------------------------------------------------------------------------------------------------------------
def rot(axis, angle):
    """Rodrigues"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def near(T, rng, ang=0.05, shift=0.01):
    """A pose close to T"""
    out = np.array(T, np.float64)
    out[:, :3] = out[:, :3] @ rot(rng.randn(3), ang * rng.randn())
    out[:, 3] += shift * rng.randn(3)
    return out


POINT_COUNTS = (0, 1, 63, 257, 1000)            # below, at and across a wave and a workgroup, with a tail
BOP_K = np.stack([np.array([[572.4, 0.0, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]]),
                  np.array([[1066.8, 0.0, 312.9], [0.0, 1067.5, 241.3], [0.0, 0.0, 1.0]])])


def pack_tables(models, syms):
    """The tables as the C ABI takes them (arrays of at least one row, so that they have an address)."""
    n = [len(m) for m in models]
    ns = [len(s) for s in syms]
    flat = [s for cls in syms for s in cls]
    return dict(pts=np.ascontiguousarray(np.concatenate([np.asarray(m, np.float32).reshape(-1, 3) for m in models] + [np.zeros((1, 3), np.float32)])),
                begin=np.concatenate([[0], np.cumsum(n)]).astype(np.int64), n_cls=len(models), total=int(sum(n)), max_points=int(max(n)),
                sym_R=np.ascontiguousarray(np.stack([np.asarray(R, np.float64) for R, _ in flat] + [np.zeros((3, 3))])),
                sym_t=np.ascontiguousarray(np.stack([np.asarray(t, np.float64).reshape(3) for _, t in flat] + [np.zeros(3)])),
                sym_begin=np.concatenate([[0], np.cumsum(ns)]).astype(np.int64), Stot=int(sum(ns)), max_syms=int(max(ns)))


def mssd_case(seed=5):
    """5 classes of 0, 1, 63, 257 and 1000 points.  Symmetry sets (identity first): 1, 1, 315 (a continuous axis at the default
    step, on the 63-point class), 2 and 9 (not a multiple of the symmetry block of 8).
    rows: 7 good rows over 2 frames, some with the ground truth moved by one of the class's symmetries;
    bad: class ids 9 and -1, frame ids 2 and -1, a NaN and an infinite pose entry, the empty class, a point behind the camera
    under the estimate (MSPD +inf, MSSD finite) and one good row."""
    from ffb6d_amd import bop
    rng = np.random.RandomState(seed)
    models = [(0.05 * rng.randn(n, 3)).astype(np.float32) for n in POINT_COUNTS]
    flip = np.diag([-1.0, -1.0, 1.0, 1.0])
    nine = bop.symmetry_transforms(continuous=[((1.0, 0.0, 0.0), (0.0, 0.01, 0.0))], max_disc_step=np.pi / 9 + 1e-9)
    assert len(nine) == 9, len(nine)
    syms = [[IDENTITY], [IDENTITY], bop.symmetry_transforms(continuous=[((0.0, 0.0, 1.0), (0.0, 0.0, 0.0))]),
            bop.symmetry_transforms(discrete=[flip]), nine]
    assert [len(s) for s in syms] == [1, 1, 315, 2, 9]

    def pose():
        T = np.zeros((3, 4))
        T[:, :3] = synth.random_rotation(rng)
        T[:, 3] = [0.1 * rng.randn(), 0.1 * rng.randn(), 0.7 + 0.2 * rng.rand()]
        return T

    def with_sym(T, c, k):
        R, t = syms[c][k]
        out = T.copy()
        out[:, :3], out[:, 3] = T[:, :3] @ R, T[:, :3] @ t + T[:, 3]
        return out

    cls = [4, 2, 3, 1, 4, 3, 2]
    gt = [pose() for _ in cls]
    est = [near(T, rng) for T in gt]
    est[1] = near(with_sym(gt[1], 2, 101), rng, 0.01, 0.002)                     # near a symmetric copy: the set matters
    est[4] = with_sym(gt[4], 4, 7)
    est[5] = near(with_sym(gt[5], 3, 1), rng, 0.01, 0.002)
    rows = dict(class_of=np.array(cls, np.int32), frame_of=np.array([0, 1, 1, 0, 1, 0, 1], np.int32), est_T=np.stack(est), gt_T=np.stack(gt))

    g = [pose() for _ in range(10)]
    e = [near(T, rng) for T in g]
    e[4][1, 2] = np.nan
    g[5][0, 3] = np.inf
    e[7][:, 3] = [0.0, 0.0, 0.02]                                                # the 1000-point cloud straddles the camera plane
    bad = dict(class_of=np.array([9, -1, 3, 3, 3, 4, 0, 4, 2, 3], np.int32), frame_of=np.array([0, 1, 2, -1, 0, 1, 0, 1, 0, 2 ** 30], np.int32),
               est_T=np.stack(e), gt_T=np.stack(g))
    return dict(models=models, syms=syms, K=BOP_K, rows=rows, bad=bad)


def vsd_case(H, W, seed=3):
    """Rows over the meshes of render_ref.small_scene() in 2 frames of H x W: good rows (two sharing a frame), an estimate that
    misses the frame entirely, both renders empty, a class without a mesh, bad class and frame ids.  The test depth is the
    ground-truth scene of each frame with noise, zeros, a NaN, an inf, a negative value and an occluder in front of one object."""
    s = render_ref.small_scene()
    rng = np.random.RandomState(seed)
    meshes = s["meshes"]
    K = s["K"] * np.array([[W / 64.0], [H / 48.0], [1.0]])
    P = render_ref.pose
    R = synth.random_rotation(rng)
    gt = [P([0.02, -0.01, 0.55], R), P([0.05, 0.02, 0.42]), P([-0.1, 0.03, 0.6], R.T), P([0.26, 0.2, 0.6]), P([0.0, 0.0, 0.5]),
          P([-0.1, 0.0, 0.6]), P([0.0, 0.0, 0.5]), P([0.0, 0.0, 0.5]), P([0.0, 0.0, 0.5])]
    class_of = np.array([1, 5, 1, 5, 1, 3, 4, 9, 1], np.int32)
    frame_of = np.array([0, 0, 1, 1, 1, 0, 1, 0, 2], np.int32)
    est = [near(T, rng, 0.1, 0.01) for T in gt]
    est[3] = P([5.0, 0.0, 0.6])                                                  # misses the frame: n_union from gt alone
    est[4], gt[4] = P([0.0, 9.0, 0.5]), P([0.0, -9.0, 0.5])                      # both renders empty: 1.0
    est, gt = np.stack(est), np.stack(gt)
    scene_ok = (class_of >= 0) & (class_of < len(meshes)) & (frame_of >= 0) & (frame_of < 2)
    scene = render_ref.render(meshes, gt[scene_ok], frame_of[scene_ok], class_of[scene_ok], K, 2, H, W)["depth"]
    test = np.where(scene > 0, scene + (0.004 * rng.randn(2, H, W)).astype(np.float32), 0).astype(np.float32)
    test[0, H // 3:H // 2, W // 4:W // 2] = 0.2                                  # an occluder far in front (beyond delta)
    test[:, ::7, ::5] = 0
    test[0, 1, 1], test[0, 2, 2], test[1, 3, 3] = np.nan, np.inf, -1.0
    diameters = np.array([0.0 if m is None else 2 * np.abs(m["xyz"]).max() for m in meshes], np.float32)
    diameters[diameters == 0] = 1.0
    return dict(meshes=meshes, K=K, class_of=class_of, frame_of=frame_of, est_T=est, gt_T=gt, depth_test=test, diameters=diameters,
                B=2, H=H, W=W, delta=0.015)


def chunk_case(seed=9):
    """Classes larger than the 1024 points one workgroup takes, none a multiple of it: 2500 (three chunks, a tail of 452), 1025 (a
    tail of one point) and 1024, with 9, 2 and 1 symmetry transforms.  The LAST point of every class lies far outside the cloud, so
    the maximum over the points is found in the last chunk (`inner` is the same set without those points: its errors are smaller).
    4 rows over 2 frames."""
    from ffb6d_amd import bop
    rng = np.random.RandomState(seed)
    models = [(0.05 * rng.randn(n, 3)).astype(np.float32) for n in (2500, 1025, 1024)]
    for m in models:
        m[-1] = [0.4, -0.3, 0.2]
    syms = [bop.symmetry_transforms(continuous=[((1.0, 0.0, 0.0), (0.0, 0.01, 0.0))], max_disc_step=np.pi / 9 + 1e-9),
            bop.symmetry_transforms(discrete=[np.diag([-1.0, -1.0, 1.0, 1.0])]), [IDENTITY]]
    assert [len(s) for s in syms] == [9, 2, 1]
    gt = []
    for _ in range(4):
        T = np.zeros((3, 4))
        T[:, :3], T[:, 3] = synth.random_rotation(rng), [0.1 * rng.randn(), 0.1 * rng.randn(), 1.2 + 0.2 * rng.rand()]
        gt.append(T)

    def turned(T):                      # a pure rotation about an axis at right angles to the far point: the error grows with the radius
        out = T.copy()
        out[:, :3] = T[:, :3] @ rot([0.3, 0.4, 0.0], 0.03 + 0.02 * rng.rand())
        return out

    rows = dict(class_of=np.array([0, 1, 2, 0], np.int32), frame_of=np.array([0, 1, 1, 0], np.int32),
                est_T=np.stack([turned(T) for T in gt]), gt_T=np.stack(gt))
    return dict(models=models, inner=[m[:-1] for m in models], syms=syms, K=BOP_K, rows=rows)


def vsd_image_case(H, W, Q=3, seed=7):
    """Synthetic depth images for the comparison alone (no render): Q rows over 2 frames of H x W.  gt and est are smooth surfaces
    with holes, est shifted against gt by up to a diameter; the test depth follows gt with noise, holes, an occluder band and values
    that are not measurements.  Rows differ, and so do the ends of the frame: a wrong offset of a later run of pixels shows."""
    rng = np.random.RandomState(seed)
    r, c = np.mgrid[0:H, 0:W].astype(np.float32)
    K = np.stack([np.array([[0.9 * W, 0.0, 0.48 * W], [0.0, 0.95 * W, 0.51 * H], [0.0, 0.0, 1.0]]),
                  np.array([[1.3 * W, 0.0, 0.52 * W], [0.0, 1.2 * W, 0.47 * H], [0.0, 0.0, 1.0]])])
    frame_of = (np.arange(Q) % 2).astype(np.int32)
    class_of = (1 + np.arange(Q) % 2).astype(np.int32)
    diameters = np.array([1.0, 0.12, 0.3], np.float32)
    gt = np.stack([0.7 + 0.1 * q + 0.05 * np.sin(r / (3.0 + q)) * np.cos(c / (5.0 + q)) for q in range(Q)]).astype(np.float32)
    est = (gt + (0.08 * rng.rand(Q, 1, 1) * np.sin((r + c) / 11.0)[None] + 0.004 * rng.randn(Q, H, W))).astype(np.float32)
    gt[rng.rand(Q, H, W) < 0.3] = 0
    est[rng.rand(Q, H, W) < 0.3] = 0
    test = np.zeros((2, H, W), np.float32)
    for b in range(2):
        test[b] = 0.7 + 0.1 * b + 0.05 * np.sin(r / (3.0 + b)) * np.cos(c / (5.0 + b)) + 0.006 * rng.randn(H, W)
    test[rng.rand(2, H, W) < 0.2] = 0
    test[:, H // 2:H // 2 + max(1, H // 10)] = 0.3                                # an occluder band
    test[0, 0, 0], test[1, H - 1, W - 1], test[0, H - 1, 0] = np.nan, np.inf, -1.0
    return dict(K=K, class_of=class_of, frame_of=frame_of, depth_test=test, depth_est=est, depth_gt=gt, diameters=diameters, B=2, H=H, W=W,
                delta=0.015)


# frames for the comparison alone: more than the 4096 pixels one workgroup takes and no multiple of it -- 97 x 131 = 12 707 (odd:
# single floats, a tail of 419 pixels in the fourth run), 96 x 132 = 12 672 (16-byte accesses, a tail of 384) -- and 480 x 641
# (480 x 640 is 75 runs exactly), whose 76 runs are more than the 64 lanes that add the partial counts of a row
VSD_IMAGE_SIZES = ((97, 131), (96, 132), (480, 641))

TAUS10 = np.arange(0.05, 0.51, 0.05)
TAU_SETS = {1: np.array([0.2]), 10: TAUS10, 16: np.linspace(0.02, 0.5, 16)}
