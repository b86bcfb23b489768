"""numpy restatements the training-sample kernels (ffb6d_amd/csrc/train_data.hip) are checked against.  OpenCV is not
available here: the HSV round trip restates OpenCV's 8-bit RGB2HSV_b / HSV2RGB_b (color_hsv.simd.hpp) and the filters are
restated in float64 (filter2D, BORDER_REFLECT_101); get_pose_gt_info is restated in float64 (ycb_dataset.py:348-386)."""
import numpy as np


def _cv_round(x):
    return np.rint(x)                       # cvRound: round half to even


def hsv_jitter_ref(b, g, r, fs, fv):
    """b, g, r integer arrays (plane 0 = OpenCV's "B") -> (b', g', r') uint8 after BGR2HSV, the reference's jitter
    (ycb_dataset.py:111-116) and HSV2BGR."""
    b, g, r = (np.asarray(x, np.int64) for x in (b, g, r))
    idx = np.arange(256)
    with np.errstate(divide="ignore"):
        sdiv = np.where(idx > 0, _cv_round((255 << 12) / np.maximum(idx, 1).astype(np.float64)), 0).astype(np.int64)
        hdiv = np.where(idx > 0, _cv_round((180 << 12) / (6.0 * np.maximum(idx, 1))), 0).astype(np.int64)
    v = np.maximum(np.maximum(b, g), r)
    vmin = np.minimum(np.minimum(b, g), r)
    diff = v - vmin
    s = (diff * sdiv[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + (1 << 11)) >> 12
    h = h + np.where(h < 0, 180, 0)
    s = np.minimum(255, np.floor(s.astype(np.float64) * fs).astype(np.int64))
    v = np.minimum(255, np.floor(v.astype(np.float64) * fv).astype(np.int64))

    f32 = np.float32
    S = s.astype(f32) * f32(1.0 / 255.0)
    V = v.astype(f32) * f32(1.0 / 255.0)
    H = h.astype(f32) * f32(6.0 / 180.0)
    H = np.where(H >= f32(6), H - f32(6), H).astype(f32)
    sector = np.floor(H).astype(np.int64)
    H = (H - sector.astype(f32)).astype(f32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    H = np.where(bad, f32(0), H).astype(f32)
    one = f32(1)
    tab = np.stack([V, V * (one - S), V * (one - S * H), V * (one - S * (one - H))]).astype(f32)
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    out = []
    for ch in range(3):
        x = np.take_along_axis(tab, sd[sector, ch][None], 0)[0]
        x = np.where(s == 0, V, x).astype(f32)
        out.append(np.clip(_cv_round(x * f32(255)), 0, 255).astype(np.uint8))
    return tuple(out)


def reflect101(p, n):
    if n == 1:
        return np.zeros_like(p)
    p = np.asarray(p).copy()
    while True:
        lo, hi = p < 0, p >= n
        if not (lo.any() or hi.any()):
            return p
        p = np.where(lo, -p, np.where(hi, 2 * n - 2 - p, p))


def filter_ref(img, taps):
    """img uint8 [3,H,W], taps (dy, dx, w) -> float64 [3,H,W] correlation with BORDER_REFLECT_101 (not rounded)."""
    _, H, W = img.shape
    ys, xs = np.arange(H), np.arange(W)
    acc = np.zeros(img.shape, np.float64)
    for dy, dx, w in zip(*taps):
        acc += float(w) * img[:, reflect101(ys + int(dy), H)][:, :, reflect101(xs + int(dx), W)]
    return acc


def pose_targets_ref(cld, labels_pt, cls_ids, RTs, mesh_kps, mesh_ctr):
    """get_pose_gt_info of one frame restated (ycb_dataset.py:348-386) with the object table of the C ABI: cls_ids [O]
    (0 = empty), RTs [O,3,4] float64, mesh_* by class id.  Returns float64 arrays (the reference's dtype before .astype)."""
    O, K, N = len(cls_ids), mesh_kps.shape[1], len(cld)
    RTo = np.zeros((O, 3, 4))
    kp3ds, ctr3ds, ids = np.zeros((O, K, 3)), np.zeros((O, 3)), np.zeros((O, 1))
    kp_t, ctr_t = np.zeros((N, K, 3)), np.zeros((N, 3))
    for i, c in enumerate(cls_ids):
        if c <= 0 or c >= len(mesh_kps):
            continue
        r, t = RTs[i][:, :3].astype(np.float64), RTs[i][:, 3].astype(np.float64)
        RTo[i] = RTs[i]
        ctr3ds[i] = np.dot(mesh_ctr[c][None].astype(np.float64), r.T)[0] + t
        kp3ds[i] = np.dot(mesh_kps[c].astype(np.float64), r.T) + t
        ids[i] = c
        msk = np.where(labels_pt == c)[0]
        ctr_t[msk] = (cld.astype(np.float64) - ctr3ds[i])[msk]
        kp_t[msk] = (cld.astype(np.float64)[:, None, :] - kp3ds[i][None])[msk]
    return dict(RTs=RTo, kp_3ds=kp3ds, ctr_3ds=ctr3ds, cls_ids=ids, kp_targ_ofst=kp_t, ctr_targ_ofst=ctr_t)
