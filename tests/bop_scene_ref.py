"""numpy restatement of include/ffb6d_bop_scene.h: instance visibility in the measured depth and the greedy matching of scored
estimates to ground-truth instances (there is no BOP toolkit to port: this file is what ffb6d_amd/bop.py and csrc/bop_scene.hip
are held against, bit for bit).  Visibility is np.float32 throughout and reuses bop_ref.ray_dist; matching is a plain Python loop.
Also here: the cases that the emulator and the device tests share."""
import numpy as np

import bop_ref

MAX_GROUP = 64
INFO_INTS = 12


# ---------------------------------------------------------------------------------------------------------------------
# visibility
# ---------------------------------------------------------------------------------------------------------------------
def measured(depth):
    """a depth that is not finite or is <= 0 counts as 0"""
    z = np.asarray(depth, np.float32)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(z) & (z > 0), z, np.float32(0)).astype(np.float32)


def bbox(sel):
    """x, y, w, h over the True pixels of sel [H,W]; -1 four times when there is none"""
    if not sel.any():
        return [-1, -1, -1, -1]
    rows, cols = np.nonzero(sel.any(axis=1))[0], np.nonzero(sel.any(axis=0))[0]
    return [int(cols[0]), int(rows[0]), int(cols[-1] - cols[0] + 1), int(rows[-1] - rows[0] + 1)]


def visib_row(depth_test, depth_obj, K, delta):
    """One row: -> info i32 [12], visib_fract f64, mask u8 [H,W]"""
    f32 = np.float32
    with np.errstate(all="ignore"):
        dt, dg = bop_ref.ray_dist(measured(depth_test), K), bop_ref.ray_dist(measured(depth_obj), K)
        delta = f32(delta)
        obj = dg > 0
        valid = obj & (dt > 0)
        visib = obj & ((dt == 0) | (dg - dt <= delta))
        support = valid & (dg - dt <= delta) & (dt - dg <= delta)
    assert (dg - dt).dtype == f32
    n_all, n_visib = int(obj.sum()), int(visib.sum())
    info = np.array([n_all, int(valid.sum()), n_visib, int(support.sum())] + bbox(obj) + bbox(visib), np.int32)
    fract = np.float64(0.0) if n_all == 0 else np.float64(n_visib) / np.float64(n_all)
    return info, fract, visib.astype(np.uint8)


def visib(depth_test, depth_obj, frame_of, K, delta):
    """depth_test [B,H,W], depth_obj [Q,H,W] -> info i32 [Q,12], visib_fract f64 [Q], mask u8 [Q,H,W]; a row whose frame id is out
    of range: counts 0, boxes -1, NaN, an all-zero mask."""
    Q = len(frame_of)
    K = np.asarray(K, np.float64).reshape(-1, 3, 3)
    info = np.tile(np.array([0] * 4 + [-1] * 8, np.int32), (Q, 1))
    fract = np.full(Q, np.nan)
    mask = np.zeros(np.asarray(depth_obj).shape, np.uint8)
    for q in range(Q):
        b = int(frame_of[q])
        if 0 <= b < len(K):
            info[q], fract[q], mask[q] = visib_row(depth_test[b], depth_obj[q], K[b], delta)
    return info, fract, mask


# ---------------------------------------------------------------------------------------------------------------------
# matching
# ---------------------------------------------------------------------------------------------------------------------
def match_group(err, score, thr, max_ests=0):
    """One group: err f64 [E,T,n_col], score f32 [E], thr f64 [n_thr] -> est_gt i32 [E,n_col,n_thr], gt_est i32 [T,n_col,n_thr]"""
    err = np.asarray(err, np.float64)
    E, T, n_col = err.shape
    thr = np.asarray(thr, np.float64).reshape(-1)
    s = np.asarray(score, np.float32).reshape(E).copy()
    s[np.isnan(s)] = -np.inf
    order = sorted(range(E), key=lambda e: (-s[e], e)) if E else []              # descending score, ties to the lower index
    considered = max_ests if 0 < max_ests < E else E
    est_gt = np.full((E, n_col, len(thr)), -1, np.int32)
    gt_est = np.full((T, n_col, len(thr)), -1, np.int32)
    for col in range(n_col):
        for k, th in enumerate(thr):
            taken = [False] * T
            for e in order[:considered]:
                best = -1
                for t in range(T):
                    v = err[e, t, col]
                    if not taken[t] and v < th and (best < 0 or v < err[e, best, col]):
                        best = t
                if best >= 0:
                    taken[best] = True
                    est_gt[e, col, k], gt_est[best, col, k] = best, e
    return est_gt, gt_est


def match(tables, err, score, thr, max_ests=None):
    """All groups of `tables` (est_begin, gt_begin, pair_begin); err [Npairs,n_col], score [Etot], thr [G,n_thr]"""
    eb, gb, pb = tables["est_begin"], tables["gt_begin"], tables["pair_begin"]
    G, n_col, n_thr = len(eb) - 1, err.shape[1], thr.shape[1]
    est_gt, gt_est = np.full((eb[-1], n_col, n_thr), -7, np.int32), np.full((gb[-1], n_col, n_thr), -7, np.int32)
    for g in range(G):
        E, T = eb[g + 1] - eb[g], gb[g + 1] - gb[g]
        e, t = match_group(err[pb[g]:pb[g + 1]].reshape(E, T, n_col), score[eb[g]:eb[g + 1]], thr[g], 0 if max_ests is None else int(max_ests[g]))
        est_gt[eb[g]:eb[g + 1]], gt_est[gb[g]:gb[g + 1]] = e, t
    return est_gt, gt_est


# ---------------------------------------------------------------------------------------------------------------------
# shared cases
# ---------------------------------------------------------------------------------------------------------------------
def visib_image_case(H, W, Q=3, seed=11, bad_row=None):
    """Synthetic depth images for the comparison alone: Q rows over 2 frames of H x W.  The object image is a smooth surface inside
    a disc that differs per row (so the boxes differ and lie away from the frame's borders) with holes and values that are not
    depths; the test depth follows it with noise (inside and outside the support band of delta), has holes, an occluder band far in
    front, a patch far behind, and values that are not measurements.  bad_row: that row's frame id is out of range."""
    rng = np.random.RandomState(seed)
    r, c = np.mgrid[0:H, 0:W].astype(np.float32)
    K = np.stack([np.array([[0.9 * W, 0.0, 0.48 * W], [0.0, 0.95 * W, 0.51 * H], [0.0, 0.0, 1.0]]),
                  np.array([[1.3 * W, 0.0, 0.52 * W], [0.0, 1.2 * W, 0.47 * H], [0.0, 0.0, 1.0]])])
    frame_of = (np.arange(Q) % 2).astype(np.int32)
    obj = np.zeros((Q, H, W), np.float32)
    for q in range(Q):
        cy, cx, rad = H * (0.45 + 0.1 * q), W * (0.55 - 0.07 * q), min(H, W) * (0.42 - 0.05 * q)
        inside = (r - cy) ** 2 + (c - cx) ** 2 < rad ** 2
        obj[q] = np.where(inside, 0.7 + 0.1 * q + 0.05 * np.sin(r / (3.0 + q)) * np.cos(c / (5.0 + q)), 0)
    obj[rng.rand(Q, H, W) < 0.1] = 0
    test = np.zeros((2, H, W), np.float32)
    for b in range(2):
        test[b] = 0.7 + 0.1 * b + 0.05 * np.sin(r / (3.0 + b)) * np.cos(c / (5.0 + b)) + 0.012 * rng.randn(H, W)
    test[rng.rand(2, H, W) < 0.2] = 0
    test[:, H // 2:H // 2 + max(1, H // 10)] = 0.3                                # an occluder band
    test[:, :, W // 3:W // 3 + max(1, W // 12)] = 2.0                             # far behind: visible, not supported
    test[0, 0, 0], test[1, H - 1, W - 1], test[0, H - 1, 0] = np.nan, np.inf, -1.0
    obj[0, H // 2 + 1, W // 2], obj[0, H // 2 + 1, W // 2 + 1], obj[0, H // 2 + 1, W // 2 + 2] = np.nan, np.inf, -1.0
    if bad_row is not None:
        frame_of[bad_row] = 2
    return dict(K=K, frame_of=frame_of, depth_test=test, depth_obj=obj, B=2, H=H, W=W, delta=0.015)


def group_tables(sizes):
    """sizes: list of (E_g, T_g) -> est_begin, gt_begin i32, pair_begin i64"""
    E, T = np.array([s[0] for s in sizes], np.int64), np.array([s[1] for s in sizes], np.int64)
    return dict(est_begin=np.concatenate([[0], np.cumsum(E)]).astype(np.int32), gt_begin=np.concatenate([[0], np.cumsum(T)]).astype(np.int32),
                pair_begin=np.concatenate([[0], np.cumsum(E * T)]).astype(np.int64))


GROUP_SIZES = ((1, 1), (0, 3), (2, 2), (7, 2), (3, 0), (64, 64), (2, 7), (0, 0), (7, 7), (1, 64), (64, 1), (1, 1))


def match_case(n_col, n_thr, sizes=GROUP_SIZES, seed=4, with_max=True):
    """Seeded random errors with planted ties (errors drawn from 12 values, so most rows hold equal errors), NaN and infinite errors,
    errors equal to a threshold; scores drawn from 5 values with NaNs; thresholds that differ per group; max_ests of 0, 1 and more."""
    rng = np.random.RandomState(seed)
    tb = group_tables(sizes)
    G, Etot, Npairs = len(sizes), int(tb["est_begin"][-1]), int(tb["pair_begin"][-1])
    values = np.round(rng.rand(12), 2)
    err = values[rng.randint(0, 12, (Npairs, n_col))]
    err[rng.rand(Npairs, n_col) < 0.05] = np.nan
    err[rng.rand(Npairs, n_col) < 0.03] = np.inf
    score = np.array([0.1, 0.5, 0.5, 0.9, -1.0], np.float32)[rng.randint(0, 5, Etot)]
    score[rng.rand(Etot) < 0.1] = np.nan
    thr = np.sort(values[rng.randint(0, 12, (G, n_thr))] + (rng.rand(G, n_thr) < 0.5) * 0.3, axis=1)      # half of them ARE error values
    out = dict(tables=tb, err=np.ascontiguousarray(err), score=score, thr=np.ascontiguousarray(thr), n_col=n_col, n_thr=n_thr,
               max_ests=np.array([(0, 1, 3, 70)[g % 4] for g in range(G)], np.int32) if with_max else None)
    return out
