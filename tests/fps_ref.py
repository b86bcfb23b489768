"""Numpy restatement of the reference's farthest-point sampling and of its box statistics: what csrc/fps.hip is held against,
bit for bit (include/ffb6d_fps.h states the same rule).  Test infrastructure only.

  fps(pts, m, start)       farthest_point_sampling.cpp:41-160, both entry points, followed literally -- mask and all;
  box(pts)                 dataset_tools/utils.py:89-115 (get_3D_bbox, get_centers_3d, get_r) in float32, as the kernel computes;
  box64(pts)               the same formulas in float64.
  fps_batch / cases        several sets in the packed layout of the C ABI, and the small sets the tests share.
"""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
f32 = np.float32


def dist2(p, c):
    """(input_pts[i] - c).squared_norm(), :18,25: x*x + y*y + z*z left to right, each operation rounded to float32"""
    with np.errstate(over="ignore"):
        d = (p - c).astype(f32)
        return ((d[..., 0] * d[..., 0]).astype(f32) + (d[..., 1] * d[..., 1]).astype(f32)).astype(f32) + (d[..., 2] * d[..., 2]).astype(f32)


def _find_max(min_dist, mask):
    """find_max_dist_idx, :56-73: max_idx = 0, max_d = 0.f; the first unmasked i with the largest min_dist > max_d"""
    cand = np.where(mask, f32(0), min_dist)
    i = int(np.argmax(cand))                              # the first of the largest
    return (i, cand[i]) if cand[i] > 0 else (0, f32(0))


def fps(pts, m, start=None):
    """pts f32 [n,3], n >= 1 -> idx i32 [m], out_pts f32 [m,3], out_dist f32 [m].
    start: int = sample_farthest_points (:77-105) with its `rand() % n` given; None = sample_farthest_points_init_center (:122-160)."""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    n = len(pts)
    mask = np.zeros(n, bool)
    min_dist = np.full(n, FLT_MAX, f32)
    idx, dist = np.zeros(m, np.int32), np.zeros(m, f32)
    if start is None:
        center = ((pts.max(0) + pts.min(0)).astype(f32) * f32(0.5)).astype(f32)         # (max + min) / 2.f = * (1.f / 2.f), :20,138
        min_dist = np.minimum(dist2(pts, center), min_dist)                              # :140-141
        cur, d = _find_max(min_dist, mask)
    else:
        cur, d = min(max(int(start), 0), n - 1), FLT_MAX
    for k in range(m):
        mask[cur] = True
        idx[k], dist[k] = cur, d
        if k < m - 1:
            upd = np.minimum(min_dist, dist2(pts, pts[cur]))                             # update_min_dist, :41-54
            min_dist = np.where(mask, min_dist, upd)
            cur, d = _find_max(min_dist, mask)
    return idx, pts[idx], dist


def box(pts):
    """corners f32 [8,3], ctr f32 [3], radius f32 of one set; zeros for an empty one"""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    if len(pts) == 0:
        return np.zeros((8, 3), f32), np.zeros(3, f32), f32(0)
    lo, hi = pts.min(0), pts.max(0)
    corners = np.array([[(hi if k & 4 else lo)[0], (hi if k & 2 else lo)[1], (hi if k & 1 else lo)[2]] for k in range(8)], f32)
    ctr = ((hi + lo).astype(f32) * f32(0.5)).astype(f32)
    with np.errstate(over="ignore"):
        d = (hi - lo).astype(f32)
        r = f32(0.5) * np.sqrt(((d[0] * d[0]).astype(f32) + (d[1] * d[1]).astype(f32)).astype(f32) + (d[2] * d[2]).astype(f32), dtype=f32)
    return corners, ctr, f32(r)


def box64(pts):
    """the reference's own lines in float64: get_3D_bbox :89-102, get_centers_3d :113-115, get_r :109-110"""
    pcld = np.asarray(pts, np.float64).reshape(-1, 3)
    if len(pcld) == 0:
        return np.zeros((8, 3)), np.zeros(3), 0.0
    min_x, max_x = pcld[:, 0].min(), pcld[:, 0].max()
    min_y, max_y = pcld[:, 1].min(), pcld[:, 1].max()
    min_z, max_z = pcld[:, 2].min(), pcld[:, 2].max()
    bbox = np.array([[min_x, min_y, min_z], [min_x, min_y, max_z], [min_x, max_y, min_z], [min_x, max_y, max_z],
                     [max_x, min_y, min_z], [max_x, min_y, max_z], [max_x, max_y, min_z], [max_x, max_y, max_z]])
    return bbox, (np.max(bbox, 0) + np.min(bbox, 0)) / 2, np.linalg.norm(bbox[7, :] - bbox[0, :]) / 2.0


def pack(sets):
    """list of [n_s,3] -> pts f32 [total + 1, 3] (a spare row, so that an empty batch still has an address), begin i64 [S+1]"""
    sets = [np.ascontiguousarray(s, f32).reshape(-1, 3) for s in sets]
    begin = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return np.concatenate(sets + [np.zeros((1, 3), f32)]), begin


def fps_batch(sets, m, start=None):
    """start: None or one int per set -> idx i32 [S,m], pts f32 [S,m,3], dist f32 [S,m]; an empty set gives -1 / 0 / 0"""
    S = len(sets)
    idx, out, dist = np.full((S, m), -1, np.int32), np.zeros((S, m, 3), f32), np.zeros((S, m), f32)
    for s, p in enumerate(sets):
        if len(p):
            idx[s], out[s], dist[s] = fps(p, m, None if start is None else start[s])
    return idx, out, dist


# ---- the point sets the tests share ---------------------------------------------------------------------------------
def random_set(n, seed):
    return np.random.RandomState(seed).uniform(-0.15, 0.15, (n, 3)).astype(f32)


def lattice_set(n, seed):
    """points on a 0.05 lattice: many equal distances, and -- above 6^3 = 216 points -- exact duplicates too"""
    return (np.random.RandomState(seed).randint(-3, 3, (n, 3)) * 0.05).astype(f32)


def duplicate_set(n, seed):
    """the second half repeats the first"""
    a = random_set((n + 1) // 2, seed)
    return np.concatenate([a, a])[:n].copy()


def identical_set(n, seed):
    return np.repeat(random_set(1, seed), n, axis=0)


KINDS = {"random": random_set, "lattice": lattice_set, "duplicate": duplicate_set, "identical": identical_set}
