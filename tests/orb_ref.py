"""Numpy restatement of include/ffb6d_orb.h: the integer ORB detector (gray, 1.2x pyramid, FAST-9 score, strict 8-neighbour
maxima, Harris response, quota per level), the lift of its pixels through a depth image into the object frame, and the
compaction into point sets.  What csrc/orb.hip is held against, bit for bit.  Test infrastructure only.

  gray / level_sizes / resize / pyramid      the images;
  fast_scores / candidates / harris(_map)    per level;
  quotas                                     the per-level quota, in double as ORB does;
  detect(rgb, ...)                           count i32 [F], kps i32 [F,Q,5], resp i64 [F,Q];
  lift(...) / compact(...)                   slot_pts, slot_ok  ->  pts, begin, n_found.
"""
import numpy as np

f32 = np.float32

CIRCLE = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1),
          (-2, -2), (-1, -3))


def gray(rgb):
    """rgb u8 [3,H,W] -> u8 [H,W]"""
    r, g, b = (rgb[c].astype(np.int64) for c in range(3))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def level_size(n, l):
    return (2 * n * 5 ** l + 6 ** l) // (2 * 6 ** l)


def level_sizes(H, W, L):
    return [(level_size(H, l), level_size(W, l)) for l in range(L)]


def _taps(n_src, n_dst):
    x = np.arange(n_dst, dtype=np.int64)
    num, den = (2 * x + 1) * n_src - n_dst, 2 * n_dst
    x0 = num // den
    return x0, np.minimum(x0 + 1, n_src - 1), ((num - x0 * den) * 2048) // den


def resize(img, Hd, Wd):
    """u8 [Hs,Ws] -> u8 [Hd,Wd]"""
    Hs, Ws = img.shape
    p = img.astype(np.int64)
    x0, x1, fx = _taps(Ws, Wd)
    y0, y1, fy = _taps(Hs, Hd)
    fy = fy[:, None]
    top = (2048 - fx) * p[y0][:, x0] + fx * p[y0][:, x1]
    bot = (2048 - fx) * p[y1][:, x0] + fx * p[y1][:, x1]
    return (((2048 - fy) * top + fy * bot + (1 << 21)) >> 22).astype(np.uint8)


def pyramid(g0, L):
    out = [g0]
    for l in range(1, L):
        out.append(resize(out[-1], level_size(g0.shape[0], l), level_size(g0.shape[1], l)))
    return out


def fast_scores(g):
    """the FAST-9 score of every pixel whose circle lies in the image; 0 on the border of 3"""
    H, W = g.shape
    out = np.zeros((H, W), np.int64)
    if H < 7 or W < 7:
        return out
    p = g.astype(np.int64)
    d = np.stack([p[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] - p[3:H - 3, 3:W - 3] for dx, dy in CIRCLE])
    best = np.zeros(d.shape[1:], np.int64)
    for k in range(16):
        arc = d[[(k + j) % 16 for j in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(0), (-arc).min(0)))
    out[3:H - 3, 3:W - 3] = best
    return out


def candidates(g, t, edge):
    """(x, y) of the strict 8-neighbour maxima above t inside the border, in pixel-index order"""
    H, W = g.shape
    if H < 2 * edge + 1 or W < 2 * edge + 1:
        return np.zeros((0, 2), np.int64)
    s = fast_scores(g)
    c = s[edge:H - edge, edge:W - edge]
    ok = c > t
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                ok &= c > s[edge + dy:H - edge + dy, edge + dx:W - edge + dx]
    y, x = np.nonzero(ok)
    return np.stack([x + edge, y + edge], 1).astype(np.int64)


def harris(g, x, y):
    p = g.astype(np.int64)[y - 4:y + 5, x - 4:x + 5]
    ix = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    iy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    a, b, c = int((ix * ix).sum()), int((iy * iy).sum()), int((ix * iy).sum())
    return 25 * (a * b - c * c) - (a + b) ** 2


def harris_map(g):
    """harris() at every pixel at least 4 inside the image (0 elsewhere), in int64: the 7x7 sums through summed-area tables"""
    H, W = g.shape
    p = g.astype(np.int64)
    ix = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])          # [H-2, W-2]
    iy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])

    def box7(v):
        c = np.zeros((v.shape[0] + 1, v.shape[1] + 1), np.int64)
        c[1:, 1:] = v.cumsum(0).cumsum(1)
        return c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]                                               # [H-8, W-8]

    a, b, c = box7(ix * ix), box7(iy * iy), box7(ix * iy)
    out = np.zeros((H, W), np.int64)
    out[4:H - 4, 4:W - 4] = 25 * (a * b - c * c) - (a + b) ** 2
    return out


def quotas(n_features=500, n_levels=8):
    f = 1.0 / 1.2
    n = n_features * (1.0 - f) / (1.0 - f ** n_levels)
    out, total = [], 0
    for _ in range(n_levels - 1):
        out.append(int(round(n)))                         # Python rounds half to even
        total += out[-1]
        n *= f
    out.append(max(n_features - total, 0))
    return np.asarray(out, np.int32)


def detect_level(g, t, edge, quota):
    """the kept candidates of one level by rank: xy i64 [n,2], resp (Python ints)"""
    xy = candidates(g, t, edge)
    resp = [int(v) for v in harris_map(g)[xy[:, 1], xy[:, 0]]] if len(xy) else []
    order = sorted(range(len(xy)), key=lambda i: (-resp[i], int(xy[i][1]) * g.shape[1] + int(xy[i][0])))[:int(quota)]
    return xy[order], [resp[i] for i in order], len(xy)


def detect(rgb, n_levels=8, t=20, edge=31, quota=None, want_counts=False):
    """rgb u8 [F,3,H,W] -> count i32 [F], kps i32 [F,Q,5], resp i64 [F,Q] (, candidates per (frame, level))"""
    rgb = np.asarray(rgb)
    F, _, H, W = rgb.shape
    quota = quotas(500, n_levels) if quota is None else np.asarray(quota, np.int32)
    Q = int(quota.sum())
    count, kps, resp = np.zeros(F, np.int32), np.full((F, Q, 5), -1, np.int32), np.zeros((F, Q), np.int64)
    n_cand = np.zeros((F, n_levels), np.int64)
    for f in range(F):
        row = 0
        for l, g in enumerate(pyramid(gray(rgb[f]), n_levels)):
            xy, r, n_cand[f, l] = detect_level(g, t, edge, quota[l])
            for (x, y), v in zip(xy, r):
                kps[f, row] = (x, y, l, ((2 * x + 1) * W) // (2 * g.shape[1]), ((2 * y + 1) * H) // (2 * g.shape[0]))
                resp[f, row] = v
                row += 1
        count[f] = row
    return (count, kps, resp, n_cand) if want_counts else (count, kps, resp)


def lift(kps, count, depth, visible, T, K, min_pixels=500):
    """kps i32 [F,Q,5], count [F], depth f32 [F,H,W], visible [F], T f64 [F,3,4], K [3,3] -> slot_pts f32 [F,Q,3], slot_ok i32 [F,Q]"""
    F, Q = kps.shape[:2]
    H, W = depth.shape[1:]
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = f32(K[0, 0]), f32(K[1, 1]), f32(K[0, 2]), f32(K[1, 2])
    pts, ok = np.zeros((F, Q, 3), f32), np.zeros((F, Q), np.int32)
    T = np.asarray(T, np.float64).reshape(F, 3, 4)
    for f in range(F):
        if visible[f] < min_pixels:
            continue
        for r in range(int(count[f])):
            X, Y = int(kps[f, r, 3]), int(kps[f, r, 4])
            if not (0 <= X < W and 0 <= Y < H):
                continue
            z = f32(depth[f, Y, X])
            if not (np.isfinite(z) and z > f32(1e-8)):
                continue
            with np.errstate(over="ignore"):
                px = f32(f32(f32(f32(X) - cx) * z) / fx)
                py = f32(f32(f32(f32(Y) - cy) * z) / fy)
            d = np.array([px, py, z], np.float64) - T[f, :, 3]
            R = T[f, :, :3]
            with np.errstate(over="ignore"):
                pts[f, r] = [f32((d[0] * R[0, j] + d[1] * R[1, j]) + d[2] * R[2, j]) for j in range(3)]
            ok[f, r] = 1
    return pts, ok


def compact(slot_pts, slot_ok, S, V):
    """-> pts f32 [S*V*Q,3] (zeros past the last point), begin i64 [S+1], n_found i32 [S]"""
    F, Q = slot_ok.shape
    assert F == S * V
    flat_ok = slot_ok.reshape(S, V * Q) != 0
    n_found = flat_ok.sum(1).astype(np.int32)
    begin = np.concatenate([[0], np.cumsum(n_found)]).astype(np.int64)
    pts = np.zeros((F * Q, 3), f32)
    pts[:begin[-1]] = slot_pts.reshape(F * Q, 3)[flat_ok.reshape(-1)]
    return pts, begin, n_found


def point_sets(pts, begin):
    return [pts[begin[s]:begin[s + 1]] for s in range(len(begin) - 1)]


# ---- the images the tests share -----------------------------------------------------------------------------------------
DOTS = ((10, 10, 200), (30, 12, 120), (50, 14, 250), (20, 30, 60), (40, 34, 51), (54, 38, 50), (12, 40, 200))


def as_rgb(g):
    """a gray image as the rgb frame whose gray it is (4899 + 9617 + 1868 = 2^14)"""
    return np.repeat(np.asarray(g, np.uint8)[None], 3, 0)


def dots_image():
    g = np.full((48, 64), 30, np.uint8)
    for x, y, v in DOTS:
        g[y, x] = v
    return g


def lattice_dots_image(n=400, step=8, value=180):
    """(n // step - 1)^2 identical isolated dots: one response shared by thousands of candidates, ranked by pixel index alone"""
    g = np.full((n, n), 30, np.uint8)
    g[5:n - 5:step, 5:n - 5:step] = value
    return g


def noise_rgb(H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, (3, H, W)).astype(np.uint8)


def frames(H, W):
    """three frames of different content: the dots (cropped or padded to the size), and two noise images"""
    g = np.full((H, W), 30, np.uint8)
    d = dots_image()
    g[:min(H, 48), :min(W, 64)] = d[:H, :W]
    out = np.stack([as_rgb(g), noise_rgb(H, W, 11), noise_rgb(H, W, 12)])
    out.setflags(write=False)
    return out


# (H, W), levels, quota: threshold 20 and edge 4 throughout
CASES = [((48, 64), 1, (16,)), ((48, 64), 1, (400,)), ((48, 64), 3, (300, 150, 80)), ((48, 64), 3, (16, 8, 4)),
         ((37, 53), 1, (12,)), ((37, 53), 3, (200, 7, 40))]


def lift_case(seed=5, F=4, Q=12, H=24, W=32):
    """keypoint rows with level-0 pixels all over the frame, depth with zeros, a NaN and an infinity under some of them; frame 2 is
    below min_pixels, frame 3 has count 0"""
    rs = np.random.RandomState(seed)
    kps = np.full((F, Q, 5), -1, np.int32)
    count = np.array([Q, 7, Q, 0], np.int32)
    for f in range(F):
        n = count[f]
        kps[f, :n, 3], kps[f, :n, 4] = rs.randint(0, W, n), rs.randint(0, H, n)
        kps[f, :n, :3] = 0
    depth = rs.uniform(0.3, 0.9, (F, H, W)).astype(np.float32)
    depth[0, kps[0, 1, 4], kps[0, 1, 3]] = 0
    depth[0, kps[0, 4, 4], kps[0, 4, 3]] = np.nan
    depth[1, kps[1, 0, 4], kps[1, 0, 3]] = np.inf
    depth[1, kps[1, 6, 4], kps[1, 6, 3]] = -0.5
    visible = np.array([60, 50, 49, 500], np.int32)
    T = np.zeros((F, 3, 4))
    for f in range(F):
        q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
        T[f, :, :3], T[f, :, 3] = q * np.sign(np.linalg.det(q)), rs.uniform(-0.2, 0.6, 3)
    K = np.array([[35.5, 0, 16.25], [0, 36, 12.5], [0, 0, 1]])
    return kps, count, depth, visible, T, K
