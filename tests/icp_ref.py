"""numpy restatement of the ICP refinement stated in include/ffb6d_refine.h (the reference repository has no ICP code, so
there is nothing to port: this file is what ffb6d_amd/refine.py and csrc/icp.hip are held against).

Steps 1-3 (scene point -> model frame, nearest model point, gate) are written operation by operation on arrays of ONE dtype:
with np.float32 every product and sum is rounded on its own, which is the device's arithmetic (numpy never fuses a multiply
with an add); with np.float64 the same steps give the comparison that decides whether a case has a genuine rounding tie
(`first_divergence`).  Step 4, the fit, is float64 from the float32 points in both."""
import numpy as np


def scene_indices(mask, frame, cls, keep=None):
    """cloud indices of the scene points of problem (frame, cls), in index order; none for a frame that is no index"""
    if frame < 0 or frame >= mask.shape[0]:
        return np.zeros(0, np.int64)
    sel = mask[frame] == cls
    if keep is not None:
        sel = sel & (keep[frame] != 0)
    return np.flatnonzero(sel)


def to_model_frame(s, T, dtype=np.float32):
    """q = R^T (s - t): d = s - t, q_j = ((d0*R0j + d1*R1j) + d2*R2j), R and t rounded once to `dtype`"""
    Rt = np.asarray(T, np.float64).astype(dtype)
    s = np.asarray(s, np.float32).astype(dtype)
    d0, d1, d2 = s[:, 0] - Rt[0, 3], s[:, 1] - Rt[1, 3], s[:, 2] - Rt[2, 3]
    return np.stack([(d0 * Rt[0, j] + d1 * Rt[1, j]) + d2 * Rt[2, j] for j in range(3)], axis=1)


def nearest(q, model, dtype=np.float32, chunk=512):
    """-> (index i64 [n], d2 dtype [n]) of the nearest model point: ((dx*dx + dy*dy) + dz*dz), lowest index on ties
    (np.argmin returns the first minimum; the first NaN when there is one).  No model points: index -1, d2 = inf."""
    n = len(q)
    if len(model) == 0:
        return np.full(n, -1, np.int64), np.full(n, np.inf, dtype)
    m = np.asarray(model, np.float32).astype(dtype)
    idx, d2 = np.zeros(n, np.int64), np.zeros(n, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, n, chunk):
            qq = q[a:a + chunk]
            dx, dy, dz = (qq[:, None, k] - m[None, :, k] for k in range(3))
            dd = (dx * dx + dy * dy) + dz * dz
            j = np.argmin(dd, axis=1)
            idx[a:a + chunk], d2[a:a + chunk] = j, dd[np.arange(len(qq)), j]
    return idx, d2


def correspond(scene, model, T, max_dist, dtype=np.float32):
    """steps 1-3 -> dict: nearest i64 [n] (before the gate), kept bool [n], idx i32 [n] (-1 where not kept), d2 dtype [n]"""
    scene = np.asarray(scene, np.float32).reshape(-1, 3)
    near, d2 = nearest(to_model_frame(scene, T, dtype), model, dtype)
    lim = dtype(max_dist) * dtype(max_dist)
    with np.errstate(invalid="ignore"):
        kept = (near >= 0) & (d2 <= lim)                       # a NaN distance is never kept
    return dict(nearest=near, kept=kept, idx=np.where(kept, near, -1).astype(np.int32), d2=d2)


def best_fit(A, B):
    """reflection-corrected least-squares [R|t] with R A_i + t ~ B_i, float64 from the float32 points
    (the reference's best_fit_transform, ffb6d/utils/pvn3d_eval_utils_kpls.py:28-61, restated)"""
    A, B = np.asarray(A, np.float32).astype(np.float64), np.asarray(B, np.float32).astype(np.float64)
    ca, cb = A.mean(axis=0), B.mean(axis=0)
    H = (A - ca).T @ (B - cb)
    U, _, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        Vt[2, :] *= -1
        R = Vt.T @ U.T
    T = np.zeros((3, 4))
    T[:, :3], T[:, 3] = R, cb - R @ ca
    return T


def box_move(model, Ta, Tb):
    """largest displacement of a corner of the model's bounding box between two poses"""
    m = np.asarray(model, np.float32).astype(np.float64)
    lo, hi = m.min(axis=0), m.max(axis=0)
    c = np.array([[(hi if k >> a & 1 else lo)[a] for a in range(3)] for k in range(8)])
    return float(np.linalg.norm((c @ Ta[:, :3].T + Ta[:, 3]) - (c @ Tb[:, :3].T + Tb[:, 3]), axis=1).max())


def icp(scene, model, T0, max_iter, max_dist, tol=0.0, min_pairs=3, dtype=np.float32):
    """The loop for one problem -> dict: T f64 [3,4], n_pairs, rms (f32), iters, history (the `nearest` array and the kept
    mask of every iteration made).  Fewer than min_pairs kept pairs: the pose stays and the problem is over."""
    scene = np.asarray(scene, np.float32).reshape(-1, 3)
    model = np.asarray(model, np.float32).reshape(-1, 3)
    T = np.array(T0, np.float64)
    n_pairs, rms, iters, history = 0, np.float32(0), 0, []
    for _ in range(max_iter):
        c = correspond(scene, model, T, max_dist, dtype)
        k = c["kept"]
        history.append((c["nearest"], k))
        n_pairs = int(k.sum())
        rms = np.float32(np.sqrt(c["d2"][k].astype(np.float64).sum() / n_pairs)) if n_pairs else np.float32(0)
        if n_pairs < min_pairs:
            break
        Tn = best_fit(model[c["nearest"][k]], scene[k])
        moved = box_move(model, Tn, T) if tol > 0 else None
        T, iters = Tn, iters + 1
        if tol > 0 and moved <= tol:
            break
    return dict(T=T, n_pairs=n_pairs, rms=rms, iters=iters, history=history)


def first_divergence(scene, model, T0, max_iter, max_dist, tol=0.0, min_pairs=3):
    """Iteration in which the float32 and the float64 restatement pick a different correspondence or keep a different set
    (a genuine rounding tie), or None.  Decided by the restatement alone."""
    a = icp(scene, model, T0, max_iter, max_dist, tol, min_pairs, np.float32)["history"]
    b = icp(scene, model, T0, max_iter, max_dist, tol, min_pairs, np.float64)["history"]
    for it, ((na, ka), (nb, kb)) in enumerate(zip(a, b)):
        if not (np.array_equal(ka, kb) and np.array_equal(na[ka], nb[kb])):
            return it
    return None if len(a) == len(b) else min(len(a), len(b))


def models_of(points):
    """list indexed by class id of f32 [n_c,3] arrays (None = no points), as evaluate.ModelPoints takes them"""
    return [np.zeros((0, 3), np.float32) if p is None else np.asarray(p, np.float32).reshape(-1, 3) for p in points]


def problem_scene(pcld, mask, frame, cls, keep=None):
    i = scene_indices(mask, frame, cls, keep)
    return pcld[frame][i] if len(i) else np.zeros((0, 3), np.float32)


def problem_model(models, cls):
    return models[cls] if 0 <= cls < len(models) else np.zeros((0, 3), np.float32)


def correspondences(pcld, mask, T, frame_of, class_of, models, max_dist, keep=None, dtype=np.float32):
    """every problem of a call -> idx i32 [P,N] (-1 beyond the count), d2 f32 [P,N] (+inf beyond the count), counts i32 [P]"""
    P, N = len(frame_of), pcld.shape[1]
    idx, d2 = np.full((P, N), -1, np.int32), np.full((P, N), np.inf, dtype)
    counts = np.zeros(P, np.int32)
    for p in range(P):
        s = problem_scene(pcld, mask, int(frame_of[p]), int(class_of[p]), keep)
        c = correspond(s, problem_model(models, int(class_of[p])), T[p], max_dist, dtype)
        counts[p] = len(s)
        idx[p, :len(s)], d2[p, :len(s)] = c["idx"], c["d2"]
    return idx, d2, counts


def icp_refine(pcld, mask, T0, frame_of, class_of, models, max_iter, max_dist, tol=0.0, min_pairs=3, keep=None, dtype=np.float32):
    """every problem of a call -> (T f64 [P,3,4], dict n_pairs i32 [P], rms f32 [P], iters i32 [P])"""
    out = [icp(problem_scene(pcld, mask, int(frame_of[p]), int(class_of[p]), keep), problem_model(models, int(class_of[p])),
               T0[p], max_iter, max_dist, tol, min_pairs, dtype) for p in range(len(frame_of))]
    return (np.stack([o["T"] for o in out]) if out else np.zeros((0, 3, 4)),
            dict(n_pairs=np.array([o["n_pairs"] for o in out], np.int32), rms=np.array([o["rms"] for o in out], np.float32),
                 iters=np.array([o["iters"] for o in out], np.int32)))


# ---- synthetic cases ---------------------------------------------------------------------------------------------------
def surface_model(seed, n_pts=4096):
    """A surface-like model cloud f32 [n_pts,3]: points on an ellipsoid of semi-axes 0.06 / 0.04 / 0.03 m with 10-15 % sinusoidal
    bumps (a Gaussian blob has no surface for ICP to slide along and stalls in local minima)."""
    rng = np.random.RandomState(seed)
    u = rng.randn(n_pts, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    theta, phi = np.arctan2(u[:, 1], u[:, 0]), np.arccos(np.clip(u[:, 2], -1, 1))
    amp, k1, k2 = 0.10 + 0.05 * rng.rand(), rng.randint(3, 6), rng.randint(2, 5)
    bump = 1.0 + amp * np.sin(k1 * theta + 6.28 * rng.rand()) * np.sin(k2 * phi + 6.28 * rng.rand())
    return (u * [0.06, 0.04, 0.03] * bump[:, None]).astype(np.float32)


def partial_view(model, gt, seed, noise=0.001, clutter=0.1):
    """The camera-facing part of `model` under the pose gt [3,4] (camera at the origin) + Gaussian noise (metres) + a fraction of
    clutter points around the object -> f32 [n,3]."""
    rng = np.random.RandomState(seed)
    gt = np.asarray(gt, np.float64)
    m = np.asarray(model, np.float64)
    p = m @ gt[:, :3].T + gt[:, 3]
    normal = (m - m.mean(axis=0)) @ gt[:, :3].T
    vis = p[np.einsum("ij,ij->i", normal, p) < 0]
    vis = vis + noise * rng.randn(*vis.shape)
    junk = gt[:, 3] + 0.1 * (rng.rand(int(clutter * len(vis)), 3) - 0.5)
    out = np.concatenate([vis, junk])
    return out[rng.permutation(len(out))].astype(np.float32)


def add(model, Ta, Tb):
    """ADD: mean distance between the model points under two poses (float64)"""
    m = np.asarray(model, np.float64)
    return float(np.linalg.norm((m @ Ta[:, :3].T + Ta[:, 3]) - (m @ Tb[:, :3].T + Tb[:, 3]), axis=1).mean())
