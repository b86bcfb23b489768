"""numpy restatement of the point-to-plane metric of include/ffb6d_refine.h (the *_plane calls of csrc/icp.hip, the `metric="plane"`
of ffb6d_amd/refine.py): the model normals (given or estimated), the class constants, steps 4p and 5p, the loop for one problem,
for the problems of a class call and for the instance calls.

Steps 1-3 are tests/icp_ref.py's, used from there unchanged, in float32 (the device's arithmetic) or float64 (the comparison that
decides whether a case has a genuine rounding tie, `first_divergence`).  Steps 4p and 5p are float64 from the float32 points and
normals in both.  The eigenvalues come from np.linalg.eigh, not from a Jacobi of this file's own: the kernels' Jacobi is held
against LAPACK."""
import numpy as np

import icp_ref
import icp_inst_ref
from icp_ref import add, correspond, models_of, partial_view, problem_model, problem_scene, surface_model      # noqa: F401

K_NORMAL = 16
SMALL_THETA = 1e-4


# ---- normals -----------------------------------------------------------------------------------------------------------------
def given_normals(normals):
    """f32 [n,3] -> f32 [n,3]: each normalised once in double; a non-finite component or zero length gives the zero vector"""
    v = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        length = np.sqrt((v * v).sum(axis=1))
        ok = np.isfinite(length) & (length > 0)
        out = np.where(ok[:, None], v / np.where(ok, length, 1.0)[:, None], 0.0)
    return out.astype(np.float32)


def neighbours(model, k):
    """i64 [n,k]: the k nearest points of the cloud to each of its points, itself included, ascending in the float32 distance
    ((dx*dx + dy*dy) + dz*dz), equal distances by the lowest index (the exact search of include/ffb6d_knn.h)"""
    m = np.asarray(model, np.float32)
    dx, dy, dz = (m[:, None, a] - m[None, :, a] for a in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = (dx * dx + dy * dy) + dz * dz
    return np.argsort(d2, axis=1, kind="stable")[:, :k]


def oriented(v):
    """the sign that makes the component of largest magnitude positive; the lowest axis wins ties"""
    big = int(np.argmax(np.abs(v)))
    return -v if v[big] < 0 else v


def estimate_normals(model, k=K_NORMAL):
    """-> (normals f32 [n,3], spectrum f64 [n,3]: the eigenvalues of every point's neighbourhood covariance, ascending).
    The zero vector when n < 3 or the second eigenvalue is zero."""
    m = np.asarray(model, np.float32).reshape(-1, 3)
    n = len(m)
    normals, spectrum = np.zeros((n, 3), np.float32), np.zeros((n, 3))
    if n < 3:
        return normals, spectrum
    nb = neighbours(m, min(k, n))
    for j in range(n):
        p = m[nb[j]].astype(np.float64)
        e = p - p.sum(axis=0) / len(p)
        lam, vec = np.linalg.eigh(e.T @ e)
        spectrum[j] = lam
        if lam[1] > 0:
            v = vec[:, 0] / np.linalg.norm(vec[:, 0])
            normals[j] = oriented(v)
    return normals, spectrum


# ---- steps 4p and 5p -----------------------------------------------------------------------------------------------------------
def class_constants(model):
    """(c f64 [3], rho): centre and half diagonal of the class's bounding box, in double from the float32 box"""
    m = np.asarray(model, np.float32).reshape(-1, 3)
    if len(m) == 0:
        return np.zeros(3), 0.0
    with np.errstate(invalid="ignore"):
        lo, hi = np.fmin.reduce(m, axis=0).astype(np.float64), np.fmax.reduce(m, axis=0).astype(np.float64)
    ext = hi - lo
    return 0.5 * (lo + hi), 0.5 * float(np.sqrt(ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2]))


def plane_system(q, m, n, c, rho):
    """step 4p over the kept pairs -> (M f64 [6,6], g f64 [6], sum r*r): q the scene points in the model frame (step 1), m / n
    the model points and normals of the pairs"""
    q, m, n = (np.asarray(x).astype(np.float64).reshape(-1, 3) for x in (q, m, n))
    u = (q - c) / rho
    a = np.concatenate([np.cross(u, n), n], axis=1)
    r = np.einsum("ij,ij->i", n, q - m) / rho
    return a.T @ a, a.T @ r, float((r * r).sum())


def solve_truncated(M, g, min_eig):
    """step 5p -> (x f64 [6], eigenvalues ascending, used bool [6]): x = -sum v (v.g)/l over l > 0 and l >= min_eig * l_max"""
    lam, vec = np.linalg.eigh(M)
    used = (lam > 0) & (lam >= min_eig * lam.max())
    x = np.zeros(6)
    for k in np.flatnonzero(used):
        x -= vec[:, k] * (vec[:, k] @ g) / lam[k]
    return x, lam, used


def rodrigues(w):
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < SMALL_THETA:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        A, B = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + A * K + B * (K @ K)


def updated_pose(T, x, c, rho):
    """R <- R Rd^T, t <- t - R_new d with Rd = exp([x[0:3]]x), d = c - Rd c + rho x[3:6]"""
    Rd = rodrigues(x[:3])
    d = c - Rd @ c + rho * x[3:]
    Tn = np.zeros((3, 4))
    Tn[:, :3] = T[:, :3] @ Rd.T
    Tn[:, 3] = T[:, 3] - Tn[:, :3] @ d
    return Tn


def plane_update(scene, model, normals, T, c, rho, near, kept, min_eig, dtype):
    """steps 4p-5p of one problem from its correspondences -> (Tn or None when x is not finite, rms_plane f32, eigenvalues, used)"""
    q = icp_ref.to_model_frame(scene[kept], T, dtype)
    M, g, rr = plane_system(q, model[near[kept]], normals[near[kept]], c, rho)
    x, lam, used = solve_truncated(M, g, min_eig)
    rms_plane = np.float32(np.sqrt(rho * rho * rr / int(kept.sum())))
    return (updated_pose(T, x, c, rho) if np.isfinite(x).all() else None), rms_plane, lam, used


# ---- the loop --------------------------------------------------------------------------------------------------------------------
def icp_plane(scene, model, normals, T0, max_iter, max_dist, tol=0.0, min_pairs=3, min_eig=1e-6, dtype=np.float32):
    """The loop for one problem -> dict: T f64 [3,4], n_pairs, rms, rms_plane (f32), iters, history (nearest, kept per iteration
    made), eig (eigenvalues and the used mask of every update made)."""
    scene = np.asarray(scene, np.float32).reshape(-1, 3)
    model = np.asarray(model, np.float32).reshape(-1, 3)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    c, rho = class_constants(model)
    T = np.array(T0, np.float64)
    n_pairs, rms, rms_plane, iters, history, eig = 0, np.float32(0), np.float32(0), 0, [], []
    for _ in range(max_iter):
        co = correspond(scene, model, T, max_dist, dtype)
        k = co["kept"]
        history.append((co["nearest"], k))
        n_pairs = int(k.sum())
        rms = np.float32(np.sqrt(co["d2"][k].astype(np.float64).sum() / n_pairs)) if n_pairs else np.float32(0)
        rms_plane = np.float32(0)
        if n_pairs and rho > 0:
            Tn, rms_plane, lam, used = plane_update(scene, model, normals, T, c, rho, co["nearest"], k, min_eig, dtype)
        if n_pairs < min_pairs or not rho > 0 or Tn is None:
            break
        eig.append((lam, used))
        moved = icp_ref.box_move(model, Tn, T) if tol > 0 else None
        T, iters = Tn, iters + 1
        if tol > 0 and moved <= tol:
            break
    return dict(T=T, n_pairs=n_pairs, rms=rms, rms_plane=rms_plane, iters=iters, history=history, eig=eig)


def first_divergence(scene, model, normals, T0, max_iter, max_dist, tol=0.0, min_pairs=3, min_eig=1e-6):
    """Iteration in which the float32 and the float64 restatement pick a different correspondence or keep a different set (a
    genuine rounding tie), or None.  Decided by the restatement alone."""
    a = icp_plane(scene, model, normals, T0, max_iter, max_dist, tol, min_pairs, min_eig, np.float32)["history"]
    b = icp_plane(scene, model, normals, T0, max_iter, max_dist, tol, min_pairs, min_eig, np.float64)["history"]
    for it, ((na, ka), (nb, kb)) in enumerate(zip(a, b)):
        if not (np.array_equal(ka, kb) and np.array_equal(na[ka], nb[kb])):
            return it
    return None if len(a) == len(b) else min(len(a), len(b))


def eig_ratios(eig):
    """every eigenvalue ratio l / l_max of the updates of a run (icp_plane's `eig`), flat"""
    return np.concatenate([lam / lam.max() for lam, _ in eig]) if eig else np.zeros(0)


def problem_normals(normals, cls):
    return normals[cls] if 0 <= cls < len(normals) else np.zeros((0, 3), np.float32)


def icp_refine_plane(pcld, mask, T0, frame_of, class_of, models, normals, max_iter, max_dist, tol=0.0, min_pairs=3, min_eig=1e-6, keep=None,
                     dtype=np.float32):
    """every problem of a class call (normals: a list like models) -> (T f64 [P,3,4], dict n_pairs, rms, rms_plane, iters, eig)"""
    out = [icp_plane(problem_scene(pcld, mask, int(frame_of[p]), int(class_of[p]), keep), problem_model(models, int(class_of[p])),
                     problem_normals(normals, int(class_of[p])), T0[p], max_iter, max_dist, tol, min_pairs, min_eig, dtype)
           for p in range(len(frame_of))]
    return (np.stack([o["T"] for o in out]) if out else np.zeros((0, 3, 4)),
            dict(n_pairs=np.array([o["n_pairs"] for o in out], np.int32), rms=np.array([o["rms"] for o in out], np.float32),
                 rms_plane=np.array([o["rms_plane"] for o in out], np.float32), iters=np.array([o["iters"] for o in out], np.int32),
                 eig=[o["eig"] for o in out]))


# ---- the instance calls: tests/icp_inst_ref.py's sets, groups and owners, this file's update ---------------------------------------
def icp_refine_plane_instances(pcld, mask, inst, T0, frame_of, class_of, inst_of, models, normals, max_iter, max_dist, mode="map", tol=0.0,
                               min_pairs=3, min_eig=1e-6, keep=None, dtype=np.float32):
    """icp_inst_ref.icp_refine_instances with steps 4p-5p -> (T, dict n_pairs, rms, rms_plane, iters, inst, writers, history, eig)"""
    assert mode in ("map", "nearest")
    P = len(frame_of)
    at, scenes = icp_inst_ref._inst_scenes(pcld, mask, inst, frame_of, class_of, inst_of, mode, keep)
    mods = [np.asarray(problem_model(models, int(class_of[p])), np.float32).reshape(-1, 3) for p in range(P)]
    nrm = [np.asarray(problem_normals(normals, int(class_of[p])), np.float32).reshape(-1, 3) for p in range(P)]
    consts = [class_constants(m) for m in mods]
    grp = icp_inst_ref.groups(frame_of, class_of, mode)
    T = np.array(T0, np.float64).reshape(P, 3, 4).copy()
    done, last = np.zeros(P, bool), [np.zeros(len(s), bool) for s in scenes]
    n_pairs, rms, iters = np.zeros(P, np.int32), np.zeros(P, np.float32), np.zeros(P, np.int32)
    rms_plane = np.zeros(P, np.float32)
    history, eig = [[] for _ in range(P)], [[] for _ in range(P)]
    for _ in range(max_iter):
        co = [correspond(scenes[p], mods[p], T[p], max_dist, dtype) if (mode == "nearest" or not done[p]) else None for p in range(P)]
        Tin = T.copy()
        for p in range(P):
            if co[p] is None:
                continue
            k, _ = icp_inst_ref._claim(co, grp, p)
            last[p] = k
            if done[p]:
                continue
            history[p].append((co[p]["nearest"], k))
            n_pairs[p] = int(k.sum())
            rms[p] = np.float32(np.sqrt(co[p]["d2"][k].astype(np.float64).sum() / n_pairs[p])) if n_pairs[p] else np.float32(0)
            c, rho = consts[p]
            rms_plane[p], Tn = np.float32(0), None
            if n_pairs[p] and rho > 0:
                Tn, rms_plane[p], lam, used = plane_update(scenes[p], mods[p], nrm[p], Tin[p], c, rho, co[p]["nearest"], k, min_eig, dtype)
            if n_pairs[p] < min_pairs or not rho > 0 or Tn is None:
                done[p] = True
                continue
            eig[p].append((lam, used))
            if tol > 0 and icp_ref.box_move(mods[p], Tn, Tin[p]) <= tol:
                done[p] = True
            T[p], iters[p] = Tn, iters[p] + 1
    out, writers = np.zeros(mask.shape, np.uint8), np.zeros(mask.shape, np.int32)
    for p in range(P):
        if len(at[p]):
            out[frame_of[p], at[p][last[p]]] = int(inst_of[p]) & 255
            writers[frame_of[p], at[p][last[p]]] += 1
    return T, dict(n_pairs=n_pairs, rms=rms, rms_plane=rms_plane, iters=iters, inst=out, writers=writers, history=history, eig=eig)


def first_divergence_instances(pcld, mask, inst, T0, frame_of, class_of, inst_of, models, normals, max_iter, max_dist, mode="map", tol=0.0,
                               min_pairs=3, min_eig=1e-6, keep=None):
    """Per problem: the first iteration in which the float32 and float64 restatements differ in a correspondence or a kept set, in
    the problem itself or (nearest) in any member of its group, or None."""
    run = lambda dt: icp_refine_plane_instances(pcld, mask, inst, T0, frame_of, class_of, inst_of, models, normals, max_iter, max_dist,      # noqa: E731
                                                mode, tol, min_pairs, min_eig, keep, dt)[1]["history"]
    a, b = run(np.float32), run(np.float64)
    own = []
    for ha, hb in zip(a, b):
        it = None if len(ha) == len(hb) else min(len(ha), len(hb))
        for i, ((na, ka), (nb, kb)) in enumerate(zip(ha, hb)):
            if not (np.array_equal(ka, kb) and np.array_equal(na[ka], nb[kb])):
                it = i
                break
        own.append(it)
    out = []
    for lo, hi in icp_inst_ref.groups(frame_of, class_of, mode):
        its = [i for i in own[lo:hi] if i is not None]
        out.append(min(its) if its else None)
    return out


def in_plane_motion(T0, T1, c):
    """For a model in the plane z = const: where the camera point that sat at the box centre c under T0 lies in the model frame
    under T1, minus c, x and y only.  An update moves it by rho v, along the normal alone, when the in-plane directions are
    truncated; what is left is the in-plane motion of the pose."""
    p0 = T0[:, :3] @ c + T0[:, 3]
    return (T1[:, :3].T @ (p0 - T1[:, 3]) - c)[:2]


# ---- synthetic cases -------------------------------------------------------------------------------------------------------------
def model_with_normals(seed, n_pts):
    """icp_ref.surface_model(seed, n_pts) and its estimated normals as the library prepares given ones"""
    m = surface_model(seed, n_pts)
    return m, given_normals(estimate_normals(m)[0])


def view_case(seeds, sizes, N=2048, per_frame=2, cap=900):
    """The device test's batch, built on the CPU: class 1 + k = surface_model(100 + seed_k, sizes[k]) with estimated normals, seen
    as icp_ref.partial_view(.., 200 + seed_k) (at most `cap` of its points) from synth.eval_pose_pair(seed_k, "near"), `per_frame`
    objects to a frame of N points; class 0 is the background and the last class has no model points.
    -> dict of numpy arrays, the model list, the normals list."""
    from ffb6d_amd import synth
    pairs = [model_with_normals(100 + s, n) for s, n in zip(seeds, sizes)]
    models = models_of([None] + [m for m, _ in pairs] + [None])
    normals = models_of([None] + [n for _, n in pairs] + [None])
    B = (len(seeds) + per_frame - 1) // per_frame
    rng = np.random.RandomState(7)
    pcld = (rng.rand(B, N, 3) * [2.0, 1.2, 1.0] + [-1.0, -0.6, 0.6]).astype(np.float32)
    mask = np.zeros((B, N), np.int64)
    T0, gts, frame_of, class_of = [], [], [], []
    for k, s in enumerate(seeds):
        b, cls = k // per_frame, 1 + k
        pred, gt = synth.eval_pose_pair(s, "near")
        scene = partial_view(models[cls], gt, 200 + s)[:cap]
        at = np.sort(rng.choice(np.flatnonzero(mask[b] == 0), len(scene), replace=False))
        pcld[b, at], mask[b, at] = scene, cls
        T0.append(pred.astype(np.float64))
        gts.append(gt.astype(np.float64))
        frame_of.append(b)
        class_of.append(cls)
    return dict(pcld=pcld, mask=mask, T0=np.stack(T0), gt=np.stack(gts), frame_of=np.array(frame_of, np.int32),
                class_of=np.array(class_of, np.int32)), models, normals


def instance_view_case(seeds, n_model=1024, N=2048, apart=1.5, free=0.4, cap=450):
    """icp_inst_ref.instance_views with normals and at most `cap` points per instance (two classes of two instances fit a frame of
    2048 points): class 1 + k = surface_model(100 + seed_k), frame k // 2, two instances `apart` model radii apart.
    -> dict of numpy arrays, the model list, the normals list."""
    from ffb6d_amd import synth
    pairs = [model_with_normals(100 + s, n_model) for s in seeds]
    models = models_of([None] + [m for m, _ in pairs])
    normals = models_of([None] + [n for _, n in pairs])
    B = (len(seeds) + 1) // 2
    rng = np.random.RandomState(17)
    pcld = (rng.rand(B, N, 3) * [2.0, 1.2, 1.0] + [-1.0, -0.6, 2.6]).astype(np.float32)
    mask, inst = np.zeros((B, N), np.int64), np.zeros((B, N), np.uint8)
    rows = []
    for k, s in enumerate(seeds):
        b, cls = k // 2, 1 + k
        radius = float(np.linalg.norm(models[cls], axis=1).max())
        pred_a, gt_a = (x.astype(np.float64) for x in synth.eval_pose_pair(s, "near"))
        pred_b, gt_b = (x.astype(np.float64) for x in synth.eval_pose_pair(s + 500, "near"))
        side = np.cross(gt_a[:, 3], [0.0, 1.0, 0.0])
        move = gt_a[:, 3] + apart * radius * side / np.linalg.norm(side) - gt_b[:, 3]
        pred_b[:, 3] += move
        gt_b[:, 3] += move
        for iid, (pred, gt) in enumerate(((pred_a, gt_a), (pred_b, gt_b)), 1):
            scene = partial_view(models[cls], gt, 200 + s + 1000 * iid)[:cap]
            at = np.sort(rng.choice(np.flatnonzero(mask[b] == 0), len(scene), replace=False))
            pcld[b, at], mask[b, at] = scene, cls
            inst[b, at] = np.where(rng.rand(len(at)) < free, 0, iid)
            rows.append((b, cls, iid, pred, gt))
    return dict(pcld=pcld, mask=mask, inst=inst, T0=np.stack([r[3] for r in rows]), gt=np.stack([r[4] for r in rows]),
                frame_of=np.array([r[0] for r in rows], np.int32), class_of=np.array([r[1] for r in rows], np.int32),
                inst_of=np.array([r[2] for r in rows], np.int32)), models, normals


def planar_grid(n=32, pitch=0.002):
    """an n x n grid in the plane z = 0 with its exact normal -> (points f32 [n*n,3], normals f32 [n*n,3])"""
    g = (np.arange(n) - (n - 1) / 2.0) * pitch
    pts = np.array([[x, y, 0.0] for x in g for y in g], np.float32)
    return pts, np.tile(np.array([0.0, 0.0, 1.0], np.float32), (len(pts), 1))


def sphere_cloud(seed, n=512, radius=0.05):
    """points on a sphere about the origin with their exact (radial) normals"""
    rng = np.random.RandomState(seed)
    u = rng.randn(n, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    pts = (radius * u).astype(np.float32)
    return pts, given_normals(pts)


def off_pose(seed, deg=6.0, shift=0.008, depth=0.8):
    """(T0, gt) [3,4]: gt a random rotation `depth` metres in front of the camera, T0 `deg` degrees and `shift` metres off it"""
    rng = np.random.RandomState(seed)

    def rot(axis, angle):
        axis = axis / np.linalg.norm(axis)
        return rodrigues(axis * angle)

    gt = np.zeros((3, 4))
    gt[:, :3], gt[:, 3] = rot(rng.randn(3), rng.rand() * np.pi), [0.05 * rng.randn(), 0.05 * rng.randn(), depth]
    T0 = np.zeros((3, 4))
    dt = rng.randn(3)
    T0[:, :3] = rot(rng.randn(3), np.deg2rad(deg)) @ gt[:, :3]
    T0[:, 3] = gt[:, 3] + shift * dt / np.linalg.norm(dt)
    return T0, gt
