"""numpy restatement of the instance calls of include/ffb6d_refine.h (problems (frame, class, instance), modes "map" and
"nearest"): what refine.correspondences_instances / icp_refine_instances and the *_inst entry points of csrc/icp.hip are held
against.  Steps 1-4 of one problem are those of tests/icp_ref.py, used from there unchanged; this file adds the scene sets cut by
the instance map, the group and owner rule, the loop in which the members of a group compete, and the cases of the tests."""
import numpy as np

from icp_ref import (add, best_fit, box_move, correspond, correspondences, first_divergence, icp, icp_refine, models_of,      # noqa: F401
                     partial_view, problem_model, problem_scene, surface_model)
import icp_ref


def scene_indices(mask, frame, cls, keep=None, inst=None, inst_of=None):
    """icp_ref.scene_indices; inst (u8 [B,N]) given: the map form -- only the points with inst == inst_of, none for an inst_of
    outside 1 .. 255"""
    at = icp_ref.scene_indices(mask, frame, cls, keep)
    if inst is None or len(at) == 0:
        return at
    if not 1 <= inst_of <= 255:
        return np.zeros(0, np.int64)
    return at[inst[frame][at] == inst_of]


# ---- several instances of a class (the instance calls of include/ffb6d_refine.h) -------------------------------------------
def groups(frame_of, class_of, mode="nearest"):
    """(begin, end) per problem: the maximal run of adjacent problems with its frame and class; map mode: the problem alone"""
    P = len(frame_of)
    out = []
    for p in range(P):
        lo, hi = p, p + 1
        if mode == "nearest":
            while lo > 0 and frame_of[lo - 1] == frame_of[p] and class_of[lo - 1] == class_of[p]:
                lo -= 1
            while hi < P and frame_of[hi] == frame_of[p] and class_of[hi] == class_of[p]:
                hi += 1
        out.append((lo, hi))
    return out


def owner(d2):
    """d2 [G,n] (the members' smallest distances to the same n scene points) -> i64 [n]: the row with the smallest distance,
    compared in d2's dtype; a NaN never owns, the first of equals stays; -1 when every row is NaN"""
    own = np.full(d2.shape[1], -1, np.int64)
    best = np.zeros(d2.shape[1], d2.dtype)
    with np.errstate(invalid="ignore"):
        for g in range(d2.shape[0]):
            take = ~np.isnan(d2[g]) & ((own < 0) | (d2[g] < best))
            own[take], best[take] = g, d2[g][take]
    return own


def _inst_scenes(pcld, mask, inst, frame_of, class_of, inst_of, mode, keep):
    at = [scene_indices(mask, int(frame_of[p]), int(class_of[p]), keep, inst if mode == "map" else None, int(inst_of[p]))
          for p in range(len(frame_of))]
    return at, [pcld[frame_of[p]][i] if len(i) else np.zeros((0, 3), np.float32) for p, i in enumerate(at)]


def _claim(c, grp, p):
    """kept mask of problem p and the owner of each of its scene points (problem index), from the correspondences of all"""
    lo, hi = grp[p]
    own = owner(np.stack([c[q]["d2"] for q in range(lo, hi)]))
    own = np.where(own >= 0, own + lo, -1)
    return c[p]["kept"] & (own == p), own


def correspondences_instances(pcld, mask, inst, T, frame_of, class_of, inst_of, models, max_dist, mode="map", keep=None, dtype=np.float32):
    """steps 1-3 of every problem of an instance call -> idx i32 [P,N], d2 [P,N], counts i32 [P], owner i32 [P,N] (problem
    index; -1 beyond the count or when no member of the group has a non-NaN distance)"""
    assert mode in ("map", "nearest")
    P, N = len(frame_of), pcld.shape[1]
    idx, d2, own = np.full((P, N), -1, np.int32), np.full((P, N), np.inf, dtype), np.full((P, N), -1, np.int32)
    counts = np.zeros(P, np.int32)
    _, scenes = _inst_scenes(pcld, mask, inst, frame_of, class_of, inst_of, mode, keep)
    c = [correspond(scenes[p], problem_model(models, int(class_of[p])), T[p], max_dist, dtype) for p in range(P)]
    grp = groups(frame_of, class_of, mode)
    for p in range(P):
        n = len(scenes[p])
        kept, o = _claim(c[:], grp, p)
        counts[p] = n
        idx[p, :n], d2[p, :n], own[p, :n] = np.where(kept, c[p]["nearest"], -1), c[p]["d2"], o
    return idx, d2, counts, own


def icp_refine_instances(pcld, mask, inst, T0, frame_of, class_of, inst_of, models, max_iter, max_dist, mode="map", tol=0.0, min_pairs=3,
                         keep=None, dtype=np.float32):
    """The loop of an instance call -> (T f64 [P,3,4], dict n_pairs, rms, iters, inst u8 [B,N], writers i32 [B,N] (problems that
    keep the point at the end: inst is decided where it is <= 1), history (per problem, per iteration made: nearest, kept)).
    map: every problem on its own, on the points the map gives it.  nearest: all problems measure their distances under the
    poses that go into the iteration, stopped problems included; then the owners, the gate and the updates."""
    assert mode in ("map", "nearest")
    P = len(frame_of)
    at, scenes = _inst_scenes(pcld, mask, inst, frame_of, class_of, inst_of, mode, keep)
    mods = [np.asarray(problem_model(models, int(class_of[p])), np.float32).reshape(-1, 3) for p in range(P)]
    grp = groups(frame_of, class_of, mode)
    T = np.array(T0, np.float64).reshape(P, 3, 4).copy()
    done, last = np.zeros(P, bool), [np.zeros(len(s), bool) for s in scenes]
    n_pairs, rms, iters = np.zeros(P, np.int32), np.zeros(P, np.float32), np.zeros(P, np.int32)
    history = [[] for _ in range(P)]
    for _ in range(max_iter):
        c = [correspond(scenes[p], mods[p], T[p], max_dist, dtype) if (mode == "nearest" or not done[p]) else None for p in range(P)]
        for p in range(P):
            if c[p] is None:
                continue
            k, _ = _claim(c, grp, p)
            last[p] = k
            if done[p]:
                continue
            history[p].append((c[p]["nearest"], k))
            n_pairs[p] = int(k.sum())
            rms[p] = np.float32(np.sqrt(c[p]["d2"][k].astype(np.float64).sum() / n_pairs[p])) if n_pairs[p] else np.float32(0)
            if n_pairs[p] < min_pairs:
                done[p] = True
                continue
            Tn = best_fit(mods[p][c[p]["nearest"][k]], scenes[p][k])
            if tol > 0 and box_move(mods[p], Tn, T[p]) <= tol:
                done[p] = True
            T[p], iters[p] = Tn, iters[p] + 1
    out, writers = np.zeros(mask.shape, np.uint8), np.zeros(mask.shape, np.int32)
    for p in range(P):
        if len(at[p]):
            out[frame_of[p], at[p][last[p]]] = int(inst_of[p]) & 255
            writers[frame_of[p], at[p][last[p]]] += 1
    return T, dict(n_pairs=n_pairs, rms=rms, iters=iters, inst=out, writers=writers, history=history)


def first_divergence_instances(pcld, mask, inst, T0, frame_of, class_of, inst_of, models, max_iter, max_dist, mode="map", tol=0.0,
                               min_pairs=3, keep=None):
    """Per problem: the iteration in which the float32 and the float64 restatement pick a different correspondence or keep a
    different set, in the problem itself or (nearest) in any member of its group, or None."""
    run = lambda dt: icp_refine_instances(pcld, mask, inst, T0, frame_of, class_of, inst_of, models, max_iter, max_dist, mode, tol,       # noqa: E731
                                          min_pairs, keep, dt)[1]["history"]
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
    for lo, hi in groups(frame_of, class_of, mode):
        its = [i for i in own[lo:hi] if i is not None]
        out.append(min(its) if its else None)
    return out


# ---- cases with several instances of a class ---------------------------------------------------------------------------
def instances_case(N=192, mask_dtype=np.int64):
    """The tiny ragged case of the instance calls.  Classes of 130 / 70 / 0 / 1100 points (ids 1 .. 4; the last crosses the
    automatic form's 1024), two frames of N points.  Problems (frame, class, instance):
       0-2   three instances of class 1 in frame 0 with 64, 65 and 7 points of their own (three of the first NaN)
       3-4   two instances of class 4 in frame 1 (30 and 25 points)
       5     class 2 in frame 1, alone (40 points)
       6-8   frame 0, class 1 again, not adjacent to 0-2: instance 2 once more, an instance no point carries (9), instance 255
       9-10  frame 1, class 4 again: instance ids 0 and 256
       11    a frame that is no index;   12  class 3, which has scene points and no model
    Every class has points of instance 0 as well.  The scene points are model points under a pose a little off the problem's."""
    from ffb6d_amd import synth
    rng = np.random.RandomState(11)
    models = models_of([None, surface_model(1, 130), surface_model(2, 70), None, surface_model(4, 1100)])
    B = 2
    pcld = (rng.rand(B, N, 3) * [2.0, 1.2, 1.0] + [-1.0, -0.6, 0.6]).astype(np.float32)
    mask, inst = np.zeros((B, N), np.int64), np.zeros((B, N), np.uint8)
    placed = {}                                                                   # (frame, class, instance) -> (pred, gt)

    def place(b, cls, iid, n, seed, shift, n_free):
        pred, gt = (x.astype(np.float64) for x in synth.eval_pose_pair(seed, "near"))
        pred[:, 3] += shift
        gt[:, 3] += shift
        m = models[cls]
        if len(m):
            d = 0.5 * (gt - pred) + pred                                         # the points lie under a pose between the two
            pts = (m[rng.randint(0, len(m), n + n_free)].astype(np.float64) @ d[:, :3].T + d[:, 3] + 0.001 * rng.randn(n + n_free, 3))
        else:
            pts = gt[:, 3] + 0.02 * rng.randn(n + n_free, 3)
        at = np.sort(rng.choice(np.flatnonzero(mask[b] == 0), n + n_free, replace=False))
        pcld[b, at], mask[b, at] = pts.astype(np.float32), cls
        own = rng.permutation(n + n_free)[:n]
        inst[b, at[own]] = iid
        placed[b, cls, iid] = pred
        return at[np.sort(own)]

    first = place(0, 1, 1, 64, 70, [0.0, 0.0, 0.0], 4)
    place(0, 1, 2, 65, 71, [0.12, 0.0, 0.0], 3)
    place(0, 1, 3, 7, 72, [-0.12, 0.05, 0.0], 3)
    place(0, 1, 255, 5, 73, [0.0, -0.12, 0.0], 0)
    place(1, 4, 1, 30, 74, [0.0, 0.0, 0.0], 3)
    place(1, 4, 2, 25, 75, [0.13, 0.0, 0.0], 3)
    place(1, 2, 1, 40, 76, [0.0, 0.0, 0.0], 5)
    place(1, 3, 1, 8, 77, [0.0, 0.0, 0.0], 2)
    pcld[0, first[:3]] = np.nan
    problems = [(0, 1, 1), (0, 1, 2), (0, 1, 3), (1, 4, 1), (1, 4, 2), (1, 2, 1), (0, 1, 2), (0, 1, 9), (0, 1, 255), (1, 4, 0), (1, 4, 256),
                (7, 1, 1), (1, 3, 1)]
    like = {(0, 1, 9): (0, 1, 1), (1, 4, 0): (1, 4, 1), (1, 4, 256): (1, 4, 2), (7, 1, 1): (0, 1, 1)}
    T = np.stack([placed[like.get(k, k)] for k in problems])
    T[6:11, :, 3] += 0.002 * rng.randn(5, 3)                                      # the repeated pairs: not the first group's poses
    keep = (rng.rand(B, N) < 0.8).astype(np.uint8)
    return dict(pcld=pcld, mask=mask.astype(mask_dtype), inst=inst, T=T, keep=keep, frame_of=np.array([p[0] for p in problems], np.int32),
                class_of=np.array([p[1] for p in problems], np.int32), inst_of=np.array([p[2] for p in problems], np.int32)), models


def instance_views(seeds, n_model=1024, N=4096, apart=1.5, free=0.4):
    """Two instances of every class, `apart` model radii apart, as partial views: class 1 + k = surface_model(100 + seed_k), frame k // 2.
    The poses are perturbed as synth.eval_pose_pair(seed, "near") does, and the share `free` of each instance's points has
    instance 0 in the map.  Rows ordered by (frame, class, instance).  -> dict of numpy arrays (truth i8 [B,N]: the instance a
    point was drawn from, 0 = background) + the model list."""
    from ffb6d_amd import synth
    models = [None] + [surface_model(100 + s, n_model) for s in seeds]
    B = (len(seeds) + 1) // 2
    rng = np.random.RandomState(17)
    pcld = (rng.rand(B, N, 3) * [2.0, 1.2, 1.0] + [-1.0, -0.6, 2.6]).astype(np.float32)
    mask, inst, truth = np.zeros((B, N), np.int64), np.zeros((B, N), np.uint8), np.zeros((B, N), np.int8)
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
            scene = partial_view(models[cls], gt, 200 + s + 1000 * iid)
            at = np.sort(rng.choice(np.flatnonzero(mask[b] == 0), len(scene), replace=False))
            pcld[b, at], mask[b, at], truth[b, at] = scene, cls, iid
            inst[b, at] = np.where(rng.rand(len(at)) < free, 0, iid)
            rows.append((b, cls, iid, pred, gt))
    return dict(pcld=pcld, mask=mask, inst=inst, truth=truth, T0=np.stack([r[3] for r in rows]), gt=np.stack([r[4] for r in rows]),
                frame_of=np.array([r[0] for r in rows], np.int32), class_of=np.array([r[1] for r in rows], np.int32),
                inst_of=np.array([r[2] for r in rows], np.int32)), models_of(models)
