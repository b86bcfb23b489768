"""numpy restatement of the rasteriser stated in include/ffb6d_render.h (the reference repository has no rasteriser source,
so there is nothing to port: this file is what ffb6d_amd/render.py and csrc/render.hip are held against, bit for bit).

Everything is float64 / int64 numpy, one operation per rounding, in the header's order (numpy never fuses a multiply with an
add); a triangle is evaluated on all candidate pixels of its clamped bounding box at once.  Also here: the scenes that the
emulator and the device tests share."""
import numpy as np

from ffb6d_amd import synth

NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
INST_BITS, FACE_BITS = 10, 22
MAX_SCREEN = float(1 << 23)


def screen_vertices(xyz, T, K, z_near):
    """-> (Xs i64 [V], Ys i64 [V], zf f32 [V], usable bool [V]) of one instance"""
    p = np.asarray(xyz, np.float32).astype(np.float64)
    T, K = np.asarray(T, np.float64), np.asarray(K, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        Xc = ((T[0, 0] * x + T[0, 1] * y) + T[0, 2] * z) + T[0, 3]
        Yc = ((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * z) + T[1, 3]
        Zc = ((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * z) + T[2, 3]
        zf = Zc.astype(np.float32)
        su = 256.0 * ((K[0, 0] * Xc) / Zc + K[0, 2])
        sv = 256.0 * ((K[1, 1] * Yc) / Zc + K[1, 2])
        usable = (zf >= np.float32(z_near)) & (np.abs(su) <= MAX_SCREEN) & (np.abs(sv) <= MAX_SCREEN)       # NaN: False
    Xs = np.rint(np.where(usable, su, 0.0)).astype(np.int64)                     # np.rint rounds half to even
    Ys = np.rint(np.where(usable, sv, 0.0)).astype(np.int64)
    return Xs, Ys, zf, usable


def triangle(sv, tri):
    """The header's per-triangle set-up -> dict(x i64 [3], y i64 [3], zf f32 [3], vi [3], a2) after the swap, or None when
    the triangle is dropped."""
    Xs, Ys, zf, usable = sv
    vi = [int(v) for v in tri]
    if any(v < 0 or v >= len(Xs) for v in vi) or not all(usable[v] for v in vi):
        return None
    x, y = [int(Xs[v]) for v in vi], [int(Ys[v]) for v in vi]
    a2 = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
    if a2 == 0:
        return None
    if a2 < 0:
        vi, x, y, a2 = [vi[0], vi[2], vi[1]], [x[0], x[2], x[1]], [y[0], y[2], y[1]], -a2
    return dict(x=x, y=y, zf=np.array([zf[v] for v in vi], np.float32), vi=vi, a2=a2)


def candidates(t, H, W):
    """rows, cols (1-D) of the sub-pixel bounding box clamped to the frame"""
    c0, c1 = max(0, -(-min(t["x"]) // 256)), min(W - 1, max(t["x"]) // 256)
    r0, r1 = max(0, -(-min(t["y"]) // 256)), min(H - 1, max(t["y"]) // 256)
    return np.arange(r0, r1 + 1, dtype=np.int64), np.arange(c0, c1 + 1, dtype=np.int64)


def edge_functions(t, rows, cols):
    """E i64 [3, ...] and the covered mask at the samples (256 col, 256 row); rows / cols broadcast against each other"""
    px, py = 256 * cols, 256 * rows
    E, covered = [], True
    for i in range(3):
        a, b = (i + 1) % 3, (i + 2) % 3
        dx, dy = t["x"][b] - t["x"][a], t["y"][b] - t["y"][a]
        e = dx * (py - t["y"][a]) - dy * (px - t["x"][a])
        owner = dy > 0 or (dy == 0 and dx < 0)
        covered = covered & ((e > 0) | ((e == 0) & owner))
        E.append(e)
    return E, covered


def weights(t, E):
    """(b_i * iz_i) [3] and w, float64"""
    a = np.float64(t["a2"])
    with np.errstate(all="ignore"):
        biz = [(e.astype(np.float64) / a) * (1.0 / np.float64(t["zf"][i])) for i, e in enumerate(E)]
    return biz, (biz[0] + biz[1]) + biz[2]


def render(meshes, T, frame_of, class_of, K, B, H, W, z_near=1e-3):
    """meshes: list indexed by class id of None or dict(xyz [V,3], rgb u8 [V,3], faces [F,3]); T [I,3,4]; K [B,3,3] or [3,3].
    -> dict rgb u8 [B,3,H,W], depth f32 [B,H,W], label / inst / face i32 [B,H,W], visible i32 [I], keys u64 [B,H,W]"""
    T = np.asarray(T, np.float64).reshape(-1, 3, 4)
    K = np.broadcast_to(np.asarray(K, np.float64), (B, 3, 3))
    n_inst = len(T)
    assert n_inst <= 1 << INST_BITS
    keys = np.full((B, H, W), NO_KEY, np.uint64)
    svs = {}
    for i in range(n_inst):
        b, c = int(frame_of[i]), int(class_of[i])
        if not (0 <= b < B and 0 <= c < len(meshes)) or meshes[c] is None or len(meshes[c]["faces"]) == 0:
            continue
        m = meshes[c]
        assert len(m["faces"]) <= 1 << FACE_BITS
        svs[i] = screen_vertices(m["xyz"], T[i], K[b], z_near)
        for f, tri in enumerate(np.asarray(m["faces"])):
            t = triangle(svs[i], tri)
            if t is None:
                continue
            rows, cols = candidates(t, H, W)
            if len(rows) == 0 or len(cols) == 0:
                continue
            rr, cc = rows[:, None], cols[None, :]
            E, covered = edge_functions(t, rr, cc)
            if not covered.any():
                continue
            _, w = weights(t, E)
            with np.errstate(all="ignore"):
                z = (1.0 / w).astype(np.float32)
            key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64((i << FACE_BITS) | f)
            view = keys[b, rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]
            view[...] = np.where(covered, np.minimum(view, key), view)
    has = keys != NO_KEY
    low = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    inst = np.where(has, low >> FACE_BITS, -1).astype(np.int32)
    face = np.where(has, low & ((1 << FACE_BITS) - 1), -1).astype(np.int32)
    depth = np.where(has, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0)).astype(np.float32)
    cls = np.asarray(class_of, np.int32)
    label = np.where(has, cls[np.maximum(inst, 0)] if n_inst else 0, 0).astype(np.int32)
    rgb = np.zeros((B, 3, H, W), np.uint8)
    for lo in np.unique(low[has]):
        i, f = int(lo) >> FACE_BITS, int(lo) & ((1 << FACE_BITS) - 1)
        m = meshes[int(class_of[i])]
        t = triangle(svs[i], np.asarray(m["faces"])[f])
        b = int(frame_of[i])
        rows, cols = np.nonzero(has[b] & (low[b] == lo))
        E, _ = edge_functions(t, rows.astype(np.int64), cols.astype(np.int64))
        biz, w = weights(t, E)
        col = np.asarray(m["rgb"], np.uint8)[t["vi"]].astype(np.float64)         # [3 vertices, 3 channels]
        for ch in range(3):
            with np.errstate(all="ignore"):
                q = np.floor(((biz[0] * col[0, ch] + biz[1] * col[1, ch]) + biz[2] * col[2, ch]) / w + 0.5)
            rgb[b, ch, rows, cols] = np.where(q < 255.0, np.maximum(q, 0.0), 255.0).astype(np.uint8)
    visible = np.bincount(inst[has], minlength=n_inst).astype(np.int32) if n_inst else np.zeros(0, np.int32)
    return dict(rgb=rgb, depth=depth, label=label, inst=inst, face=face, visible=visible, keys=keys)


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def pose(t, R=None):
    T = np.zeros((3, 4))
    T[:, :3], T[:, 3] = (np.eye(3) if R is None else R), t
    return T


def pack(meshes):
    """The mesh set as the C ABI takes it: dict verts f32 [Vtot,3], colors u8 [Vtot,3], faces i32 [Ftot,3], vert_begin /
    face_begin i64 [n_cls+1], n_cls, max_verts, max_faces (arrays of at least one row, so that they have an address)."""
    nv = [0 if m is None else len(m["xyz"]) for m in meshes]
    nf = [0 if m is None else len(m["faces"]) for m in meshes]
    live = [m for m in meshes if m is not None]
    cat = lambda k, dt, w: np.ascontiguousarray(np.concatenate([np.asarray(m[k], dt).reshape(-1, w) for m in live] + [np.zeros((1, w), dt)]))  # noqa: E731
    return dict(verts=cat("xyz", np.float32, 3), colors=cat("rgb", np.uint8, 3), faces=cat("faces", np.int32, 3),
                vert_begin=np.concatenate([[0], np.cumsum(nv)]).astype(np.int64),
                face_begin=np.concatenate([[0], np.cumsum(nf)]).astype(np.int64), n_cls=len(meshes), Vtot=int(sum(nv)),
                Ftot=int(sum(nf)), max_verts=int(max(nv)), max_faces=int(max(nf)))


def quad_mesh(x0, y0, x1, y1, z, seed=0, flip=False):
    """Two triangles over the rectangle [x0, x1] x [y0, y1] at depth z (metres, the mesh's own frame), split along the
    diagonal (x0, y0) - (x1, y1)."""
    xyz = np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], np.float32)
    faces = np.array([[0, 2, 1], [0, 3, 2]] if flip else [[0, 1, 2], [0, 2, 3]], np.int32)
    return dict(xyz=xyz, rgb=np.random.RandomState(seed).randint(0, 256, (4, 3)).astype(np.uint8), faces=faces)


SMALL_K = np.array([[61.3, 0.0, 31.4], [0.0, 59.7, 23.7], [0.0, 0.0, 1.0]])


def small_scene():
    """2 frames of 48 x 64.  Classes: 1 a subdivision-2 icosphere (320 faces), 2 a quad larger than the frame, 3 a mesh with one
    vertex behind the near plane and one degenerate face, 4 empty, 5 a second sphere.  Instances: spheres in both frames
    (one cut by the frame's border), the quad behind them in frame 1, two identical instances at one pose (the tie goes to the
    lower one), mesh 3, the empty class, a frame index of 7, a class id of 9, a NaN pose."""
    rng = np.random.RandomState(11)
    odd = dict(xyz=np.array([[-0.05, -0.04, 0.0], [0.06, -0.03, 0.01], [0.0, 0.05, 0.02], [0.07, 0.06, -0.01], [0.0, 0.0, -0.7],
                             [-0.08, 0.07, 0.03]], np.float32),
               rgb=rng.randint(0, 256, (6, 3)).astype(np.uint8),
               faces=np.array([[0, 1, 2], [1, 3, 2], [0, 2, 4], [2, 2, 3], [0, 2, 5], [1, 1, 1]], np.int32))
    meshes = [None, synth.sphere_mesh(2, 0.1, seed=3), quad_mesh(-2.0, -1.5, 2.0, 1.5, 0.0, seed=4), odd, None,
              synth.sphere_mesh(1, 0.07, seed=5)]
    R = synth.random_rotation(rng)
    inst = [(0, 1, pose([0.02, -0.01, 0.55], R)),
            (0, 3, pose([-0.12, 0.08, 0.6], synth.rot_z(0.3))),
            (0, 5, pose([0.05, 0.02, 0.42])),                                     # in front of the first sphere
            (1, 2, pose([0.0, 0.0, 1.25], synth.rot_z(0.1))),                    # fills frame 1 behind everything
            (1, 1, pose([-0.1, 0.03, 0.6], R.T)),
            (1, 1, pose([-0.1, 0.03, 0.6], R.T)),                                # the same again: loses every tie
            (1, 5, pose([0.26, 0.2, 0.6])),                                      # cut by the border
            (1, 4, pose([0.0, 0.0, 0.5])),                                       # empty class
            (7, 1, pose([0.0, 0.0, 0.5])),                                       # no such frame
            (0, 9, pose([0.0, 0.0, 0.5])),                                       # no such class
            (0, 1, pose([np.nan, 0.0, 0.5]))]                                    # NaN pose
    return dict(meshes=meshes, T=np.stack([t for _, _, t in inst]), frame_of=np.array([b for b, _, _ in inst], np.int32),
                class_of=np.array([c for _, c, _ in inst], np.int32), K=np.stack([SMALL_K, SMALL_K * [[1.1], [0.9], [1.0]]]),
                B=2, H=48, W=64)
