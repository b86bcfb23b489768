"""Cases and independent references for the rigid fit (csrc/kabsch.h: best_fit_transform and the ICP update): thin, planar,
mirrored, degenerate and far-from-the-origin point sets, the float64 LAPACK fit they are held against, the same fit in extended
precision that measures how good that reference is, and the least-squares objective in extended precision.  No GPU, no package
import: numpy only.

Terms.  H = sum (a_i - c_a)(b_i - c_b)^T = U diag(s1, s2, s3) V^T, d = det(V U^T) = +-1 (the reference's reflection
correction, ffb6d/utils/pvn3d_eval_utils_kpls.py:53-56), R = V diag(1, 1, d) U^T.  cond = s1 / (s2 + d s3) is the sensitivity
of R to a perturbation of H relative to s1 (infinite when s2 + d s3 <= 0: the rotation about the first axis is then free).

The bars of tests/test_rigid_fit_gpu.py come from REF_ROT and REF_OBJ below: what fit64 reaches against fit_ld on these very
cases, measured and pinned by tests/test_rigid_fit_cpu.py -- never from what a kernel gives."""
import functools

import numpy as np

LD = np.longdouble
EXTENT = 0.1
NS = (1, 2, 3, 4, 9, 50)
TAUS = (1e-1, 1e-2, 1e-3, 1e-4)
ROTATIONS = ("random", "pi", "tiny", "identity")
NOISES = (0.0, 1e-3, 1e-1)
OFFSETS = (0.0, 2.0, 2000.0)
SEEDS = (0, 1, 2)
COND_MAX = 1e10                # the rotation is asserted for cond <= COND_MAX
COND_BAND = (3e9, 3e10)        # no case lies here, so no rounding of the reference decides a case's class

# measured by tests/test_rigid_fit_cpu.py::test_reference_against_extended_precision (fit64 against fit_ld, every case):
REF_ROT = 9.2e-15              # largest |R64 - R_ld| / cond over the cases with cond <= COND_MAX
REF_OBJ = 3.4e-15              # largest (objective(R64) - objective(R_ld)) / s1
ROT_BAR = 10 * REF_ROT         # |R_dev - R64| <= ROT_BAR * cond
OBJ_BAR = 10 * REF_OBJ         # objective(R_dev) - objective(R64) <= OBJ_BAR * s1


def families(n):
    """(name, extent ratios or None) of the point-set families that exist for n points"""
    out = [("full", (1, 1, 1)), ("planar", (1, 1, 0))]
    out += [(f"strip{t:g}", (1, t, 0)) for t in TAUS] + [(f"rod{t:g}", (1, t, t)) for t in TAUS]
    out += [("line", None), ("equal", None)]
    if n >= 4:
        out.append(("cube", None))
    return out


def rotation_about(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] *= -1
    return q


def cube_points(n):
    """n >= 4 points with sum a a^T a multiple of the identity (s1 = s2 = s3): alternate corners of a cube for n = 4, else whole
    cubes of shrinking size, the rest at the centre"""
    c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    if n < 8:
        pts = [c[[7, 4, 2, 1]]]
    else:
        pts = [c * (1 - 0.1 * k) for k in range(n // 8)]
    pts = np.concatenate(pts + [np.zeros((n, 3))])[:n]
    return pts * (EXTENT / 2)


def base_points(family, ratios, n, rng):
    """the model set about its own centre, float64 [n,3]"""
    if family == "equal":
        return np.zeros((n, 3))
    if family == "line":                                        # axis-parallel to (1, 2, 3): an exact line in float32 as it stands
        return np.outer(np.linspace(-1, 1, n) if n > 1 else np.zeros(1), [1, 2, 3]) * (EXTENT / 8)
    if family == "cube":
        return cube_points(n)
    return (rng.rand(n, 3) - 0.5) * np.asarray(ratios, np.float64) * EXTENT @ random_rotation(rng).T


def make_case(family, ratios, n, rot, mirror, noise, offset, seed):
    """-> A, B float32 [n,3]: B = R A + t (+ noise) (mirrored in z), the model's centre `offset` units from the origin"""
    rng = np.random.RandomState(seed)
    pts = base_points(family, ratios, n, rng)
    u = rng.randn(3)
    A = (pts + offset * u / np.linalg.norm(u)).astype(np.float32)
    axis = rng.randn(3)
    R = {"random": lambda: random_rotation(rng), "pi": lambda: 2 * np.outer(axis, axis) / (axis @ axis) - np.eye(3),
         "tiny": lambda: rotation_about(axis, 1e-7), "identity": lambda: np.eye(3)}[rot]()
    t = 0.3 * rng.randn(3) if (rot != "identity" or offset) else np.array([0.5, 0.5, 0.5])
    B = A.astype(np.float64) @ R.T + t + noise * EXTENT * rng.randn(n, 3)
    if mirror:
        B = B * [1, 1, -1]
    return A, B.astype(np.float32)


def may_be_free(family, n, mirror):
    """the cases whose rotation may be undetermined (cond > COND_MAX): rank <= 1 sets, and mirrored sets with s2 = s3"""
    return family in ("line", "equal") or n <= 2 or (family == "cube" and mirror)


def _cond_of(A, B):
    return float(fit64(A[None], B[None])["cond"][0])


@functools.lru_cache(maxsize=None)
def build(n):
    """Every case with n points -> (A f32 [P,n,3], B f32 [P,n,3], meta: list of dicts).  Deterministic.  A draw whose cond falls
    into COND_BAND, or above COND_MAX in a family that is meant to fix its rotation, is drawn again with the next seed: the class
    of a case is decided here, by the reference alone."""
    As, Bs, meta = [], [], []
    for family, ratios in families(n):
        for rot in ROTATIONS:
            for mirror in (False, True):
                for noise in NOISES:
                    for offset in OFFSETS:
                        for seed in SEEDS:
                            free_ok = may_be_free(family, n, mirror)
                            for attempt in range(50):
                                s = (len(meta) * 50 + attempt) * 7 + seed
                                A, B = make_case(family, ratios, n, rot, mirror, noise, offset, s)
                                c = _cond_of(A, B)
                                if not (COND_BAND[0] <= c <= COND_BAND[1]) and (free_ok or c < COND_BAND[0]):
                                    break
                            else:
                                raise RuntimeError(f"no usable draw for {family} n={n} {rot} mirror={mirror} noise={noise} offset={offset}")
                            As.append(A)
                            Bs.append(B)
                            meta.append(dict(family=family, n=n, rot=rot, mirror=mirror, noise=noise, offset=offset, seed=s,
                                             may_be_free=free_ok))
    A, B = np.stack(As), np.stack(Bs)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B, meta


# ---- the float64 reference --------------------------------------------------------------------------------------------------
def fit64(A, B):
    """The reference's best_fit_transform (pvn3d_eval_utils_kpls.py:28-61) on the float32 points taken to float64, two-pass
    centring, LAPACK's SVD, the det < 0 correction (:53-56), for a batch [P,n,3]
    -> dict R [P,3,3], t [P,3], ca, cb [P,3], s [P,3] (descending), d [P] (+-1), cond [P] (inf where s2 + d s3 <= 0)"""
    A, B = np.asarray(A, np.float32).astype(np.float64), np.asarray(B, np.float32).astype(np.float64)
    ca, cb = A.mean(axis=1), B.mean(axis=1)
    H = np.einsum("pni,pnj->pij", A - ca[:, None], B - cb[:, None])
    U, s, Vt = np.linalg.svd(H)
    R = np.swapaxes(Vt, 1, 2) @ np.swapaxes(U, 1, 2)
    d = np.where(np.linalg.det(R) < 0, -1.0, 1.0)
    Vt = Vt.copy()
    Vt[:, 2, :] *= d[:, None]
    R = np.swapaxes(Vt, 1, 2) @ np.swapaxes(U, 1, 2)
    gap = s[:, 1] + d * s[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.where(gap > 0, s[:, 0] / np.where(gap > 0, gap, 1.0), np.inf)
    return dict(R=R, t=cb - np.einsum("pij,pj->pi", R, ca), ca=ca, cb=cb, s=s, d=d, cond=cond)


# ---- the same fit in extended precision ----------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _unit(a, fallback):
    n = np.sqrt((a * a).sum(axis=1))
    ok = n > 0
    return np.where(ok[:, None], a / np.where(ok, n, 1)[:, None], fallback), n


def jacobi_svd_ld(H, sweeps=60):
    """Cyclic one-sided Jacobi on a batch of 3x3 matrices in np.longdouble, elementwise numpy throughout (LAPACK has no long
    double): -> G = H V with orthogonal columns, V orthogonal."""
    G = np.array(H, LD)
    V = np.broadcast_to(np.eye(3, dtype=LD), G.shape).copy()
    tol = 4 * np.finfo(LD).eps
    for _ in range(sweeps):
        any_rot = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            alpha, beta = (G[:, :, p] ** 2).sum(axis=1), (G[:, :, q] ** 2).sum(axis=1)
            gamma = (G[:, :, p] * G[:, :, q]).sum(axis=1)
            act = np.abs(gamma) > tol * np.sqrt(alpha) * np.sqrt(beta)
            if not act.any():
                continue
            any_rot = True
            g = np.where(act, gamma, LD(1))
            zeta = (beta - alpha) / (2 * g)
            t = np.where(zeta >= 0, LD(1), LD(-1)) / (np.abs(zeta) + np.sqrt(zeta * zeta + 1))
            cs = 1 / np.sqrt(t * t + 1)
            sn = np.where(act, t * cs, LD(0))
            cs = np.where(act, cs, LD(1))
            for M in (G, V):
                mp, mq = M[:, :, p].copy(), M[:, :, q].copy()
                M[:, :, p] = cs[:, None] * mp - sn[:, None] * mq
                M[:, :, q] = sn[:, None] * mp + cs[:, None] * mq
        if not any_rot:
            break
    return G, V


def fit_ld(A, B):
    """fit64 in np.longdouble -> dict R [P,3,3], s [P,3], d [P] (all longdouble).  Its only use is to measure fit64."""
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than float64 on this platform"
    A, B = np.asarray(A, np.float32).astype(LD), np.asarray(B, np.float32).astype(LD)
    n = LD(A.shape[1])
    ca, cb = A.sum(axis=1) / n, B.sum(axis=1) / n
    Ac, Bc = A - ca[:, None], B - cb[:, None]
    H = (Ac[:, :, :, None] * Bc[:, :, None, :]).sum(axis=1)
    G, V = jacobi_svd_ld(H)
    order = np.argsort(-(G * G).sum(axis=1), axis=1, kind="stable")
    P = np.arange(len(G))
    g = [G[P, :, order[:, k]] for k in range(3)]
    v = [V[P, :, order[:, k]] for k in range(3)]
    ex = np.broadcast_to(np.array([1, 0, 0], LD), g[0].shape)
    u1, s1 = _unit(g[0], ex)
    zero = s1 == 0                                              # H = 0: the identity (V = I then, u_k := v_k)
    u1 = np.where(zero[:, None], v[0], u1)
    u2, s2 = _unit(g[1], ex)
    u2 = u2 - (u2 * u1).sum(axis=1)[:, None] * u1
    u2, rest = _unit(u2, ex)
    k = np.argmin(np.abs(u1), axis=1)
    alt, _ = _unit(_cross(u1, np.eye(3, dtype=LD)[k]), ex)      # rank 1: any unit vector orthogonal to u1
    free = ~(s2 > LD(2) ** -68 * s1) | ~(rest > 0.5)
    u2 = np.where(free[:, None], alt, u2)
    u2 = np.where(zero[:, None], v[1], u2)
    u3, v3 = _cross(u1, u2), _cross(v[0], v[1])
    R = v[0][:, :, None] * u1[:, None, :] + v[1][:, :, None] * u2[:, None, :] + v3[:, :, None] * u3[:, None, :]
    s3 = np.sqrt((g[2] * g[2]).sum(axis=1))
    d = np.where((_cross(g[0], g[1]) * g[2]).sum(axis=1) * (v3 * v[2]).sum(axis=1) < 0, LD(-1), LD(1))
    return dict(R=R, s=np.stack([s1, s2, s3], axis=1), d=d)


def objective(R, A, B):
    """sum |R (a - c_a) - (b - c_b)|^2 in np.longdouble, per problem [P]"""
    A, B = np.asarray(A, np.float32).astype(LD), np.asarray(B, np.float32).astype(LD)
    n = LD(A.shape[1])
    Ac, Bc = A - (A.sum(axis=1) / n)[:, None], B - (B.sum(axis=1) / n)[:, None]
    R = np.asarray(R).astype(LD)
    RA = (Ac[:, :, None, :] * R[:, None, :, :]).sum(axis=3)
    return ((RA - Bc) ** 2).sum(axis=(1, 2))


@functools.lru_cache(maxsize=None)
def reference(n):
    """fit64 of build(n) with its objective (longdouble [P]); computed once, shared, read-only"""
    A, B, _ = build(n)
    ref = fit64(A, B)
    ref["obj"] = objective(ref["R"], A, B)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def by_family(meta, values, sel=None):
    """largest value per family (over the selected cases) as a printable dict"""
    out = {}
    for i, m in enumerate(meta):
        if sel is None or sel[i]:
            out[m["family"]] = max(out.get(m["family"], 0.0), float(values[i]))
    return out


# ---- model clouds for the ICP path ----------------------------------------------------------------------------------------------
def icp_models():
    """Thin and planar model clouds, each centred and with its centroid 2 units out: (name, points f32 [n,3]) with n in 64..256.
    The long axis is stratified (neighbours at least EXTENT / 2n apart), so that under the exact pose every scene point's nearest
    model point is its own."""
    out = []
    fams = [("planar", (1, 1, 0))] + [(f"strip{t:g}", (1, t, 0)) for t in TAUS] + [(f"rod{t:g}", (1, t, t)) for t in TAUS]
    for k, (name, ratios) in enumerate(fams):
        for offset in (0.0, 2.0):
            rng = np.random.RandomState(900 + 2 * k + int(offset))
            n = (64, 100, 130, 256)[k % 4]
            x = (np.arange(n) + 0.5 * rng.rand(n)) / n - 0.5
            pts = np.stack([x, rng.rand(n) - 0.5, rng.rand(n) - 0.5], axis=1) * np.asarray(ratios, np.float64) * EXTENT
            u = rng.randn(3)
            pts = pts @ random_rotation(rng).T + offset * u / np.linalg.norm(u)
            out.append((f"{name}@{offset:g}", pts[rng.permutation(n)].astype(np.float32)))
    return out
