"""The rigid fit on the device (csrc/kabsch.h through best_fit_kernel of csrc/pose.hip and icp_solve_kernel of csrc/icp.hip)
against the float64 LAPACK fit of tests/rigid_fit_cases.py, on thin, planar, mirrored, degenerate and far-from-the-origin sets.

Every case of one point count goes into ONE best_fit_transform_batch call (the entry point takes one n per call): 2808 problems
for n >= 4, 2592 below -- more than one workgroup of best_fit_kernel (64 threads, one per problem) and no multiple of 64.

Asserted for every case: R orthonormal with det +1 and t = c_b - R c_a to 1e-12, finite output, and
    objective(R_dev) - objective(R64) <= OBJ_BAR * s1            (objective = sum |R (a - c_a) - (b - c_b)|^2 in long double);
for every case with cond = s1 / (s2 + d s3) <= 1e10 (all but exact rank <= 1 sets and mirrored sets with s2 = s3):
    max |R_dev - R64| <= ROT_BAR * cond.
ROT_BAR and OBJ_BAR are ten times what the reference itself reaches against extended precision
(tests/test_rigid_fit_cpu.py measures and pins them).  Each test prints its largest figure per family before it asserts.

The same functions run on the SIMT emulator from tests/test_rigid_fit_cpu.py."""
import numpy as np
import pytest
import torch

import icp_ref
import rigid_fit_cases as C
from ffb6d_amd import pose

pytestmark = pytest.mark.gpu

_RUNS = {}


def fit_dev(device, A, B):
    T = pose.best_fit_transform_batch(torch.from_numpy(np.array(A, np.float32)).to(device),
                                      torch.from_numpy(np.array(B, np.float32)).to(device))
    return T.cpu().numpy()


def run(device, n):
    """the device's [P,3,4] for every case of n points: one call, made once"""
    key = (str(device), n)
    if key not in _RUNS:
        A, B, _ = C.build(n)
        assert len(A) > 64 and len(A) % 64 != 0
        T = fit_dev(device, A, B)
        T.setflags(write=False)
        _RUNS[key] = T
    return _RUNS[key]


def rot_class(n):
    """cases whose rotation is asserted; every other case must be one the table declares free"""
    _, _, meta = C.build(n)
    sel = C.reference(n)["cond"] <= C.COND_MAX
    for m, s in zip(meta, sel):
        assert s or m["may_be_free"], f"case table: {m} has cond > {C.COND_MAX:g} and is not declared free"
    return sel


@pytest.mark.parametrize("n", C.NS)
def test_output_is_a_rigid_transform(device, n):
    A, B, meta = C.build(n)
    ref, T = C.reference(n), run(device, n)
    assert T.shape == (len(A), 3, 4) and T.dtype == np.float64 and np.isfinite(T).all()
    R, t = T[:, :, :3], T[:, :, 3]
    orth = np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max(axis=(1, 2))
    det = np.abs(np.linalg.det(R) - 1)
    terr = np.abs(t - (ref["cb"] - np.einsum("pij,pj->pi", R, ref["ca"]))).max(axis=1)
    tbar = 1e-12 * (np.linalg.norm(ref["ca"], axis=1) + np.linalg.norm(ref["cb"], axis=1) + 1)
    print(f"n={n}: |R^T R - I| {orth.max():.2e}  |det R - 1| {det.max():.2e}  |t - (cb - R ca)| / bar {np.max(terr / tbar):.2e}")
    assert orth.max() <= 1e-12 and det.max() <= 1e-12
    assert np.all(terr <= tbar)


@pytest.mark.parametrize("n", C.NS)
def test_objective_is_the_minimum(device, n):
    A, B, meta = C.build(n)
    ref, T = C.reference(n), run(device, n)
    excess = C.objective(T[:, :, :3], A, B) - ref["obj"]
    s1 = ref["s"][:, 0].astype(C.LD)
    pos = ref["s"][:, 0] > 0
    print(f"n={n}: largest excess objective / s1 per family:",
          C.by_family(meta, np.where(pos, excess / np.where(pos, s1, 1), 0), pos))
    assert np.all(excess <= C.OBJ_BAR * s1), [meta[i] for i in np.flatnonzero(~(excess <= C.OBJ_BAR * s1))[:5]]


@pytest.mark.parametrize("n", C.NS)
def test_rotation_matches_float64_svd(device, n):
    A, B, meta = C.build(n)
    ref, T, sel = C.reference(n), run(device, n), rot_class(n)
    if not sel.any():
        assert n <= 2                                            # one or two points fix no rotation: the objective test covers them
        return
    err = np.abs(T[:, :, :3] - ref["R"]).max(axis=(1, 2))
    ratio = np.where(sel, err / np.where(sel, ref["cond"], 1), 0)
    print(f"n={n}: {int(sel.sum())} of {len(sel)} cases, largest cond {ref['cond'][sel].max():.2e}; largest |R_dev - R64| / cond per family:",
          C.by_family(meta, ratio, sel))
    bad = np.flatnonzero(ratio > C.ROT_BAR)
    assert len(bad) == 0, [(meta[i], float(ratio[i])) for i in bad[:5]]


def test_zero_covariance_gives_the_identity_exactly(device):
    for n in C.NS:
        _, _, meta = C.build(n)
        T = run(device, n)
        eq = np.array([m["family"] == "equal" or n == 1 for m in meta])
        assert eq.any() and np.array_equal(T[eq][:, :, :3], np.broadcast_to(np.eye(3), (int(eq.sum()), 3, 3)))


def test_a_problem_alone_gives_the_bits_of_the_batch(device):
    for n in (3, 50):
        A, B, meta = C.build(n)
        T = run(device, n)
        picks = [0, 63, 64, len(A) - 1] + [i for i, m in enumerate(meta) if m["family"] in ("rod0.0001", "strip0.001", "line")][::97]
        for i in picks:
            alone = fit_dev(device, A[i:i + 1], B[i:i + 1])
            assert np.array_equal(alone.view(np.uint64), T[i:i + 1].view(np.uint64)), meta[i]


def test_nan_and_inf_problems_leave_their_neighbours_alone(device):
    A, B, _ = C.build(9)
    T = run(device, 9)
    A2, B2 = A.copy(), B.copy()
    A2[5, 3, 1] = np.nan
    B2[64, 0, 0] = np.inf
    A2[130, :, :] = -np.inf
    B2[len(A) - 2, 8, 2] = np.nan
    hit = np.zeros(len(A), bool)
    hit[[5, 64, 130, len(A) - 2]] = True
    T2 = fit_dev(device, A2, B2)                                   # returns: the sweeps are bounded
    assert np.array_equal(T2[~hit].view(np.uint64), T[~hit].view(np.uint64))
    assert not np.isfinite(T2[hit]).all(axis=(1, 2)).any()


@pytest.mark.parametrize("e", [-20, 20])
def test_scaling_by_a_power_of_two(device, e):
    n = 9
    A, B, meta = C.build(n)
    ref, T, sel = C.reference(n), run(device, n), rot_class(n)
    f = np.float32(2.0 ** e)
    As, Bs = A * f, B * f
    assert np.isfinite(As).all() and np.isfinite(Bs).all() and np.array_equal(As / f, A) and np.array_equal(Bs / f, B)
    Ts = fit_dev(device, As, Bs)
    dR = np.abs(Ts[:, :, :3] - T[:, :, :3]).max(axis=(1, 2))
    print(f"2^{e}: largest |R_scaled - R| / cond {np.max(np.where(sel, dR / np.where(sel, ref['cond'], 1), 0)):.2e}")
    assert np.all(dR[sel] <= C.ROT_BAR * ref["cond"][sel])
    na, nb = np.linalg.norm(ref["ca"], axis=1), np.linalg.norm(ref["cb"], axis=1)
    dt = np.abs(Ts[:, :, 3] / float(f) - T[:, :, 3]).max(axis=1)
    assert np.all(dt[sel] <= 3 * C.ROT_BAR * ref["cond"][sel] * na[sel] + 1e-12 * (na + nb + 1)[sel])
    Rs = Ts[:, :, :3]                                              # and t is that of the scaled problem, for every case
    terr = np.abs(Ts[:, :, 3] - float(f) * (ref["cb"] - np.einsum("pij,pj->pi", Rs, ref["ca"]))).max(axis=1)
    assert np.all(terr <= 1e-12 * (float(f) * (na + nb) + 1))


def test_permuting_the_points(device):
    for n in (4, 50):
        A, B, meta = C.build(n)
        ref, T, sel = C.reference(n), run(device, n), rot_class(n)
        perm = np.random.RandomState(n).permutation(n)
        Tp = fit_dev(device, A[:, perm], B[:, perm])
        dR = np.abs(Tp[:, :, :3] - T[:, :, :3]).max(axis=(1, 2))
        ratio = np.where(sel, dR / np.where(sel, ref["cond"], 1), 0)
        print(f"n={n}: largest |R_permuted - R| / cond per family:", C.by_family(meta, ratio, sel))
        assert np.all(ratio <= C.ROT_BAR)


# ---- the ICP path --------------------------------------------------------------------------------------------------------------
def icp_case():
    """One problem per model cloud of rigid_fit_cases.icp_models(), each in a frame of its own: the scene is the model under the
    problem's pose, which is also the pose the iteration starts from, so every correspondence is the identity."""
    named = C.icp_models()
    models = icp_ref.models_of([None] + [m for _, m in named])
    N = max(len(m) for m in models)
    P = len(named)
    rng = np.random.RandomState(77)
    pcld = (rng.rand(P, N, 3) + [5.0, 5.0, 5.0]).astype(np.float32)          # background, far from every object
    mask = np.zeros((P, N), np.int64)
    T0 = np.zeros((P, 3, 4))
    for p in range(P):
        m = models[1 + p]
        T0[p, :, :3], T0[p, :, 3] = C.random_rotation(rng), 0.3 * rng.randn(3)
        at = np.sort(rng.choice(N, len(m), replace=False))
        pcld[p, at] = (m.astype(np.float64) @ T0[p, :, :3].T + T0[p, :, 3]).astype(np.float32)
        mask[p, at] = 1 + p
    return dict(names=[k for k, _ in named], pcld=pcld, mask=mask, T0=T0, frame_of=np.arange(P, dtype=np.int32),
                class_of=np.arange(1, P + 1, dtype=np.int32)), models


def check_icp_one_iteration(run_icp):
    """run_icp(case, models) -> (T f64 [P,3,4], n_pairs [P], iters [P]) of ONE iteration with max_dist = inf"""
    case, models = icp_case()
    T, n_pairs, iters = run_icp(case, models)
    figures = {}
    for p, name in enumerate(case["names"]):
        m = models[1 + p]
        scene = icp_ref.problem_scene(case["pcld"], case["mask"], p, 1 + p)
        want = icp_ref.icp(scene, m, case["T0"][p], 1, float("inf"), dtype=np.float64)
        near, kept = want["history"][0]
        assert kept.all() and np.array_equal(near, np.arange(len(m))), name      # scene point i <-> model point i
        assert n_pairs[p] == len(m) == want["n_pairs"] and iters[p] == 1
        ref = C.fit64(m[near][None], scene[None])
        cond, s1 = float(ref["cond"][0]), float(ref["s"][0, 0])
        assert cond <= C.COND_MAX, (name, cond)
        cancel = (s1 + len(m) * np.linalg.norm(ref["ca"][0]) * np.linalg.norm(ref["cb"][0])) / s1      # H = sum m s^T - n ca cb^T
        err = np.abs(T[p, :, :3] - want["T"][:, :3]).max()
        figures[name] = err / (cond * cancel)
        assert np.abs(T[p, :, 3] - (ref["cb"][0] - T[p, :, :3] @ ref["ca"][0])).max() <= 1e-12 * (
            np.linalg.norm(ref["ca"][0]) + np.linalg.norm(ref["cb"][0]) + 1)
    print("ICP update: |R_dev - R64| / (cond * (s1 + n |ca| |cb|) / s1):", {k: f"{v:.2e}" for k, v in figures.items()})
    bad = {k: v for k, v in figures.items() if not v <= C.ROT_BAR}
    assert not bad, bad


def test_icp_update_on_thin_and_planar_models(device):
    from ffb6d_amd import evaluate, refine

    def run_icp(case, models):
        prepared = refine.PreparedModels(evaluate.ModelPoints(models, device=device))
        d = [torch.from_numpy(case[k]).to(device) for k in ("pcld", "mask")]
        T, st = refine.icp_refine(d[0], d[1], case["T0"], case["frame_of"], case["class_of"], prepared, max_iter=1,
                                  max_dist=float("inf"))
        return T.cpu().numpy(), st["n_pairs"].cpu().numpy(), st["iters"].cpu().numpy()
    check_icp_one_iteration(run_icp)
