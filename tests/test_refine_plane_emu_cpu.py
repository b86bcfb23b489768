"""The point-to-plane metric of csrc/icp.hip on the SIMT emulator (tests/simt), without a GPU: the normals (estimated and given),
ffb6d_icp_refine_plane_f32 and ffb6d_icp_refine_plane_inst_f32 through the C ABI on tiny ragged problems, held against the numpy
restatement (tests/icp_plane_ref.py) -- the normals to 1e-12 where the restatement's spectrum decides them, the loop within the bar
of the device test, both forms of the search as bits, degenerate problems and max_iter = 0 as bits, and the point calls' bits
untouched by a plane call made before them."""
import numpy as np
import pytest

import icp_inst_ref as iref
import icp_plane_ref as pref
import icp_ref
from ffb6d_amd import synth
from test_refine_emu_cpu import _p, prepare
from test_refine_instances_emu_cpu import MODE, refine_inst
from tests.simt.build import load

MIN_EIG = 1e-6


@pytest.fixture(scope="module")
def emu():
    """the emulated library (tests/simt/build.py); the search form is back at its default when the module is over"""
    lib = load()
    yield lib
    lib.ffb6d_icp_set_form(0)


def plane_case():
    """Classes of 130 / 70 / 0 / 18 (a planar grid with duplicated rows) / 2 points (ids 1 .. 5), two frames of 192 points, eight
    problems with scene sets of 70 (three of them NaN), 40, 4 (the grid), 0, 1 (the class of two points), 65 (a block of 64 and a
    block of one lane), 9 (the class without model points) and 0 (a frame that is no index) points.  Some normals of class 2 are
    given as zero, NaN and inf: they become the zero vector."""
    rng = np.random.RandomState(5)
    g = np.arange(4) / 64.0
    grid = np.array([[x, y, 0.0] for x in g for y in g] + [[g[0], g[3], 0.0], [g[2], g[2], 0.0]], np.float32)
    two = np.array([[0.0, 0.0, 0.0], [0.01, 0.02, 0.0]], np.float32)
    models = icp_ref.models_of([None, icp_ref.surface_model(1, 130), icp_ref.surface_model(2, 70), None, grid, two])
    B, N = 2, 192
    pcld = (rng.rand(B, N, 3) * [2.0, 1.2, 1.0] + [-1.0, -0.6, 0.6]).astype(np.float32)
    mask = np.zeros((B, N), np.int64)
    problems = [(0, 1), (0, 2), (1, 4), (1, 2), (1, 5), (1, 1), (1, 3), (7, 1)]
    T = np.zeros((len(problems), 3, 4))
    for p, (b, cls) in enumerate(problems):
        pred, gt = synth.eval_pose_pair(60 + p, "near")
        T[p] = pred
        n = {0: 70, 1: 40, 5: 65}.get(p)
        if n:
            m = models[cls]
            d = 0.3 * (gt.astype(np.float64) - pred) + pred                       # a pose a little off the problem's own
            scene = (m[rng.randint(0, len(m), n)].astype(np.float64) @ d[:, :3].T + d[:, 3] + 0.001 * rng.randn(n, 3)).astype(np.float32)
            at = np.sort(rng.choice(np.flatnonzero(mask[b] == 0), n, replace=False))
            pcld[b, at], mask[b, at] = scene, cls
    T[2, :, :3], T[2, :, 3] = np.eye(3), [0.0, 0.0, 1.0]
    T[4, :, :3], T[4, :, 3] = np.eye(3), [0.0, 0.0, 1.0]
    at = np.flatnonzero(mask[1] == 0)[:4]                                         # the grid: four points off the plane, tilted
    xy = np.array([[g[1] + 0.001, g[1]], [g[2], g[1] + 0.001], [g[1], g[2] - 0.001], [g[3], g[3]]])
    pcld[1, at] = np.column_stack([xy, 1.002 + 0.02 * xy[:, 0] - 0.03 * xy[:, 1]])      # (coplanar: the residual can vanish)
    mask[1, at] = 4
    at = np.flatnonzero(mask[1] == 0)[:1]
    pcld[1, at], mask[1, at] = [[0.001, 0.001, 1.001]], 5
    mask[1, np.flatnonzero(mask[1] == 0)[:9]] = 3
    pcld[0, np.flatnonzero(mask[0] == 1)[:3]] = np.nan                            # NaN scene points of problem 0
    normals_in = [pref.estimate_normals(m)[0] for m in models]
    normals_in[2][[3, 17, 40]] = [[0.0, 0.0, 0.0], [np.nan, 1.0, 0.0], [np.inf, 0.0, 0.0]]
    normals_in[2][5] *= 3.0                                                       # (and one that is not of unit length)
    return dict(pcld=pcld, mask=mask, T=T, frame_of=np.array([b for b, _ in problems], np.int32),
                class_of=np.array([c for _, c in problems], np.int32), normals_in=normals_in), models


def set_normals(lib, normals_in):
    """the normals buffer of the library from given normals (a list like the models) -> (buffer, f32 [total,3] as prepared)"""
    flat = np.ascontiguousarray(np.concatenate(normals_in), np.float32)
    nb = lib.ffb6d_icp_normals_bytes(len(flat))
    buf = np.full(nb, 0x55, np.uint8)
    assert lib.ffb6d_icp_set_normals(_p(flat), len(flat), _p(buf), nb, None) == 0, lib.ffb6d_last_error()
    return buf, buf.view(np.float32)[:4 * len(flat)].reshape(-1, 4)


def estimated(lib, models):
    pts = np.ascontiguousarray(np.concatenate(models), np.float32)
    begin = np.concatenate([[0], np.cumsum([len(m) for m in models])]).astype(np.int64)
    nb = lib.ffb6d_icp_normals_bytes(len(pts))
    buf = np.full(nb, 0x55, np.uint8)
    rc = lib.ffb6d_icp_estimate_normals_f32(_p(pts), _p(begin), len(models), len(pts), _p(buf), nb, None)
    assert rc == 0, lib.ffb6d_last_error()
    return buf.view(np.float32)[:4 * len(pts)].reshape(-1, 4), begin


def refine_plane(lib, buf, nbuf, n_cls, total, case, max_iter, max_dist, tol=0.0, min_pairs=3, min_eig=MIN_EIG, T0=None):
    T0 = case["T"] if T0 is None else T0
    P, (B, N) = len(case["frame_of"]), case["mask"].shape
    wbytes = lib.ffb6d_icp_plane_workspace_bytes(P, N)
    ws = np.full(wbytes, 0x55, np.uint8)
    T, n_pairs = np.full((P, 3, 4), 7.0), np.full(P, 7, np.int32)
    rms, rms_plane, iters = np.full(P, 7, np.float32), np.full(P, 7, np.float32), np.full(P, 7, np.int32)
    rc = lib.ffb6d_icp_refine_plane_f32(_p(buf), _p(nbuf), n_cls, total, _p(case["pcld"]), _p(case["mask"]), 64, None, _p(case["frame_of"]),
                                        _p(case["class_of"]), _p(T0), P, B, N, N, max_dist, max_iter, tol, min_pairs, min_eig, _p(T),
                                        _p(n_pairs), _p(rms), _p(rms_plane), _p(iters), _p(ws), wbytes, None)
    assert rc == 0, lib.ffb6d_last_error()
    return T, dict(n_pairs=n_pairs, rms=rms, rms_plane=rms_plane, iters=iters)


def refine_point(lib, buf, n_cls, total, case, max_iter, max_dist, tol=0.0):
    P, (B, N) = len(case["frame_of"]), case["mask"].shape
    wbytes = lib.ffb6d_icp_workspace_bytes(P, N)
    ws = np.full(wbytes, 0x55, np.uint8)
    T, n_pairs, rms, iters = np.full((P, 3, 4), 7.0), np.full(P, 7, np.int32), np.full(P, 7, np.float32), np.full(P, 7, np.int32)
    rc = lib.ffb6d_icp_refine_f32(_p(buf), n_cls, total, _p(case["pcld"]), _p(case["mask"]), 64, None, _p(case["frame_of"]),
                                  _p(case["class_of"]), _p(case["T"]), P, B, N, N, max_dist, max_iter, tol, 3, _p(T), _p(n_pairs), _p(rms),
                                  _p(iters), _p(ws), wbytes, None)
    assert rc == 0, lib.ffb6d_last_error()
    return T, dict(n_pairs=n_pairs, rms=rms, iters=iters)


def refine_plane_inst(lib, buf, nbuf, n_cls, total, case, mode, max_iter, max_dist, tol=0.0, sel=None, min_eig=MIN_EIG):
    sel = slice(None) if sel is None else sel
    frame_of, class_of, inst_of = (np.ascontiguousarray(case[k][sel]) for k in ("frame_of", "class_of", "inst_of"))
    T0 = np.ascontiguousarray(case["T"][sel])
    mask = case["mask"]
    P, (B, N) = len(frame_of), mask.shape
    wbytes = lib.ffb6d_icp_plane_inst_workspace_bytes(P, N, MODE[mode])
    ws = np.full(wbytes, 0x55, np.uint8)
    T, n_pairs, iters = np.full((P, 3, 4), 7.0), np.full(P, 7, np.int32), np.full(P, 7, np.int32)
    rms, rms_plane = np.full(P, 7, np.float32), np.full(P, 7, np.float32)
    out = np.full((B, N), 7, np.uint8)
    rc = lib.ffb6d_icp_refine_plane_inst_f32(_p(buf), _p(nbuf), n_cls, total, _p(case["pcld"]), _p(mask), 8 * mask.itemsize, None,
                                             _p(case["inst"]), _p(frame_of), _p(class_of), _p(inst_of), _p(T0), P, B, N, N, max_dist, max_iter,
                                             tol, 3, min_eig, MODE[mode], _p(T), _p(n_pairs), _p(rms), _p(rms_plane), _p(iters), _p(out),
                                             _p(ws), wbytes, None)
    assert rc == 0, lib.ffb6d_last_error()
    return T, dict(n_pairs=n_pairs, rms=rms, rms_plane=rms_plane, iters=iters, inst=out)


def assert_clear_of_the_truncation_edge(eig, min_eig=MIN_EIG):
    """no eigenvalue ratio of any update of the restatement within a decade of min_eig: no truncation decision on a rounding edge"""
    for per_problem in eig:
        r = pref.eig_ratios(per_problem)
        assert not np.any((r >= min_eig / 10) & (r <= 10 * min_eig)), r


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ---- normals -----------------------------------------------------------------------------------------------------------------
def test_estimated_normals_match_the_restatement(emu):
    case, models = plane_case()
    got, begin = estimated(emu, models)
    assert not got[:, 3].any()
    decided = 0
    for c, m in enumerate(models):
        want, spectrum = pref.estimate_normals(m)
        n = got[begin[c]:begin[c + 1], :3]
        if len(m) < 3:
            assert not n.any()                                                    # fewer than three points: the zero vector
            continue
        clear = (spectrum[:, 1] - spectrum[:, 0]) > 1e-6 * spectrum[:, 2]
        assert clear.sum() >= 0.9 * len(m)
        decided += int(clear.sum())
        dots = np.einsum("ij,ij->i", unit(n[clear]), unit(want[clear]))
        assert np.all(dots >= 1 - 1e-12), (c, dots.min())                        # the direction AND the sign
        big = np.abs(n[clear]).argmax(axis=1)
        assert np.all(n[clear][np.arange(len(big)), big] > 0)
        assert np.all(np.abs(np.linalg.norm(n[clear].astype(np.float64), axis=1) - 1) <= 2e-7)
    assert decided > 200
    grid = got[begin[4]:begin[5], :3]
    assert np.array_equal(grid, np.tile(np.float32([0, 0, 1]), (18, 1)))          # the planar grid: exactly its normal


def test_a_spheres_estimated_normals_are_radial(emu):
    """The 16 neighbours of a point lie within a cap about it; the normal of the plane fitted to them is held to the cap's own
    angular radius from the radial direction (computed here from the neighbour sets, not from the code under test)."""
    pts, radial = pref.sphere_cloud(3, 600)
    got, _ = estimated(emu, [pts])
    nb = pref.neighbours(pts, 16)
    cap = np.einsum("ijk,ik->ij", unit(pts[nb]), unit(pts)).min(axis=1)           # cos of the farthest neighbour's angle
    dots = np.abs(np.einsum("ij,ij->i", unit(got[:, :3]), unit(radial)))
    assert np.all(dots >= cap) and np.median(dots) > 0.999, (dots.min(), cap.min())


def test_given_normals_are_normalised_once_and_bad_ones_become_zero(emu):
    case, _ = plane_case()
    _, got = set_normals(emu, case["normals_in"])
    want = pref.given_normals(np.concatenate(case["normals_in"]))
    assert np.array_equal(got[:, :3].view(np.uint32), want.view(np.uint32)) and not got[:, 3].any()
    b2 = 130
    assert not got[b2 + 3, :3].any() and not got[b2 + 17, :3].any() and not got[b2 + 40, :3].any()
    assert abs(np.linalg.norm(got[b2 + 5, :3].astype(np.float64)) - 1) <= 2e-7
    assert not got[-2:, :3].any()                                                 # the class of two points has no normals


# ---- the loop ------------------------------------------------------------------------------------------------------------------
def test_plane_loop_on_the_emulator_matches_the_restatement(emu):
    lib = emu
    case, models = plane_case()
    buf, n_cls, total = prepare(lib, models)
    nbuf, prepared = set_normals(lib, case["normals_in"])
    begin = np.concatenate([[0], np.cumsum([len(m) for m in models])])
    normals = [prepared[begin[c]:begin[c + 1], :3] for c in range(len(models))]
    point_before, got = {}, {}
    for form in (0, 1):
        lib.ffb6d_icp_set_form(form)
        point_before[form] = refine_point(lib, buf, n_cls, total, case, 6, 0.006)
    for form in (0, 1):
        lib.ffb6d_icp_set_form(form)
        for tol in (0.0, 2e-4):
            T, st = refine_plane(lib, buf, nbuf, n_cls, total, case, 6, 0.006, tol)
            wT, wst = pref.icp_refine_plane(case["pcld"], case["mask"], case["T"], case["frame_of"], case["class_of"], models, normals, 6,
                                            0.006, tol, 3, MIN_EIG)
            assert_clear_of_the_truncation_edge(wst["eig"])
            assert np.array_equal(st["n_pairs"], wst["n_pairs"]) and np.array_equal(st["iters"], wst["iters"]), (form, tol, st, wst)
            assert np.abs(T - wT).max() <= 2e-5, (form, tol, np.abs(T - wT).reshape(len(T), -1).max(axis=1))
            assert np.all(np.abs(st["rms"] - wst["rms"]) <= 1e-6 * wst["rms"])
            assert np.all(np.abs(st["rms_plane"] - wst["rms_plane"]) <= 1e-6 * wst["rms_plane"])
            assert list(st["n_pairs"]) == [wst["n_pairs"][0], wst["n_pairs"][1], 4, 0, 1, wst["n_pairs"][5], 0, 0]
            assert list(st["iters"][3:5]) == [0, 0] and list(st["iters"][6:]) == [0, 0]
            for p in (3, 4, 6, 7):                                                # degenerate problems: the input poses as bits
                assert np.array_equal(T[p].view(np.uint64), case["T"][p].view(np.uint64))
            assert st["iters"][0] >= 1 and st["iters"][2] >= 1 and st["iters"][5] >= 1 and (tol == 0.0) == (st["iters"][0] == 6)
            assert st["rms_plane"][4] > 0 or st["n_pairs"][4] == 0 or not np.any(normals[5])      # (two points: zero normals, r = 0)
            got[form, tol] = (T.copy(), {k: v.copy() for k, v in st.items()})
    for tol in (0.0, 2e-4):                                                       # the two forms of the search: the same bits
        assert np.array_equal(got[0, tol][0].view(np.uint64), got[1, tol][0].view(np.uint64))
        for k in ("rms", "rms_plane"):
            assert np.array_equal(got[0, tol][1][k].view(np.uint32), got[1, tol][1][k].view(np.uint32))
    # the grid (exact normal, zero rows): three directions truncated, its in-plane pose untouched, the residual gone
    wst = pref.icp_refine_plane(case["pcld"], case["mask"], case["T"], case["frame_of"], case["class_of"], models, normals, 6, 0.006)[1]
    lam, used = wst["eig"][2][0]
    assert used.sum() == 3 and np.all(lam[~used] <= 1e-12 * lam.max())
    Tg = got[0, 0.0][0][2]
    c, _ = pref.class_constants(models[4])
    assert got[0, 0.0][1]["rms_plane"][2] <= 1e-6
    assert np.abs(pref.in_plane_motion(case["T"][2], Tg, c)).max() <= 1e-6
    # the point calls after the plane calls: the bits they gave before
    for form in (0, 1):
        lib.ffb6d_icp_set_form(form)
        T, st = refine_point(lib, buf, n_cls, total, case, 6, 0.006)
        assert np.array_equal(T.view(np.uint64), point_before[form][0].view(np.uint64))
        for k in ("n_pairs", "rms", "iters"):
            assert np.array_equal(st[k].view(np.uint32), point_before[form][1][k].view(np.uint32))


def test_the_first_iteration_keeps_the_pairs_of_the_point_metric(emu):
    """Steps 1-3 are shared: after one iteration the kept pairs and their distances -- n_pairs, and rms, whose sum is made in the
    same order -- are the point call's bits; so is the instance map the two metrics write from the kept pairs."""
    lib = emu
    case, models = plane_case()
    buf, n_cls, total = prepare(lib, models)
    nbuf, prepared = set_normals(lib, case["normals_in"])
    begin = np.concatenate([[0], np.cumsum([len(m) for m in models])])
    P, (B, N) = len(case["frame_of"]), case["mask"].shape
    for form in (0, 1):
        lib.ffb6d_icp_set_form(form)
        _, pt = refine_point(lib, buf, n_cls, total, case, 1, 0.006)
        _, pl = refine_plane(lib, buf, nbuf, n_cls, total, case, 1, 0.006)
        assert np.array_equal(pt["n_pairs"], pl["n_pairs"]) and np.array_equal(pt["rms"].view(np.uint32), pl["rms"].view(np.uint32))
        # per point: the plane call returns no idx / d2 rows, so the rows of the point metric's single step (pinned to the restatement
        # as bits by tests/test_refine_emu_cpu.py) go through step 4p here; a pair the plane call matched to another model point
        # would read another normal and another m, and rms_plane would show it
        idx, d2, counts = np.full((P, N), 7, np.int32), np.full((P, N), 7, np.float32), np.full(P, 7, np.int32)
        wbytes = lib.ffb6d_icp_workspace_bytes(P, N)
        ws = np.zeros(wbytes, np.uint8)
        rc = lib.ffb6d_icp_correspond_f32(_p(buf), n_cls, total, _p(case["pcld"]), _p(case["mask"]), 64, None, _p(case["frame_of"]),
                                          _p(case["class_of"]), _p(case["T"]), P, B, N, N, 0.006, _p(idx), _p(d2), _p(counts), _p(ws), wbytes, None)
        assert rc == 0, lib.ffb6d_last_error()
        checked = 0
        for p in range(P):
            cls = int(case["class_of"][p])
            scene = icp_ref.problem_scene(case["pcld"], case["mask"], int(case["frame_of"][p]), cls)
            kept = idx[p, :len(scene)] >= 0
            assert kept.sum() == pl["n_pairs"][p] and len(scene) == counts[p]
            model = icp_ref.problem_model(models, cls)
            c, rho = pref.class_constants(model)
            if not kept.any() or not rho > 0:
                assert pl["rms_plane"][p] == 0
                continue
            at = idx[p, :len(scene)][kept]
            q = icp_ref.to_model_frame(scene[kept], case["T"][p], np.float32)
            rr = pref.plane_system(q, model[at], prepared[begin[cls]:begin[cls + 1], :3][at], c, rho)[2]
            want = np.sqrt(rho * rho * rr / kept.sum())
            assert abs(pl["rms_plane"][p] - want) <= 1e-6 * want, (form, p, pl["rms_plane"][p], want)
            assert abs(pl["rms"][p] - np.sqrt(d2[p, :len(scene)][kept].astype(np.float64).sum() / kept.sum())) <= 1e-6 * pl["rms"][p]
            checked += 1
        assert checked >= 4
    icase, imodels = iref.instances_case(192)
    ibuf, in_cls, itotal = prepare(lib, imodels)
    inb, _ = set_normals(lib, [pref.estimate_normals(m)[0] for m in imodels])
    for mode in ("map", "nearest"):
        _, pt = refine_inst(lib, ibuf, in_cls, itotal, icase, mode, 1, 0.006)
        _, pl = refine_plane_inst(lib, ibuf, inb, in_cls, itotal, icase, mode, 1, 0.006)
        assert np.array_equal(pt["inst"], pl["inst"]) and np.array_equal(pt["n_pairs"], pl["n_pairs"])
        assert np.array_equal(pt["rms"].view(np.uint32), pl["rms"].view(np.uint32))


def test_max_iter_zero_and_refusals(emu):
    lib = emu
    case, models = plane_case()
    buf, n_cls, total = prepare(lib, models)
    nbuf, _ = set_normals(lib, case["normals_in"])
    T, st = refine_plane(lib, buf, nbuf, n_cls, total, case, 0, 0.006)
    assert np.array_equal(T.view(np.uint64), case["T"].view(np.uint64))
    assert not st["n_pairs"].any() and not st["iters"].any() and not st["rms"].any() and not st["rms_plane"].any()
    P, (B, N) = len(case["frame_of"]), case["mask"].shape
    wbytes = lib.ffb6d_icp_plane_workspace_bytes(P, N)
    assert wbytes > lib.ffb6d_icp_workspace_bytes(P, N) and lib.ffb6d_icp_plane_workspace_bytes(0, N) == 0
    assert lib.ffb6d_icp_plane_inst_workspace_bytes(P, N, 1) > lib.ffb6d_icp_inst_workspace_bytes(P, N, 1)
    assert lib.ffb6d_icp_plane_inst_workspace_bytes(P, N, 2) == 0
    ws = np.zeros(wbytes, np.uint8)
    T = np.full((P, 3, 4), 7.0)
    call = lambda nb, min_eig, nbytes: lib.ffb6d_icp_refine_plane_f32(                                              # noqa: E731
        _p(buf), _p(nb), n_cls, total, _p(case["pcld"]), _p(case["mask"]), 64, None, _p(case["frame_of"]), _p(case["class_of"]), _p(case["T"]), P,
        B, N, N, 0.006, 3, 0.0, 3, min_eig, _p(T), None, None, None, None, _p(ws), nbytes, None)
    assert call(None, MIN_EIG, wbytes) != 0 and b"normals" in lib.ffb6d_last_error()
    assert call(nbuf, 1.0, wbytes) != 0 and b"min_eig" in lib.ffb6d_last_error()
    assert call(nbuf, MIN_EIG, lib.ffb6d_icp_workspace_bytes(P, N)) != 0 and b"workspace" in lib.ffb6d_last_error()
    assert np.all(T == 7.0)                                                       # on an error no output is written
    assert call(nbuf, MIN_EIG, wbytes) == 0 and not np.any(T == 7.0)


# ---- the instance calls --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["map", "nearest"])
def test_plane_instance_loop_on_the_emulator_matches_the_restatement(emu, mode):
    lib = emu
    case, models = iref.instances_case(192)
    buf, n_cls, total = prepare(lib, models)
    nbuf, prepared = set_normals(lib, [pref.estimate_normals(m)[0] for m in models])
    begin = np.concatenate([[0], np.cumsum([len(m) for m in models])])
    normals = [prepared[begin[c]:begin[c + 1], :3] for c in range(len(models))]
    args = (case["pcld"], case["mask"], case["inst"], case["T"], case["frame_of"], case["class_of"], case["inst_of"], models, normals)
    got = {}
    for form in (-1, 0):
        lib.ffb6d_icp_set_form(form)
        T, st = refine_plane_inst(lib, buf, nbuf, n_cls, total, case, mode, 4, 0.006, 2e-4)
        got[form] = (T, st)
    for k in ("n_pairs", "rms", "rms_plane", "iters", "inst"):                    # the forms of the search: the same bits
        assert np.array_equal(got[-1][1][k], got[0][1][k])
    assert np.array_equal(got[-1][0].view(np.uint64), got[0][0].view(np.uint64))
    T, st = got[0]
    wT, wst = pref.icp_refine_plane_instances(*args, 4, 0.006, mode, 2e-4, 3, MIN_EIG)
    assert_clear_of_the_truncation_edge(wst["eig"])
    tie = None
    excused = []
    for p in range(len(T)):
        ok = np.abs(T[p] - wT[p]).max() <= 2e-5 and st["n_pairs"][p] == wst["n_pairs"][p] and st["iters"][p] == wst["iters"][p] \
            and abs(st["rms"][p] - wst["rms"][p]) <= 1e-6 * wst["rms"][p] \
            and abs(st["rms_plane"][p] - wst["rms_plane"][p]) <= 1e-6 * wst["rms_plane"][p]
        if not ok:
            tie = tie or pref.first_divergence_instances(*args, 4, 0.006, mode, 2e-4, 3, MIN_EIG)
            assert tie[p] is not None, (p, np.abs(T[p] - wT[p]).max(), st["n_pairs"][p], wst["n_pairs"][p], st["iters"][p], wst["iters"][p])
            excused.append(p)
    assert len(excused) <= len(T) // 10, excused
    decided = wst["writers"] <= 1
    if not excused:
        assert np.array_equal(st["inst"][decided], wst["inst"][decided])
    assert st["iters"][[0, 1, 3, 4, 5]].min() >= 1 and not st["iters"][11:].any()
    for p in (7, 9, 10, 11, 12) if mode == "map" else (11, 12):                   # no pairs: the input poses as bits
        assert np.array_equal(T[p].view(np.uint64), case["T"][p].view(np.uint64))


def test_a_nearest_problem_alone_in_its_group_gives_the_class_calls_bits(emu):
    lib = emu
    case, models = iref.instances_case(192)
    buf, n_cls, total = prepare(lib, models)
    nbuf, _ = set_normals(lib, [pref.estimate_normals(m)[0] for m in models])
    sel = slice(5, 6)                                                             # class 2 in frame 1, alone
    T, st = refine_plane_inst(lib, buf, nbuf, n_cls, total, case, "nearest", 4, 0.006, 0.0, sel=sel)
    one = dict(case, frame_of=case["frame_of"][sel], class_of=case["class_of"][sel], T=np.ascontiguousarray(case["T"][sel]))
    cT, cst = refine_plane(lib, buf, nbuf, n_cls, total, one, 4, 0.006)
    assert st["iters"][0] == 4 and np.array_equal(T.view(np.uint64), cT.view(np.uint64))
    for k in ("n_pairs", "rms", "rms_plane", "iters"):
        assert np.array_equal(st[k].view(np.uint32), cst[k].view(np.uint32))
