"""csrc/icp.hip on the SIMT emulator (tests/simt), without a GPU: the unmodified kernel source compiled for the host, run through
the C ABI of include/ffb6d_refine.h on tiny ragged problems and held against the numpy restatement (tests/icp_ref.py) -- the
correspondences as bits in both forms of the search, the loop within the bar of the device test, degenerate problems as bits."""
import numpy as np
import pytest

import icp_ref
from ffb6d_amd import synth
from tests.simt.build import load, ptr as _p

INF = float("inf")


@pytest.fixture(scope="module")
def emu_icp():
    """the emulated library (tests/simt/build.py)"""
    return load()


def tiny_case():
    """Classes of 130 / 70 / 0 / 18 (grid with duplicated rows) points, two frames of 192 points, six problems: two objects in
    frame 0, the grid, the empty class (with scene points), an empty scene set, a frame that is no index."""
    rng = np.random.RandomState(5)
    g = np.arange(4) / 64.0
    grid = np.array([[x, y, 0.0] for x in g for y in g] + [[g[0], g[3], 0.0], [g[2], g[2], 0.0]], np.float32)
    models = icp_ref.models_of([None, icp_ref.surface_model(1, 130), icp_ref.surface_model(2, 70), None, grid])
    B, N = 2, 192
    pcld = (rng.rand(B, N, 3) * [2.0, 1.2, 1.0] + [-1.0, -0.6, 0.6]).astype(np.float32)
    mask = np.zeros((B, N), np.int64)
    problems = [(0, 1), (0, 2), (1, 4), (1, 3), (1, 2), (7, 1)]
    T = np.zeros((len(problems), 3, 4))
    for p, (b, cls) in enumerate(problems):
        pred, gt = synth.eval_pose_pair(60 + p, "near")
        T[p] = pred
        if p < 2:
            n = (70, 40)[p]
            m = models[cls]
            d = 0.3 * (gt.astype(np.float64) - pred) + pred                       # a pose a little off the problem's own
            scene = (m[rng.randint(0, len(m), n)].astype(np.float64) @ d[:, :3].T + d[:, 3] + 0.001 * rng.randn(n, 3)).astype(np.float32)
            at = np.sort(rng.choice(np.flatnonzero(mask[b] == 0), n, replace=False))
            pcld[b, at], mask[b, at] = scene, cls
    T[2, :, :3], T[2, :, 3] = np.eye(3), [0.0, 0.0, 1.0]
    at = np.flatnonzero(mask[1] == 0)[:4]
    pcld[1, at] = [[1 / 128.0, 0.0, 1.0], [g[0], g[3], 1.0], [g[2], g[2], 1.0], [0.5, 0.5, 1.0]]
    mask[1, at] = 4
    mask[1, np.flatnonzero(mask[1] == 0)[:9]] = 3
    pcld[0, np.flatnonzero(mask[0] == 1)[:3]] = np.nan                            # NaN scene points of problem 0
    return dict(pcld=pcld, mask=mask, T=T, frame_of=np.array([b for b, _ in problems], np.int32),
                class_of=np.array([c for _, c in problems], np.int32)), models


def prepare(lib, models):
    pts = np.ascontiguousarray(np.concatenate(models), np.float32)
    begin = np.concatenate([[0], np.cumsum([len(m) for m in models])]).astype(np.int64)
    nbytes = lib.ffb6d_icp_prepared_bytes(len(pts), len(models))
    buf = np.zeros(nbytes, np.uint8)
    assert lib.ffb6d_icp_prepare(_p(pts), _p(begin), len(models), len(pts), _p(buf), nbytes, None) == 0, lib.ffb6d_last_error()
    return buf, len(models), len(pts)


def _canon(x):
    x = np.array(x, np.float32)
    x[np.isnan(x)] = np.nan
    return x.view(np.uint32)


@pytest.mark.parametrize("mask_dtype", [np.int64, np.int32])
def test_correspondences_on_the_emulator_equal_the_restatement_as_bits(emu_icp, mask_dtype):
    lib = emu_icp
    case, models = tiny_case()
    buf, n_cls, total = prepare(lib, models)
    mask = case["mask"].astype(mask_dtype)
    keep = (np.random.RandomState(2).rand(*mask.shape) < 0.8).astype(np.uint8)
    P, (B, N) = len(case["frame_of"]), mask.shape
    wbytes = lib.ffb6d_icp_workspace_bytes(P, N)
    ws = np.zeros(wbytes, np.uint8)
    pairs = {}
    try:
        for form in (0, 1):
            lib.ffb6d_icp_set_form(form)
            ctr = np.zeros(1, np.uint64)
            lib.ffb6d_icp_set_pair_counter(_p(ctr))
            for max_dist, kp in ((INF, None), (0.004, None), (0.004, keep)):
                idx, d2, counts = np.full((P, N), 7, np.int32), np.full((P, N), 7, np.float32), np.full(P, 7, np.int32)
                rc = lib.ffb6d_icp_correspond_f32(_p(buf), n_cls, total, _p(case["pcld"]), _p(mask), 8 * mask.itemsize,
                                                  _p(kp) if kp is not None else None, _p(case["frame_of"]), _p(case["class_of"]),
                                                  _p(case["T"]), P, B, N, N, max_dist, _p(idx), _p(d2), _p(counts), _p(ws), wbytes, None)
                assert rc == 0, lib.ffb6d_last_error()
                widx, wd2, wcounts = icp_ref.correspondences(case["pcld"], case["mask"], case["T"], case["frame_of"], case["class_of"],
                                                             models, max_dist, keep=kp)
                assert np.array_equal(counts, wcounts) and np.array_equal(idx, widx), (form, max_dist)
                assert np.array_equal(_canon(d2), _canon(wd2)), (form, max_dist)
                if kp is None:
                    assert list(idx[2, :4]) == ([0, 3, 10, 15] if max_dist == INF else [-1, 3, 10, -1])      # ties: the lowest index
                    assert list(wcounts) == [70, 40, 4, 9, 0, 0] and np.isnan(d2[0, :3]).all() and (idx[0, :3] == -1).all()
            pairs[form] = int(ctr[0])
    finally:
        lib.ffb6d_icp_set_pair_counter(None)
        lib.ffb6d_icp_set_form(0)
    assert 0 < pairs[1] < pairs[0]                                                # the pruned form skipped tiles


def test_refine_on_the_emulator_matches_the_restatement(emu_icp):
    lib = emu_icp
    case, models = tiny_case()
    buf, n_cls, total = prepare(lib, models)
    P, (B, N) = len(case["frame_of"]), case["mask"].shape
    wbytes = lib.ffb6d_icp_workspace_bytes(P, N)
    ws = np.zeros(wbytes, np.uint8)
    got = {}
    try:
        for form in (0, 1):
            lib.ffb6d_icp_set_form(form)
            for tol in (0.0, 2e-4):
                T, n_pairs = np.full((P, 3, 4), 7.0), np.full(P, 7, np.int32)
                rms, iters = np.full(P, 7, np.float32), np.full(P, 7, np.int32)
                rc = lib.ffb6d_icp_refine_f32(_p(buf), n_cls, total, _p(case["pcld"]), _p(case["mask"]), 64, None, _p(case["frame_of"]),
                                              _p(case["class_of"]), _p(case["T"]), P, B, N, N, 0.006, 6, tol, 3, _p(T), _p(n_pairs), _p(rms),
                                              _p(iters), _p(ws), wbytes, None)
                assert rc == 0, lib.ffb6d_last_error()
                wT, wst = icp_ref.icp_refine(case["pcld"], case["mask"], case["T"], case["frame_of"], case["class_of"], models, 6, 0.006, tol)
                assert np.array_equal(n_pairs, wst["n_pairs"]) and np.array_equal(iters, wst["iters"]), (form, tol, n_pairs, iters, wst)
                assert np.abs(T[:2] - wT[:2]).max() <= 2e-5 and np.all(np.abs(rms - wst["rms"]) <= 1e-6 * wst["rms"])
                assert list(iters[2:]) == [0, 0, 0, 0] and list(n_pairs[2:]) == [2, 0, 0, 0]      # grid: 2 pairs < min_pairs; empty ones
                assert np.array_equal(T[2:].view(np.uint64), case["T"][2:].view(np.uint64))       # input poses as bits
                assert iters[0] >= 1 and (tol == 0.0) == (iters[0] == 6)
                got[form, tol] = (T.copy(), rms.copy())
    finally:
        lib.ffb6d_icp_set_form(0)
    for tol in (0.0, 2e-4):                                                       # the two forms: the same bits
        assert np.array_equal(got[0, tol][0].view(np.uint64), got[1, tol][0].view(np.uint64))
        assert np.array_equal(got[0, tol][1].view(np.uint32), got[1, tol][1].view(np.uint32))
