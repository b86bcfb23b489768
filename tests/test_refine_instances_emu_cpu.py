"""The instance calls of csrc/icp.hip on the SIMT emulator (tests/simt), without a GPU: ffb6d_icp_correspond_inst_f32 and
ffb6d_icp_refine_inst_f32 through the C ABI on the tiny ragged case of tests/icp_inst_ref.py (`instances_case`), held against the
numpy restatement -- the single step as bits in both modes and all forms of the search, the loop within the bar of the device
test, the anchors to the class calls as bits, degenerate problems as bits."""
import numpy as np
import pytest

import icp_inst_ref as iref
from test_refine_emu_cpu import _canon, _p, prepare
from tests.simt.build import load

INF = float("inf")
MODE = {"map": 0, "nearest": 1}


@pytest.fixture(scope="module")
def emu():
    """the emulated library (tests/simt/build.py); the search form is back at its default when the module is over"""
    lib = load()
    yield lib
    lib.ffb6d_icp_set_form(0)


def correspond_inst(lib, buf, n_cls, total, case, mode, max_dist, keep=None, inst="case", T=None, sel=None):
    sel = slice(None) if sel is None else sel
    frame_of, class_of, inst_of = (np.ascontiguousarray(case[k][sel]) for k in ("frame_of", "class_of", "inst_of"))
    T = np.ascontiguousarray(case["T"][sel] if T is None else T)
    mask = case["mask"]
    P, (B, N) = len(frame_of), mask.shape
    wbytes = lib.ffb6d_icp_inst_workspace_bytes(P, N, MODE[mode])
    ws = np.zeros(wbytes, np.uint8)
    idx, d2, counts, owner = np.full((P, N), 7, np.int32), np.full((P, N), 7, np.float32), np.full(P, 7, np.int32), np.full((P, N), 7, np.int32)
    imap = case["inst"] if isinstance(inst, str) else inst
    rc = lib.ffb6d_icp_correspond_inst_f32(_p(buf), n_cls, total, _p(case["pcld"]), _p(mask), 8 * mask.itemsize,
                                           _p(keep) if keep is not None else None, _p(imap) if imap is not None else None, _p(frame_of),
                                           _p(class_of), _p(inst_of), _p(T), P, B, N, N, max_dist, MODE[mode], _p(idx), _p(d2), _p(counts),
                                           _p(owner), _p(ws), wbytes, None)
    assert rc == 0, lib.ffb6d_last_error()
    return idx, d2, counts, owner


def refine_inst(lib, buf, n_cls, total, case, mode, max_iter, max_dist, tol=0.0, keep=None, inst="case", sel=None, T0=None):
    sel = slice(None) if sel is None else sel
    frame_of, class_of, inst_of = (np.ascontiguousarray(case[k][sel]) for k in ("frame_of", "class_of", "inst_of"))
    T0 = np.ascontiguousarray(case["T"][sel] if T0 is None else T0)
    mask = case["mask"]
    P, (B, N) = len(frame_of), mask.shape
    wbytes = lib.ffb6d_icp_inst_workspace_bytes(P, N, MODE[mode])
    ws = np.zeros(wbytes, np.uint8)
    T, n_pairs, rms, iters = np.full((P, 3, 4), 7.0), np.full(P, 7, np.int32), np.full(P, 7, np.float32), np.full(P, 7, np.int32)
    out = np.full((B, N), 7, np.uint8)
    imap = case["inst"] if isinstance(inst, str) else inst
    rc = lib.ffb6d_icp_refine_inst_f32(_p(buf), n_cls, total, _p(case["pcld"]), _p(mask), 8 * mask.itemsize,
                                       _p(keep) if keep is not None else None, _p(imap) if imap is not None else None, _p(frame_of),
                                       _p(class_of), _p(inst_of), _p(T0), P, B, N, N, max_dist, max_iter, tol, 3, MODE[mode], _p(T),
                                       _p(n_pairs), _p(rms), _p(iters), _p(out), _p(ws), wbytes, None)
    assert rc == 0, lib.ffb6d_last_error()
    return T, dict(n_pairs=n_pairs, rms=rms, iters=iters, inst=out)


def judge_loop(got, want, tie):
    """The bar of tests/test_refine_gpu.py::test_loop_matches_the_restatement, per problem; a problem is excused only when the
    float32 and the float64 restatement diverge (in it or, nearest mode, in its group).  -> excused problems"""
    (T, st), (wT, wst) = got, want
    err = np.abs(T - wT).reshape(len(T), -1).max(axis=1)
    excused = []
    for p in range(len(T)):
        ok = err[p] <= 2e-5 and st["n_pairs"][p] == wst["n_pairs"][p] and abs(st["rms"][p] - wst["rms"][p]) <= 1e-6 * wst["rms"][p] \
            and st["iters"][p] == wst["iters"][p]
        if not ok:
            assert tie()[p] is not None, (p, err[p], st["n_pairs"][p], wst["n_pairs"][p], st["rms"][p], wst["rms"][p], st["iters"][p])
            excused.append(p)
    return excused


@pytest.mark.parametrize("N,mask_dtype", [(192, np.int64), (300, np.int32)])
@pytest.mark.parametrize("mode", ["map", "nearest"])
def test_single_step_on_the_emulator_equals_the_restatement_as_bits(emu, N, mask_dtype, mode):
    case, models = iref.instances_case(N, mask_dtype)
    buf, n_cls, total = prepare(emu, models)
    got = {}
    for form in (-1, 0, 1):
        emu.ffb6d_icp_set_form(form)
        for max_dist, kp in ((INF, None), (0.006, None), (0.006, case["keep"])):
            idx, d2, counts, owner = correspond_inst(emu, buf, n_cls, total, case, mode, max_dist, kp)
            widx, wd2, wcounts, wowner = iref.correspondences_instances(case["pcld"], case["mask"], case["inst"], case["T"], case["frame_of"],
                                                                          case["class_of"], case["inst_of"], models, max_dist, mode, kp)
            assert np.array_equal(counts, wcounts) and np.array_equal(idx, widx), (form, max_dist)
            assert np.array_equal(_canon(d2), _canon(wd2)) and np.array_equal(owner, wowner), (form, max_dist)
            got[form, max_dist, kp is None] = (idx, _canon(d2), owner)
            if kp is None and mode == "map":
                assert list(counts) == [64, 65, 7, 30, 25, 40, 65, 0, 5, 0, 0, 0, 8]
                assert np.isnan(d2[0, :3]).all() and (idx[0, :3] == -1).all() and (owner[0, :3] == -1).all()
            if kp is None and mode == "nearest":
                assert list(counts) == [151, 151, 151, 61, 61, 45, 151, 151, 151, 61, 61, 0, 10]
                assert np.array_equal(owner[0], owner[1]) and np.array_equal(owner[0], owner[2]) and np.array_equal(owner[6], owner[8])
                assert set(np.unique(owner[0, :151])) == {-1, 0, 1, 2} and set(np.unique(owner[6, :151])) <= {-1, 6, 7, 8}
                assert (owner[12, :10] == 12).all() and (idx[12] == -1).all()   # no model: +inf owns, nothing is kept
    for key, val in got.items():                                                  # the forms of the search: the same bits
        for a, b in zip(val, got[(0,) + key[1:]]):
            assert np.array_equal(a, b)


def test_an_exact_tie_between_siblings_goes_to_the_lower_row(emu):
    case, models = iref.instances_case(192)
    buf, n_cls, total = prepare(emu, models)
    T = np.stack([case["T"][0], case["T"][0], case["T"][2]])
    idx, d2, counts, owner = correspond_inst(emu, buf, n_cls, total, case, "nearest", INF, T=T, sel=slice(0, 3))
    assert np.array_equal(_canon(d2[0]), _canon(d2[1]))
    assert (owner[:, :151] != 1).all() and (owner[0, :151] == 0).sum() > 60 and (idx[1] == -1).all()
    widx, _, _, wowner = iref.correspondences_instances(case["pcld"], case["mask"], None, T, case["frame_of"][:3], case["class_of"][:3],
                                                           case["inst_of"][:3], models, INF, "nearest")
    assert np.array_equal(idx, widx) and np.array_equal(owner, wowner)


@pytest.mark.parametrize("mode", ["map", "nearest"])
def test_loop_on_the_emulator_matches_the_restatement(emu, mode):
    case, models = iref.instances_case(192)
    buf, n_cls, total = prepare(emu, models)
    args = (case["pcld"], case["mask"], case["inst"], case["T"], case["frame_of"], case["class_of"], case["inst_of"], models)
    got = {}
    for form in (0, 1):
        emu.ffb6d_icp_set_form(form)
        for tol in (0.0, 3e-4):
            T, st = refine_inst(emu, buf, n_cls, total, case, mode, 6, 0.012, tol)
            wT, wst = iref.icp_refine_instances(*args, 6, 0.012, mode, tol)
            excused = judge_loop((T, st), (wT, wst), lambda: iref.first_divergence_instances(*args, 6, 0.012, mode, tol))
            assert len(excused) <= 1
            if not excused:
                decided = wst["writers"] <= 1
                assert np.array_equal(st["inst"][decided], wst["inst"][decided]) and (wst["inst"] > 0).sum() > 100
            for p in (7, 9, 10, 11, 12) if mode == "map" else (11, 12):           # no scene points / no model: the input pose as bits
                assert st["iters"][p] == 0 and st["n_pairs"][p] == 0 and np.array_equal(T[p].view(np.uint64), case["T"][p].view(np.uint64))
            assert st["iters"][0] >= 1 and st["iters"][3] >= 1
            if tol > 0:
                assert (wst["iters"] < 6).any() and (wst["iters"][:6] > 0).all()
            got[form, tol] = (T.copy(), st)
    for tol in (0.0, 3e-4):                                                       # the two forms: the same bits
        a, b = got[0, tol], got[1, tol]
        assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1]["inst"], b[1]["inst"])
        assert np.array_equal(a[1]["rms"].view(np.uint32), b[1]["rms"].view(np.uint32))


def test_anchors_to_the_class_calls_as_bits(emu):
    """map mode with the map 1 on every class point, and nearest mode with singleton groups, are ffb6d_icp_refine_f32; nearest
    mode does not read the map."""
    case, models = iref.instances_case(192)
    buf, n_cls, total = prepare(emu, models)
    sel = np.array([0, 3, 5, 11, 12, 6])                                          # no two adjacent rows share (frame, class)
    frame_of, class_of = np.ascontiguousarray(case["frame_of"][sel]), np.ascontiguousarray(case["class_of"][sel])
    T0 = np.ascontiguousarray(case["T"][sel])
    P, (B, N) = len(sel), case["mask"].shape
    ones = dict(case, inst=(case["mask"] > 0).astype(np.uint8), inst_of=np.ones(len(case["inst_of"]), np.int32))
    for tol in (0.0, 3e-4):
        wbytes = emu.ffb6d_icp_workspace_bytes(P, N)
        ws = np.zeros(wbytes, np.uint8)
        T, n_pairs, rms, iters = np.full((P, 3, 4), 7.0), np.full(P, 7, np.int32), np.full(P, 7, np.float32), np.full(P, 7, np.int32)
        rc = emu.ffb6d_icp_refine_f32(_p(buf), n_cls, total, _p(case["pcld"]), _p(case["mask"]), 64, None, _p(frame_of), _p(class_of), _p(T0),
                                      P, B, N, N, 0.012, 6, tol, 3, _p(T), _p(n_pairs), _p(rms), _p(iters), _p(ws), wbytes, None)
        assert rc == 0, emu.ffb6d_last_error()
        assert iters[0] >= 1 and iters[1] >= 1
        runs = [refine_inst(emu, buf, n_cls, total, ones, "map", 6, 0.012, tol, sel=sel),
                refine_inst(emu, buf, n_cls, total, case, "nearest", 6, 0.012, tol, sel=sel),
                refine_inst(emu, buf, n_cls, total, case, "nearest", 6, 0.012, tol, sel=sel, inst=None)]
        for gT, gst in runs:
            assert np.array_equal(gT.view(np.uint64), T.view(np.uint64)) and np.array_equal(gst["n_pairs"], n_pairs)
            assert np.array_equal(gst["rms"].view(np.uint32), rms.view(np.uint32)) and np.array_equal(gst["iters"], iters)
        assert np.array_equal(runs[1][1]["inst"], runs[2][1]["inst"])


def test_argument_errors_have_their_own_messages(emu):
    case, models = iref.instances_case(192)
    buf, n_cls, total = prepare(emu, models)
    P, (B, N) = len(case["frame_of"]), case["mask"].shape
    wbytes = emu.ffb6d_icp_inst_workspace_bytes(P, N, 0)
    assert wbytes > emu.ffb6d_icp_workspace_bytes(P, N) and emu.ffb6d_icp_inst_workspace_bytes(P, N, 2) == 0
    assert emu.ffb6d_icp_inst_workspace_bytes(0, N, 0) == 0 and emu.ffb6d_icp_inst_workspace_bytes(P, N, 1) == wbytes
    ws = np.zeros(wbytes, np.uint8)
    T, out = np.full((P, 3, 4), 7.0), np.full((B, N), 7, np.uint8)

    def call(P=P, mode=0, inst=case["inst"], wbytes=wbytes):
        return emu.ffb6d_icp_refine_inst_f32(_p(buf), n_cls, total, _p(case["pcld"]), _p(case["mask"]), 64, None,
                                             _p(inst) if inst is not None else None, _p(case["frame_of"]), _p(case["class_of"]),
                                             _p(case["inst_of"]), _p(case["T"]), P, B, N, N, 0.01, 3, 0.0, 3, mode, _p(T), None, None, None,
                                             _p(out), _p(ws), wbytes, None)
    for kw, text in ((dict(mode=2), "mode must be 0 (map) or 1 (nearest)"), (dict(mode=-1), "mode must be"), (dict(inst=None), "needs the instance map"),
                     (dict(P=65536), "at most 65535")):
        assert call(**kw) == -1 and text in emu.ffb6d_last_error().decode(), kw
    assert call(wbytes=wbytes - 1) == -3 and "workspace" in emu.ffb6d_last_error().decode()
    assert (T == 7.0).all() and (out == 7).all()                                 # nothing was launched, nothing written
    assert call(mode=1, inst=None) == 0
