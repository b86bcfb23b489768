"""Pose evaluation without a GPU (ffb6d_amd/evaluate.py, csrc/pose_eval.hip): the AUC arithmetic against the reference's
own results (tests/golden/eval_small.npz, make_golden_eval.py) bit for bit, the workspace formula of include/ffb6d_eval.h,
and the ADD / ADD-S kernel itself run through the SIMT emulator (tests/simt) on small cases against a float64 restatement."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN
from ffb6d_amd import evaluate
from tests.simt.build import load

spec = importlib.util.spec_from_file_location("make_golden_eval", os.path.join(GOLDEN, "make_golden_eval.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "eval_small.npz"))


def test_cal_auc_equals_the_reference_bit_for_bit(golden):
    for i, lst in enumerate(gen.auc_lists()):
        got = evaluate.cal_auc(lst)
        assert got == golden[f"auc{i}"], (i, got, golden[f"auc{i}"])
    assert evaluate.cal_auc([]) == 0


def test_vocap_quirks():
    # distances beyond the threshold are dropped; the curve closes at 0.1 with the last accuracy
    rec = np.array([0.02, 0.04, np.inf])
    prec = np.array([1 / 3, 2 / 3, 1.0], np.float32)
    want = (0.02 * np.float64(np.float32(1 / 3)) + 0.02 * np.float64(np.float32(2 / 3)) + 0.06 * np.float64(np.float32(2 / 3))) * 10
    assert abs(evaluate.VOCap(rec, prec) - want) < 1e-12
    assert evaluate.VOCap(np.array([np.inf]), np.array([1.0], np.float32)) == 0


def _filled_eval():
    te = evaluate.TorchEval(n_cls=gen.N_CLS)
    te.cls_add_dis, te.cls_adds_dis, te.pred_kp_errs = gen.te_lists()
    return te


def test_torcheval_cal_auc_equals_the_reference(golden, tmp_path):
    te = _filled_eval()
    res = te.cal_auc(save_dir=str(tmp_path))
    for k in gen.TE_KEYS:
        assert np.array_equal(np.asarray(res[k], np.float64), golden[f"te_{k}"]), k
    assert [res["mean_add_auc"], res["mean_adds_auc"], res["mean_add_s_auc"]] == list(golden["te_means"])
    # the reference prints a float32 (its kp errors are float32 numpy scalars); the shortest repr read back is that value
    assert res["mean_kp_err"] == np.float32(golden["te_mean_kp_err"])
    # ADD(-S) is ADD-S exactly on the symmetric ids
    for c in range(1, gen.N_CLS):
        want = res["adds_auc_lst"][c] if c in evaluate.YCB_SYM_CLS_IDS else res["add_auc_lst"][c]
        assert res["add_s_auc_lst"][c] == want
    assert len(os.listdir(tmp_path)) == 2
    # a second summary does not count class 0 twice (the reference's would)
    again = te.cal_auc()
    for k in gen.TE_KEYS:
        assert np.array_equal(np.asarray(again[k]), np.asarray(res[k])), k


def test_cal_lm_add_uses_a_tenth_of_the_diameter():
    rng = np.random.RandomState(3)
    te = evaluate.TorchEval(n_cls=16, sym_cls_ids=evaluate.LM_SYM_CLS_IDS)
    for obj in (4, 10):
        for _ in range(50):
            a = float(np.float32(0.03 * rng.rand()))
            s = float(np.float32(a * rng.rand()))
            for lst, v in ((te.cls_add_dis, a), (te.cls_adds_dis, s)):
                lst[obj].append(v)
                lst[0].append(v)
    for obj, diameter in ((4, 102.1), (10, 164.6)):
        res = te.cal_lm_add(obj, diameter)
        d = diameter / 1000.0 * 0.1                              # pvn3d_eval_utils_kpls.py:420-422, restated
        assert res["add"] == np.mean(np.array(te.cls_add_dis[obj]) < d) * 100
        assert res["adds"] == np.mean(np.array(te.cls_adds_dis[obj]) < d) * 100
        assert res["add_auc_lst"] == [evaluate.cal_auc(te.cls_add_dis[obj])]
        sym = te.cls_adds_dis[obj] if obj in evaluate.LM_SYM_CLS_IDS else te.cls_add_dis[obj]
        assert res["add_s_auc_lst"] == [evaluate.cal_auc(sym)]
        assert 0 < res["adds"] <= 100 and res["adds"] >= res["add"]


def test_workspace_formula(native_lib):
    for Q, n in ((1, 1), (3, 100), (40, 2620), (7, 16384)):
        assert native_lib.ffb6d_pose_add_adds_workspace_bytes(Q, n) == 36 * Q * n
    for Q, n in ((0, 100), (5, 0), (-1, 10), (4, -3)):
        assert native_lib.ffb6d_pose_add_adds_workspace_bytes(Q, n) == 0


# ---- the kernel on the SIMT emulator ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu_eval():
    """the emulated library (tests/simt/build.py)"""
    return load()


def ref_add_adds(p, pred, gt):
    """float64 restatement of basic_utils.py:651-669 (the poses' float32 values, exactly)."""
    p = p.astype(np.float64)
    pd = p @ pred[:, :3].astype(np.float64).T + pred[:, 3]
    g = p @ gt[:, :3].astype(np.float64).T + gt[:, 3]
    if len(p) == 0:
        return np.nan, np.nan
    add = np.linalg.norm(pd - g, axis=1).mean()
    mins = np.concatenate([np.sqrt(((g[i:i + 512, None] - pd[None]) ** 2).sum(-1)).min(1) for i in range(0, len(p), 512)])
    return add, mins.mean()


def _ptr(a):
    return a.ctypes.data


def run_emulated(lib, models, cls, pred, gt, ws_bytes=None, out=None):
    sizes = [len(m) for m in models]
    pts = np.ascontiguousarray(np.concatenate(models), np.float32).reshape(-1, 3)
    begin = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cls = np.asarray(cls, np.int32)
    pred, gt = np.ascontiguousarray(pred, np.float32), np.ascontiguousarray(gt, np.float32)
    Q = len(cls)
    need = lib.ffb6d_pose_add_adds_workspace_bytes(Q, max(sizes))
    ws = np.zeros(max(need, 1), np.uint8)
    add, adds = out if out is not None else (np.zeros(Q, np.float32), np.zeros(Q, np.float32))
    rc = lib.ffb6d_pose_add_adds_f32(_ptr(pts), _ptr(begin), len(models), _ptr(cls), _ptr(pred), _ptr(gt), Q, _ptr(add),
                                     _ptr(adds), _ptr(ws), need if ws_bytes is None else ws_bytes, None)
    return rc, add, adds


def test_kernel_on_the_emulator_matches_float64(emu_eval):
    from ffb6d_amd import synth
    models = [synth.model_cloud(900 + c, n) for c, n in enumerate((1, 63, 300, 0, 257))]
    rows = [(0, "near"), (1, "near"), (2, "far"), (2, "zero"), (1, "same"), (4, "near"), (3, "near"), (2, "near")]
    cls = [c for c, _ in rows]
    pairs = [synth.eval_pose_pair(950 + k, kind) for k, (_, kind) in enumerate(rows)]
    pred, gt = np.stack([p for p, _ in pairs]), np.stack([g for _, g in pairs])
    rc, add, adds = run_emulated(emu_eval, models, cls, pred, gt)
    assert rc == 0, emu_eval.ffb6d_last_error()
    for q, c in enumerate(cls):
        want_add, want_adds = ref_add_adds(models[c], pred[q], gt[q])
        if len(models[c]) == 0:
            assert np.isnan(add[q]) and np.isnan(adds[q])
            continue
        assert abs(add[q] - want_add) <= 1e-6 + 1e-6 * want_add, (q, add[q], want_add)
        assert abs(adds[q] - want_adds) <= 1e-6 + 1e-6 * want_adds, (q, adds[q], want_adds)
        assert adds[q] <= add[q]
    assert add[4] == 0 and adds[4] == 0                  # identical poses
    # one row alone gives the bits it gets inside the batch
    rc, add1, adds1 = run_emulated(emu_eval, models, cls[2:3], pred[2:3], gt[2:3])
    assert rc == 0 and add1[0] == add[2] and adds1[0] == adds[2]


def test_kernel_on_the_emulator_rejects_bad_arguments(emu_eval):
    from ffb6d_amd import synth
    models = [synth.model_cloud(990, 40), synth.model_cloud(991, 70)]
    pred, gt = synth.eval_pose_pair(992)
    sentinel = (np.full(2, 7.0, np.float32), np.full(2, 7.0, np.float32))
    rc, add, adds = run_emulated(emu_eval, models, [1, 2], np.stack([pred, pred]), np.stack([gt, gt]), out=sentinel)
    assert rc != 0 and "class_of[1]" in emu_eval.ffb6d_last_error().decode()
    assert np.all(add == 7.0) and np.all(adds == 7.0)
    rc, add, adds = run_emulated(emu_eval, models, [0, 1], np.stack([pred, pred]), np.stack([gt, gt]),
                                 ws_bytes=36 * 2 * 70 - 4, out=sentinel)
    assert rc != 0 and "workspace" in emu_eval.ffb6d_last_error().decode()
    assert np.all(add == 7.0) and np.all(adds == 7.0)
