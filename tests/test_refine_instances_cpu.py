"""Instance-aware ICP without a GPU: the library exports the new entry points of include/ffb6d_refine.h and refuses bad arguments
before any HIP call, the class calls' workspace formula is what it was, the Python layer validates and routes, and the numpy
restatement (tests/icp_inst_ref.py) follows the rule the header states."""
import inspect

import numpy as np
import pytest
import torch

import icp_inst_ref as iref

NEW = ("ffb6d_icp_inst_workspace_bytes", "ffb6d_icp_correspond_inst_f32", "ffb6d_icp_refine_inst_f32")
INF = float("inf")


def test_library_exports_the_instance_entry_points(native_lib):
    from ffb6d_amd import _lib
    for name in NEW:
        assert hasattr(native_lib, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["ffb6d_icp_correspond_inst_f32"][1]) == 25 and len(_lib.SIGNATURES["ffb6d_icp_refine_inst_f32"][1]) == 29


def test_sizes_are_host_logic(native_lib):
    a256 = lambda n: (n + 255) // 256 * 256                                      # noqa: E731
    P, stride = 80, 12288
    tiles = stride // 64
    base = a256(16 * P * stride) + a256(4 * P) + a256(8 * 17 * P * tiles) + a256(8 * 12 * P) + a256(16 * P)
    assert native_lib.ffb6d_icp_workspace_bytes(P, stride) == base                # the class calls: unchanged
    want = base + 2 * a256(4 * P * stride) + a256(8 * P)                          # + the idx and d2 rows and the groups
    assert native_lib.ffb6d_icp_inst_workspace_bytes(P, stride, 0) == want == native_lib.ffb6d_icp_inst_workspace_bytes(P, stride, 1)
    for args in ((0, stride, 0), (P, 0, 1), (P, stride, 2), (P, stride, -1)):
        assert native_lib.ffb6d_icp_inst_workspace_bytes(*args) == 0


def test_argument_errors_are_reported_without_a_gpu(native_lib):
    from ffb6d_amd import _lib
    ok = dict(prepared=64, n_cls=3, total=100, pcld=64, mask=64, bits=64, keep=None, inst=64, frame_of=64, class_of=64, inst_of=64, T0=64,
              P=2, B=1, N=128, stride=128, max_dist=INF, max_iter=5, tol=0.0, min_pairs=3, mode=0, T=64, n_pairs=None, rms=None, iters=None,
              inst_out=None, ws=None, ws_bytes=0, stream=None)

    def call(**kw):
        return native_lib.ffb6d_icp_refine_inst_f32(*dict(ok, **kw).values())

    assert call(P=0) == 0
    assert call(mode=2) == -1 and "mode must be 0 (map) or 1 (nearest), got 2" in _lib.last_error()
    assert call(mode=-1) == -1 and "mode must be" in _lib.last_error()
    assert call(inst=None) == -1 and "needs the instance map" in _lib.last_error()
    assert call(P=65536) == -1 and "at most 65535" in _lib.last_error()
    assert call(inst_of=None) == -1 and "inst_of" in _lib.last_error()
    assert call(max_iter=-1) == -1 and "max_iter" in _lib.last_error()
    assert call(bits=16) == -1 and "mask_bits" in _lib.last_error()
    assert call() == -3 and "workspace" in _lib.last_error()                      # too small: reported, nothing launched
    assert call(mode=1, inst=None) == -3 and "workspace" in _lib.last_error()     # nearest mode takes no map
    corr = native_lib.ffb6d_icp_correspond_inst_f32
    head = (64, 3, 100, 64, 64, 64, None)
    tail = (None, None, None, None, None, 0, None)
    assert corr(*head, 64, 64, 64, 64, 64, 0, 1, 128, 128, INF, 0, *tail) == 0
    assert corr(*head, 64, 64, 64, 64, 64, 2, 1, 128, 128, INF, 0, *tail) == -3 and "workspace" in _lib.last_error()
    assert corr(*head, None, 64, 64, 64, 64, 2, 1, 128, 128, INF, 0, *tail) == -1 and "needs the instance map" in _lib.last_error()
    assert corr(*head, 64, 64, 64, 64, 64, 2, 1, 128, 128, INF, 3, *tail) == -1 and "mode must be" in _lib.last_error()
    assert corr(*head, 64, 64, 64, 64, 64, 70000, 1, 128, 128, INF, 1, *tail) == -1 and "at most 65535" in _lib.last_error()


def test_python_layer_validates_and_routes():
    from ffb6d_amd import _lib, pipeline, pose, refine
    prepared = refine.PreparedModels.__new__(refine.PreparedModels)
    prepared.device, prepared.n_cls = torch.device("cpu"), 2
    pcld, mask, inst = torch.zeros(1, 8, 3), torch.zeros(1, 8, dtype=torch.int64), torch.zeros(1, 8, dtype=torch.uint8)
    for fn in (refine.icp_refine_instances, refine.correspondences_instances):
        with pytest.raises(_lib.FFB6DNativeError):                                # no CPU fallback
            fn(pcld, mask, inst, np.zeros((1, 3, 4)), [0], [1], [1], prepared)
        with pytest.raises(ValueError, match="mode"):
            fn(pcld, mask, inst, np.zeros((1, 3, 4)), [0], [1], [1], prepared, mode="votes")
        assert inspect.signature(fn).parameters["mode"].default == "map"
    sig = inspect.signature(pose.solve_instances_refined).parameters
    assert list(sig)[:8] == list(inspect.signature(pose.solve_instances).parameters)[:7] + ["refine"]
    assert sig["refine"].default is None and sig["refine_mask"].default is False and sig["r_lst"].default is None
    assert "unsupported" in inspect.signature(pose.solve_instances).parameters   # solve_instances keeps refusing refine= / refine_mask=
    with pytest.raises(TypeError):
        pose.solve_instances(pcld, mask, pcld, pcld, np.zeros((2, 1, 3)), np.zeros((2, 3)), 2, refine_mask=True)
    net = torch.nn.Linear(1, 1)
    make = lambda **kw: pipeline.SensorToPose(net, np.eye(3), 8, np.zeros((2, 1, 3)), np.zeros((2, 3)), **kw)      # noqa: E731
    assert make(max_instances=2, instance_refine=dict(models=None)).instance_refine == dict(models=None)
    assert make().instance_refine is None
    with pytest.raises(ValueError, match="instance_refine needs max_instances"):
        make(instance_refine=dict())
    with pytest.raises(ValueError):
        make(max_instances=2, refine=dict())


# ---- the restatement follows the rule ------------------------------------------------------------------------------------------
def test_groups_are_runs_of_adjacent_equal_pairs():
    f, c = [0, 0, 0, 1, 1, 0, 0, 2], [1, 1, 2, 2, 2, 1, 1, 1]
    assert iref.groups(f, c) == [(0, 2), (0, 2), (2, 3), (3, 5), (3, 5), (5, 7), (5, 7), (7, 8)]
    assert iref.groups(f, c, "map") == [(p, p + 1) for p in range(8)]


def test_owner_is_the_first_smallest_and_never_a_nan():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    d2 = np.array([[1.0, nan, nan, 2.0, inf, nan], [1.0, 3.0, nan, 1.5, inf, inf], [0.5, 2.0, nan, 1.5, 1.0, nan]], np.float32)
    assert list(iref.owner(d2)) == [2, 2, -1, 1, 2, 1]
    assert list(iref.owner(d2[:1])) == [0, -1, -1, 0, 0, -1]


def test_scene_indices_keeps_its_class_form_and_gains_the_map():
    case, _ = iref.instances_case(192)
    mask, inst = case["mask"], case["inst"]
    all1 = iref.scene_indices(mask, 0, 1)
    assert len(all1) == 151 and np.array_equal(all1, np.flatnonzero(mask[0] == 1))
    parts = [iref.scene_indices(mask, 0, 1, None, inst, k) for k in (1, 2, 3, 255)]
    assert [len(p) for p in parts] == [64, 65, 7, 5] and len(np.unique(np.concatenate(parts))) == 141      # 10 points of instance 0
    for bad in (0, 256, -1):
        assert len(iref.scene_indices(mask, 0, 1, None, inst, bad)) == 0
    assert len(iref.scene_indices(mask, 7, 1, None, inst, 1)) == 0


def test_restatement_of_the_single_step():
    case, models = iref.instances_case(192)
    args = (case["pcld"], case["mask"], case["inst"], case["T"], case["frame_of"], case["class_of"], case["inst_of"], models)
    idx, d2, counts, own = iref.correspondences_instances(*args, 0.006, "nearest")
    for lo, hi in ((0, 3), (3, 5), (6, 9), (9, 11)):
        n = counts[lo]
        assert (counts[lo:hi] == n).all() and all(np.array_equal(own[lo], own[q]) for q in range(lo, hi))
        assert ((idx[lo:hi, :n] >= 0).sum(axis=0) <= 1).all()                    # at most one member keeps a point
        for q in range(lo, hi):
            kept = idx[q, :n] >= 0
            assert (own[q, :n][kept] == q).all() and (d2[q, :n][kept] <= np.float32(0.006) ** 2).all()
            assert (d2[q, :n][kept] <= d2[lo:hi, :n][:, kept].min(axis=0)).all()
    # a problem alone in its group, and every map-mode problem, is the class form on its set
    cidx, cd2, ccounts = iref.correspondences(case["pcld"], case["mask"], case["T"], case["frame_of"], case["class_of"], models, 0.006)
    assert np.array_equal(idx[5], cidx[5]) and np.array_equal(d2[5], cd2[5]) and (own[5, :counts[5]] == 5).all()
    midx, md2, mcounts, mown = iref.correspondences_instances(*args, 0.006, "map")
    assert list(mcounts) == [64, 65, 7, 30, 25, 40, 65, 0, 5, 0, 0, 0, 8] and (mown[1, :65] == 1).all() and (mown[7] == -1).all()


def test_restatement_of_the_loop_anchors_to_the_class_form():
    case, models = iref.instances_case(192)
    sel = np.array([0, 3, 5, 11, 12])
    f, c, T0 = case["frame_of"][sel], case["class_of"][sel], case["T"][sel]
    wT, wst = iref.icp_refine(case["pcld"], case["mask"], T0, f, c, models, 6, 0.012, tol=3e-4)
    ones = (case["mask"] > 0).astype(np.uint8)
    for mode, imap, iof in (("map", ones, np.ones(5, np.int32)), ("nearest", None, case["inst_of"][sel])):
        T, st = iref.icp_refine_instances(case["pcld"], case["mask"], imap, T0, f, c, iof, models, 6, 0.012, mode, tol=3e-4)
        assert np.array_equal(T, wT) and all(np.array_equal(st[k], wst[k]) for k in wst)
    assert wst["iters"][0] >= 1


def test_a_stopped_problem_goes_on_competing_in_the_restatement():
    """nearest mode, one sibling at its goal with a tolerance: it stops, and the points it owns stay out of its sibling's fit"""
    case, models = iref.instance_views((0,), n_model=512, N=2048)
    args = lambda T: (case["pcld"], case["mask"], None, T, case["frame_of"], case["class_of"], case["inst_of"], models)      # noqa: E731
    settled, _ = iref.icp_refine_instances(*args(case["T0"]), 20, 0.02, "nearest")
    T0 = case["T0"].copy()
    T0[0] = settled[0]
    T, st = iref.icp_refine_instances(*args(T0), 8, 0.02, "nearest", tol=1e-4)
    assert st["iters"][0] < st["iters"][1] == 8 and st["writers"].max() == 1
    own, other = (st["inst"] == 1) & (case["truth"] == 1), (st["inst"] == 2) & (case["truth"] == 1)
    assert own.sum() > 10 * max(other.sum(), 1)
