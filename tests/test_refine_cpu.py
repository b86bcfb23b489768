"""ICP refinement without a GPU (ffb6d_amd/refine.py, csrc/icp.hip, include/ffb6d_refine.h): the library exports the header's
entry points and validates their arguments before any HIP call, the Python layer refuses CPU tensors, and the numpy
restatement the device is held against (tests/icp_ref.py) behaves like an ICP."""
import inspect

import numpy as np
import pytest
import torch

import icp_ref
from ffb6d_amd import synth

ENTRY_POINTS = ("ffb6d_icp_prepared_bytes", "ffb6d_icp_prepare", "ffb6d_icp_workspace_bytes", "ffb6d_icp_set_form",
                "ffb6d_icp_set_pair_counter", "ffb6d_icp_correspond_f32", "ffb6d_icp_refine_f32")


def test_library_exports_the_refinement_entry_points(native_lib):
    from ffb6d_amd import _lib
    for name in ENTRY_POINTS:
        assert hasattr(native_lib, name) and name in _lib.SIGNATURES, name


def test_sizes_are_host_logic(native_lib):
    a256 = lambda n: (n + 255) // 256 * 256                                      # noqa: E731
    P, stride = 40, 12288
    tiles = stride // 64
    want = a256(16 * P * stride) + a256(4 * P) + a256(8 * 17 * P * tiles) + a256(8 * 12 * P) + a256(16 * P)
    assert native_lib.ffb6d_icp_workspace_bytes(P, stride) == want
    assert native_lib.ffb6d_icp_workspace_bytes(0, stride) == 0 and native_lib.ffb6d_icp_workspace_bytes(3, 0) == 0
    total, n_cls = 5 * 2048 + 7, 6
    max_tiles = total // 64 + n_cls
    want = a256(16 * n_cls) + a256(32 * n_cls) + a256(16 * total) + a256(16 * 64 * max_tiles) + a256(32 * max_tiles)
    assert native_lib.ffb6d_icp_prepared_bytes(total, n_cls) == want
    assert native_lib.ffb6d_icp_prepared_bytes(10, 0) == 0
    for form in (1, -1, 0):
        native_lib.ffb6d_icp_set_form(form)
    assert native_lib.ffb6d_icp_set_pair_counter(None) == 0


def test_argument_errors_are_reported_without_a_gpu(native_lib):
    from ffb6d_amd import _lib
    inf = float("inf")
    refine = native_lib.ffb6d_icp_refine_f32
    ok = dict(prepared=64, n_cls=3, total=100, pcld=64, mask=64, bits=64, keep=None, frame_of=64, class_of=64, T0=64, P=2, B=1, N=128,
              stride=128, max_dist=inf, max_iter=5, tol=0.0, min_pairs=3, T=64, n_pairs=None, rms=None, iters=None, ws=None, ws_bytes=0,
              stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return refine(*a.values())

    assert call(P=0) == 0                                                         # nothing to do
    assert call(P=-1) == -1 and "bad sizes" in _lib.last_error()
    assert call(bits=16) == -1 and "mask_bits" in _lib.last_error()
    assert call(stride=64) == -1 and "set_stride" in _lib.last_error()
    assert call(max_dist=0.0) == -1 and "max_dist" in _lib.last_error()
    assert call(max_iter=-1) == -1 and "max_iter" in _lib.last_error()
    assert call(min_pairs=0) == -1 and "min_pairs" in _lib.last_error()
    assert call(T0=None) == -1 and "null pointer" in _lib.last_error()
    assert call() != 0 and "workspace" in _lib.last_error()                       # too small: reported, nothing launched
    corr = native_lib.ffb6d_icp_correspond_f32
    assert corr(64, 3, 100, 64, 64, 64, None, 64, 64, 64, 0, 1, 128, 128, inf, None, None, None, None, 0, None) == 0
    assert corr(64, 3, 100, 64, 64, 64, None, 64, 64, 64, 2, 1, 128, 128, inf, None, None, None, None, 0, None) != 0
    assert "workspace" in _lib.last_error()
    assert native_lib.ffb6d_icp_prepare(None, None, 3, 100, None, 0, None) == -1 and "null pointer" in _lib.last_error()
    assert native_lib.ffb6d_icp_prepare(64, 64, 3, 100, 64, 16, None) != 0 and "bytes" in _lib.last_error()


def test_refine_refuses_cpu_tensors():
    from ffb6d_amd import _lib, evaluate, refine
    models = evaluate.ModelPoints([None, icp_ref.surface_model(1, 64)], device="cpu")
    with pytest.raises(_lib.FFB6DNativeError):
        refine.PreparedModels(models)
    prepared = refine.PreparedModels.__new__(refine.PreparedModels)               # as if prepared: the calls check their own tensors
    prepared.device, prepared.n_cls = torch.device("cpu"), 2
    pcld, mask = torch.zeros(1, 8, 3), torch.zeros(1, 8, dtype=torch.int64)
    for fn in (refine.icp_refine, refine.correspondences):
        with pytest.raises(_lib.FFB6DNativeError):
            fn(pcld, mask, np.zeros((1, 3, 4)), [0], [1], prepared)


def test_solve_poses_and_the_pipeline_take_refine_with_default_none():
    from ffb6d_amd import pipeline, pose
    assert inspect.signature(pose.solve_poses).parameters["refine"].default is None
    assert inspect.signature(pipeline.SensorToPose.__init__).parameters["refine"].default is None


def test_restatement_recovers_an_exact_pose_in_one_iteration():
    """Noise-free full-model input under the true correspondences' pose: one iteration is the Kabsch of a permutation."""
    for seed in range(3):
        model = icp_ref.surface_model(10 + seed, 512)
        pred, gt = synth.eval_pose_pair(seed, "near")
        gt = gt.astype(np.float64)
        scene = (model.astype(np.float64) @ gt[:, :3].T + gt[:, 3])[np.random.RandomState(seed).permutation(len(model))]
        out = icp_ref.icp(scene.astype(np.float32), model, gt, 1, float("inf"))
        assert out["iters"] == 1 and out["n_pairs"] == len(model)
        assert np.abs(out["T"] - gt).max() <= 1e-6
        assert out["rms"] < 1e-6


def test_restatement_ties_gate_and_degenerate_input():
    g = np.arange(4) / 64.0
    model = np.array([[x, y, 0.0] for x in g for y in g] + [[g[0], g[3], 0.0]], np.float32)      # row 16 duplicates row 3
    T = np.zeros((3, 4))
    T[:, :3], T[:, 3] = np.eye(3), [0.0, 0.0, 1.0]
    scene = np.array([[1 / 128.0, 0.0, 1.0], [g[0], g[3], 1.0], [np.nan, 0.0, 1.0], [0.5, 0.5, 1.0]], np.float32)
    c = icp_ref.correspond(scene, model, T, 0.05)
    assert list(c["idx"]) == [0, 3, -1, -1]                                       # equidistant from rows 0 and 4; the duplicate; NaN; gated
    assert c["d2"][0] == np.float32(1 / 128.0) ** 2 and c["d2"][1] == 0 and np.isnan(c["d2"][2])
    assert icp_ref.correspond(scene, model, T, float("inf"))["idx"][3] >= 0 and icp_ref.correspond(scene, model, T, float("inf"))["idx"][2] == -1
    out = icp_ref.icp(scene[:2], model, T, 5, 0.05)                                # two pairs < min_pairs: the pose stays
    assert out["iters"] == 0 and out["n_pairs"] == 2 and np.array_equal(out["T"], T)
    out = icp_ref.icp(scene, np.zeros((0, 3), np.float32), T, 5, 0.05)
    assert out["iters"] == 0 and out["n_pairs"] == 0 and np.array_equal(out["T"], T)


def test_restatement_stops_early_with_a_tolerance():
    model = icp_ref.surface_model(103, 2048)
    pred, gt = synth.eval_pose_pair(3, "near")
    scene = icp_ref.partial_view(model, gt, 203)
    full = icp_ref.icp(scene, model, pred, 30, 0.02)
    early = icp_ref.icp(scene, model, pred, 30, 0.02, tol=1e-5)
    assert full["iters"] == 30 and 1 <= early["iters"] < 30
    assert icp_ref.add(model, early["T"], full["T"]) < 1e-4
