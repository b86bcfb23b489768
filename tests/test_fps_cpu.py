"""Farthest-point sampling without a GPU: the numpy restatement (tests/fps_ref.py) reproduces every index sequence recorded from
the reference's compiled farthest_point_sampling.cpp (tests/golden/fps_ref.npz, made by tests/golden/make_golden_fps.py) exactly,
include/ffb6d_fps.h is bound one to one, and ffb6d_amd.objinfo judges on the host what the host can see.  The box formulas have
no recorded golden -- the reference's MeshUtils imports OpenCV and plyfile, which the build image lacks -- so they are pinned by
the restatement of its lines and by hand-computed vectors."""
import os

import numpy as np
import pytest
import torch

import fps_ref
from conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "fps_ref.npz"))
    return [dict(kind=str(g["kind"][i]), n=int(g["n"][i]), m=int(g["m"][i]), pts=g[f"pts{i}"], ctr=g[f"ctr{i}"].astype(np.int32),
                 rnd=g[f"rnd{i}"].astype(np.int32)) for i in range(len(g["n"]))]


def test_the_golden_covers_the_sizes_and_kinds_it_is_meant_to(golden):
    assert {c["n"] for c in golden} == {1, 5, 64, 65, 300, 1000, 5000}
    assert {c["kind"] for c in golden} == set(fps_ref.KINDS)
    assert max(c["m"] for c in golden) == 2048 and any(c["m"] > c["n"] for c in golden)
    for c in golden:
        assert c["pts"].dtype == np.float32 and c["pts"].shape == (c["n"], 3) and c["ctr"].shape == c["rnd"].shape == (c["m"],)
        assert 0 <= c["rnd"][0] < c["n"]
    assert any(len(set(c["ctr"].tolist())) < min(c["n"], c["m"]) for c in golden if c["kind"] == "duplicate")       # the index-0 rule
    assert os.path.getsize(os.path.join(GOLDEN, "fps_ref.npz")) < 200 * 1024


def test_the_restatement_reproduces_every_reference_sequence_exactly(golden):
    for i, c in enumerate(golden):
        idx, pts, dist = fps_ref.fps(c["pts"], c["m"], None)
        assert np.array_equal(idx, c["ctr"]), (i, "init_center")
        assert np.array_equal(pts, c["pts"][c["ctr"]])
        idx, _, dist = fps_ref.fps(c["pts"], c["m"], int(c["rnd"][0]))
        assert np.array_equal(idx, c["rnd"]), (i, "given start")
        assert dist[0] == fps_ref.FLT_MAX and (dist[1:] <= dist[0]).all()


def test_the_distances_of_the_restatement_are_what_they_are_said_to_be():
    """out_dist[k] is the pick's squared distance to the nearest earlier pick, in the reference's float32 arithmetic; it never
    grows, and it is 0 exactly where the index-0 rule has taken over"""
    pts = fps_ref.duplicate_set(40, 3)
    idx, out, dist = fps_ref.fps(pts, 30, 7)
    for k in range(1, 30):
        assert dist[k] == fps_ref.dist2(pts[idx[:k]], out[k]).min()
    assert (np.diff(dist[1:]) <= 0).all() and (dist[1:20] > 0).all() and not dist[20:].any() and not idx[20:].any()


def test_box_restatement_against_hand_computed_vectors():
    pts = np.array([[1, -2, 3], [-1, 2, 7], [0, 0, 4]], np.float32)
    want = [[-1, -2, 3], [-1, -2, 7], [-1, 2, 3], [-1, 2, 7], [1, -2, 3], [1, -2, 7], [1, 2, 3], [1, 2, 7]]
    for corners, ctr, radius in (fps_ref.box(pts), fps_ref.box64(pts)):
        assert np.array_equal(corners, want) and np.array_equal(ctr, [0, 0, 5]) and radius == 3
    c, m, r = fps_ref.box(np.zeros((0, 3), np.float32))
    assert not c.any() and not m.any() and r == 0
    p = fps_ref.random_set(500, 1)
    (c32, m32, r32), (c64, m64, r64) = fps_ref.box(p), fps_ref.box64(p)
    assert np.array_equal(c32, c64) and np.array_equal(m32, m64.astype(np.float32)) and abs(r32 - r64) <= 1e-6 * r64      # halving is exact


def test_prototypes_mirror_the_header(native_lib):
    from ffb6d_amd import _lib
    for name in ("ffb6d_fps_resident_capacity", "ffb6d_fps_set_form", "ffb6d_fps_workspace_bytes", "ffb6d_fps_f32", "ffb6d_box_info_f32"):
        assert name in _lib.SIGNATURES and hasattr(native_lib, name)
    cap = native_lib.ffb6d_fps_resident_capacity()
    assert cap >= 8192
    try:
        assert native_lib.ffb6d_fps_workspace_bytes(21, cap, 8) == 0 and native_lib.ffb6d_fps_workspace_bytes(21, cap + 1, 8) == (21 * (cap + 1) * 4 + 255) // 256 * 256
        native_lib.ffb6d_fps_set_form(2)
        assert native_lib.ffb6d_fps_workspace_bytes(3, 100, 8) == 1280
        native_lib.ffb6d_fps_set_form(1)
        assert native_lib.ffb6d_fps_workspace_bytes(3, cap + 1, 8) == 0
        assert native_lib.ffb6d_fps_f32(None, 8, 3, 0, cap + 1, 8, None, 8, None, None, None, 0, None) == -1 and "capacity" in _lib.last_error()
    finally:
        native_lib.ffb6d_fps_set_form(0)
    # refused before anything touches a device
    assert native_lib.ffb6d_fps_f32(None, None, 1, 0, 0, 0, None, None, None, None, None, 0, None) == -1 and "bad sizes" in _lib.last_error()
    assert native_lib.ffb6d_fps_f32(None, None, 0, 0, 0, 8, None, None, None, None, None, 0, None) == -1 and "bad sizes" in _lib.last_error()
    assert native_lib.ffb6d_fps_f32(None, 8, 1, 0, 0, 8, None, None, None, None, None, 0, None) == -1 and "no output" in _lib.last_error()
    assert native_lib.ffb6d_box_info_f32(None, None, 1, 0, 8, None, None, None) == -1 and "null pointer" in _lib.last_error()


def test_objinfo_judges_on_the_host_what_the_host_can_see(native_lib):
    from ffb6d_amd import _lib, objinfo
    good = np.zeros((10, 3), np.float32)
    for bad in (np.zeros((10, 2), np.float32), np.zeros(10, np.float32), np.zeros((2, 3, 10, 3), np.float32), np.zeros((0, 10, 3), np.float32)):
        with pytest.raises(ValueError, match="points must"):
            objinfo.farthest_point_sampling(bad, 4)
        with pytest.raises(ValueError, match="points must"):
            objinfo.box_info(bad)
    with pytest.raises(TypeError, match="floating point"):
        objinfo.farthest_point_sampling(np.zeros((10, 3), np.int32), 4)
    for v in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[3, 1] = v
        with pytest.raises(ValueError, match="not finite"):
            objinfo.farthest_point_sampling(bad, 4)
        with pytest.raises(ValueError, match="not finite"):
            objinfo.box_info(bad[None])
    for m in (0, -1, 2.5):
        with pytest.raises(ValueError, match="at least 1"):
            objinfo.farthest_point_sampling(good, m)
    with pytest.raises(ValueError, match="center"):
        objinfo.farthest_point_sampling(good, 4, start="centre of mass")
    with pytest.raises(_lib.FFB6DNativeError, match="GPU only"):          # no CPU fallback
        objinfo.farthest_point_sampling(torch.zeros(10, 3), 4)
    with pytest.raises(_lib.FFB6DNativeError, match="GPU only"):
        objinfo.box_info(torch.zeros(2, 10, 3))
    with pytest.raises(TypeError, match="PreparedMeshes"):
        objinfo.ObjectInfo.from_points(good)
    with pytest.raises(ValueError, match="form must be"):
        objinfo.set_form(3)
    assert objinfo.set_form(2) == 0 and objinfo.FORM == 2
    assert objinfo.set_form(0) == 2 and objinfo.FORM == 0
    assert objinfo.resident_capacity() == native_lib.ffb6d_fps_resident_capacity()
    s = objinfo._Sets()
    s.S, s.counts, s.device = 3, np.array([5, 0, 7]), torch.device("cpu")
    assert objinfo._start("center", s) is None
    assert objinfo._start(4, s).tolist() == [4, 4, 4] and objinfo._start([4, 0, 6], s).dtype == torch.int32
    assert objinfo._start([0, 9, 0], s).tolist() == [0, 9, 0]             # an empty set has no first pick to name
    for bad in (5, -1, [0, 0, 7], [0, 0], 1.0):
        with pytest.raises(ValueError, match="start"):
            objinfo._start(bad, s)


def test_save_txt_round_trips_through_loadtxt(tmp_path):
    """the files of gen_obj_info.py:98-117, read the way Basic_Utils.get_kps / get_ctr read them (np.loadtxt)"""
    from ffb6d_amd import objinfo
    rng = np.random.RandomState(5)
    kps = rng.uniform(-0.2, 0.2, (3, 8, 3)).astype(np.float32)
    corners = np.stack([fps_ref.box(k)[0] for k in kps])
    ctr = np.stack([fps_ref.box(k)[1] for k in kps])
    radius = np.array([fps_ref.box(k)[2] for k in kps], np.float32)
    info = objinfo.ObjectInfo(*(torch.from_numpy(a) for a in (kps, ctr, corners, radius)))
    assert info.n_cls == 3 and info.n_kps == 8 and np.array_equal(info.r_lst.numpy(), radius[1:]) and info.models is None
    written = info.save_txt(str(tmp_path / "kps"), [None, "ape", "can"])
    assert sorted(os.path.basename(p) for p in written) == sorted(f"{n}_{s}.txt" for n in ("ape", "can") for s in ("fps", "corners", "center", "radius"))
    for c, name in ((1, "ape"), (2, "can")):
        load = lambda s: np.loadtxt(str(tmp_path / "kps" / f"{name}_{s}.txt"), dtype=np.float32)      # noqa: E731
        assert np.array_equal(load("fps"), kps[c]) and np.array_equal(load("corners"), corners[c])
        assert np.array_equal(load("center"), ctr[c]) and load("center").shape == (3,)
        assert load("radius").shape == () and load("radius") == radius[c]
    assert info.save_txt(str(tmp_path / "by_dict"), {2: "can"}) and not os.path.exists(str(tmp_path / "by_dict" / "ape_fps.txt"))
    with pytest.raises(ValueError, match="names"):
        info.save_txt(str(tmp_path / "kps"), ["a"])
