"""csrc/orb.hip on the device, through ffb6d_amd.objinfo and the C ABI: the detector and the lift give the bits of the numpy
restatement (tests/orb_ref.py) on the cases of the emulator tests and on a full-size noise frame with the default parameters (tens
of thousands of candidates on a level); ObjectInfo.from_meshes gives the bits of the chain render_ref -> orb_ref -> lift -> fps_ref;
save_txt writes the two extra files; two runs give identical bytes; a mesh of one colour does not crash."""
import os

import numpy as np
import pytest
import torch

import fps_ref
import orb_ref
import render_ref

from ffb6d_amd import _lib, objinfo, render, synth

pytestmark = pytest.mark.gpu

H, W, K = 96, 128, np.array([[140.0, 0, 64], [0, 140, 48], [0, 0, 1]])        # the reference's camera at a fifth of its size
VIEWS = dict(K=K, H=H, W=W, n1=2, n2=2, min_pixels=50, n_features=60, n_levels=2, edge=8)


def _np(t):
    return t.cpu().numpy()


def assert_detect(got, want, what):
    for name, g, w in zip(("count", "kps", "resp"), got, want):
        g = _np(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(g, w), (what, name, int(np.count_nonzero(g != w)))


def raw_detect(device, rgb, L, t, edge, quota):
    """ffb6d_orb_detect_u8 with explicit quotas, on the current stream"""
    quota = np.ascontiguousarray(quota, np.int32)
    return objinfo._orb_detect(torch.from_numpy(np.array(rgb)).to(device), quota, L, t, edge)


@pytest.mark.parametrize("size,L,quota", orb_ref.CASES)
def test_the_detector_gives_the_bits_of_the_restatement(device, size, L, quota):
    rgb = orb_ref.frames(*size)
    assert_detect(raw_detect(device, rgb, L, 20, 4, quota), orb_ref.detect(rgb, L, 20, 4, quota), (size, L, quota))


@pytest.fixture(scope="module")
def noise_frame():
    """480 x 640 uniform noise, the default parameters: the longest candidate lists (all eight levels live, many tiles, more
    candidates than a workgroup has threads and than one LDS chunk holds), and the restatement, computed once"""
    rgb = orb_ref.noise_rgb(480, 640, 22)[None]
    want = orb_ref.detect(rgb, 8, 20, 31, orb_ref.quotas(500, 8), want_counts=True)
    assert want[3][0, 0] > 20000 and (want[3][0] > 0).all()
    for a in (rgb,) + want:
        a.setflags(write=False)
    return rgb, want[:3]


def test_a_full_size_noise_frame_with_the_default_parameters(device, noise_frame):
    rgb, want = noise_frame
    got = objinfo.orb_detect(torch.from_numpy(rgb.copy()).to(device))
    assert_detect(got, want, "noise")
    again = objinfo.orb_detect(torch.from_numpy(rgb.copy()).to(device))
    for a, b in zip(got, again):
        assert torch.equal(a, b)                               # the append order of the candidates does not leak


def test_long_lists_are_cut_the_same_way_whatever_path_ranks_them(device):
    """about 3000 noise candidates on one level with a quota below and above their number, and 2401 equal responses"""
    rgb = orb_ref.noise_rgb(160, 220, 21)[None]
    for quota in (50, 3200):
        assert_detect(raw_detect(device, rgb, 1, 20, 4, (quota,)), orb_ref.detect(rgb, 1, 20, 4, (quota,)), quota)
    rgb = orb_ref.as_rgb(orb_ref.lattice_dots_image())[None]
    want = orb_ref.detect(rgb, 1, 20, 4, (100,))
    assert want[0][0] == 100 and len(set(want[2][0].tolist())) == 1
    assert_detect(raw_detect(device, rgb, 1, 20, 4, (100,)), want, "lattice")


def test_orb_detect_refuses_what_it_cannot_take(device):
    with pytest.raises(TypeError):
        objinfo.orb_detect(torch.zeros((1, 3, 48, 64), device=device))
    with pytest.raises(ValueError):
        objinfo.orb_detect(torch.zeros((1, 3, 48, 64), dtype=torch.uint8, device=device), edge=3)
    with pytest.raises(_lib.FFB6DNativeError):
        objinfo.orb_detect(torch.zeros((1, 3, 3, 64), dtype=torch.uint8, device=device))


@pytest.mark.parametrize("S,V", [(2, 2), (4, 1), (1, 4)])
def test_lift_and_compaction_give_the_bits_of_the_restatement(device, S, V):
    kps, count, depth, visible, T, Kl = orb_ref.lift_case()
    F, Q = kps.shape[:2]
    want_pts, want_ok = orb_ref.lift(kps, count, depth, visible, T, Kl, 50)
    d = lambda a: torch.from_numpy(a).to(device)                                                                  # noqa: E731
    dk, dc, dd, dv, dT = d(kps), d(count), d(depth), d(visible), d(T)
    slot_pts = torch.full((F, Q, 3), 7, dtype=torch.float32, device=device)
    slot_ok = torch.full((F, Q), 7, dtype=torch.int32, device=device)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.ffb6d_orb_lift_f32(dk.data_ptr(), dc.data_ptr(), dd.data_ptr(), dv.data_ptr(), dT.data_ptr(), F, Q, depth.shape[1], depth.shape[2],
                                Kl[0, 0], Kl[1, 1], Kl[0, 2], Kl[1, 2], 50, slot_pts.data_ptr(), slot_ok.data_ptr(), st)
    _lib.check(rc, "ffb6d_orb_lift_f32")
    assert np.array_equal(_np(slot_ok), want_ok) and np.array_equal(_np(slot_pts).view(np.int32), want_pts.view(np.int32))
    pts = torch.full((F * Q, 3), 7, dtype=torch.float32, device=device)
    begin = torch.full((S + 1,), 7, dtype=torch.int64, device=device)
    n_found = torch.full((S,), 7, dtype=torch.int32, device=device)
    rc = lib.ffb6d_orb_compact_f32(slot_pts.data_ptr(), slot_ok.data_ptr(), S, V, Q, pts.data_ptr(), begin.data_ptr(), n_found.data_ptr(), st)
    _lib.check(rc, "ffb6d_orb_compact_f32")
    w_pts, w_begin, w_found = orb_ref.compact(want_pts, want_ok, S, V)
    assert np.array_equal(_np(n_found), w_found) and np.array_equal(_np(begin), w_begin)
    assert np.array_equal(_np(pts).view(np.int32), w_pts.view(np.int32))


def two_meshes():
    """class 0 = the background; an icosphere with its seeded colours; a squashed one with other colours"""
    a = synth.sphere_mesh(2)
    b = synth.sphere_mesh(2, radius=0.08, seed=4)
    b = dict(xyz=(b["xyz"] * np.array([1.0, 0.7, 1.2], np.float32)).astype(np.float32), faces=b["faces"],
             rgb=np.random.RandomState(9).randint(0, 256, b["rgb"].shape).astype(np.uint8))
    return [None, a, b]


def reference_chain(meshes, n_keypoints=8, **views):
    """render_ref -> orb_ref -> lift -> fps_ref, with the arguments of objinfo.textured_points"""
    S, V = len(meshes), views["n1"] * views["n2"]
    radius = np.array([fps_ref.box(m["xyz"] if m is not None else np.zeros((0, 3)))[2] for m in meshes], np.float32)
    T = objinfo.view_poses(radius, views["n1"], views["n2"]).reshape(S * V, 3, 4)
    out = render_ref.render(meshes, T, np.arange(S * V), np.repeat(np.arange(S), V), views["K"], S * V, views["H"], views["W"])
    quota = orb_ref.quotas(views["n_features"], views["n_levels"])
    count, kps, _ = orb_ref.detect(out["rgb"], views["n_levels"], 20, views["edge"], quota)
    slot_pts, slot_ok = orb_ref.lift(kps, count, out["depth"], out["visible"], T, views["K"], views["min_pixels"])
    pts, begin, n_found = orb_ref.compact(slot_pts, slot_ok, S, V)
    mesh_kps = fps_ref.fps_batch(orb_ref.point_sets(pts, begin), n_keypoints, None)[1]
    return dict(T=T, pts=pts, begin=begin, n_found=n_found, mesh_kps=mesh_kps, visible=out["visible"], count=count)


@pytest.fixture(scope="module")
def scene(device):
    meshes = two_meshes()
    want = reference_chain(meshes, **VIEWS)
    info = objinfo.ObjectInfo.from_meshes(render.PreparedMeshes(meshes, device=device), n_keypoints=8, n_model_points=64, **VIEWS)
    return meshes, want, info


def test_from_meshes_gives_the_bits_of_the_reference_chain(device, scene):
    meshes, want, info = scene
    assert want["n_found"][0] == 0 and (want["n_found"][1:] >= 8).all(), want["n_found"]       # the case has points to sample
    assert (want["visible"][4:] >= 50).all() and not want["visible"][:4].any()
    assert np.array_equal(_np(objinfo.view_poses(info.radius, 2, 2)).reshape(-1, 3, 4), want["T"])          # device poses = host poses
    tex = info.textured
    assert tex.S == 3 and tex.max_n == 4 * 60 and tuple(tex.pts.shape) == (3 * 4 * 60, 3)
    assert np.array_equal(_np(info.n_found), want["n_found"]) and np.array_equal(_np(tex.begin), want["begin"])
    assert np.array_equal(_np(tex.pts).view(np.int32), want["pts"].view(np.int32))
    assert np.array_equal(_np(info.mesh_kps).view(np.int32), want["mesh_kps"].view(np.int32))
    assert not _np(info.mesh_kps[0]).any() and info.kps_idx is None
    # everything else is from_points'
    base = objinfo.ObjectInfo.from_points(render.PreparedMeshes(meshes, device=device), n_keypoints=8, n_model_points=64)
    assert torch.equal(info.fps_kps, base.mesh_kps) and torch.equal(info.mesh_ctr, base.mesh_ctr) and torch.equal(info.radius, base.radius)
    assert torch.equal(info.corners, base.corners) and torch.equal(info.models.pts, base.models.pts)
    assert not torch.equal(info.mesh_kps, base.mesh_kps)
    assert base.fps_kps is None and base.n_found is None and base.textured is None
    # the keypoints lie on the surface: the textured points are lifted from rendered depth
    r = np.linalg.norm(_np(info.mesh_kps[1]), axis=1)
    assert np.abs(r - 0.1).max() < 2e-3
    # farthest_point_sampling takes the point sets as they are
    idx, pts = objinfo.farthest_point_sampling(tex, 8, start="center")
    assert torch.equal(pts, info.mesh_kps) and (_np(idx[0]) == -1).all()


def test_two_runs_give_identical_bytes(device, scene):
    meshes, _, info = scene
    again = objinfo.ObjectInfo.from_meshes(meshes, n_keypoints=8, n_model_points=64, **VIEWS)
    assert torch.equal(again.mesh_kps, info.mesh_kps) and torch.equal(again.n_found, info.n_found)
    assert torch.equal(again.textured.pts, info.textured.pts) and torch.equal(again.textured.begin, info.textured.begin)


def test_chunks_of_frames_give_the_same_points(device, scene, monkeypatch):
    """one object per chunk instead of all three in one"""
    meshes, _, info = scene
    monkeypatch.setattr(objinfo, "CHUNK_FRAMES", 4)
    tex = objinfo.textured_points(meshes, **VIEWS)
    assert torch.equal(tex.pts, info.textured.pts) and torch.equal(tex.begin, info.textured.begin)
    assert torch.equal(tex.n_found, info.n_found)


def test_save_txt_writes_the_two_files_of_the_textured_keypoints(device, scene, tmp_path):
    meshes, _, info = scene
    written = info.save_txt(str(tmp_path), [None, "ball", "egg"])
    names = sorted(os.path.basename(p) for p in written)
    assert names == sorted(f"{n}_{s}.txt" for n in ("ball", "egg") for s in ("fps", "corners", "center", "radius", "ORB_fps", "8_kps"))
    for c, n in ((1, "ball"), (2, "egg")):
        for suffix in ("ORB_fps", "8_kps"):
            back = np.loadtxt(os.path.join(str(tmp_path), f"{n}_{suffix}.txt"), dtype=np.float32)
            assert np.array_equal(back.view(np.int32), _np(info.mesh_kps[c]).view(np.int32)), (n, suffix)
        back = np.loadtxt(os.path.join(str(tmp_path), f"{n}_fps.txt"), dtype=np.float32)
        assert np.array_equal(back.view(np.int32), _np(info.fps_kps[c]).view(np.int32))
    # an object built by from_points writes exactly the files it wrote before
    base = objinfo.ObjectInfo.from_points(render.PreparedMeshes(meshes, device=device), n_keypoints=8)
    plain = base.save_txt(str(tmp_path / "plain"), [None, "ball", "egg"])
    assert sorted(os.path.basename(p) for p in plain) == sorted(f"{n}_{s}.txt" for n in ("ball", "egg")
                                                                for s in ("fps", "corners", "center", "radius"))


def test_a_mesh_of_one_colour_does_not_crash(device):
    m = synth.sphere_mesh(1)
    meshes = [None, dict(xyz=m["xyz"], faces=m["faces"], rgb=np.full(m["rgb"].shape, 120, np.uint8))]
    want = reference_chain(meshes, **VIEWS)
    info = objinfo.ObjectInfo.from_meshes(meshes, n_keypoints=8, **VIEWS)
    assert (want["visible"][4:] >= 50).all()
    assert np.array_equal(_np(info.n_found), want["n_found"])
    assert np.array_equal(_np(info.textured.pts).view(np.int32), want["pts"].view(np.int32))
    assert np.array_equal(_np(info.mesh_kps).view(np.int32), want["mesh_kps"].view(np.int32))
    assert info.models is None
