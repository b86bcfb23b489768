"""csrc/fps.hip on the device, through ffb6d_amd.objinfo: the index sequences recorded from the reference's compiled
farthest_point_sampling.cpp (tests/golden/fps_ref.npz) are reproduced exactly; both kernel forms give the bits of the numpy
restatement (tests/fps_ref.py) at every size where the code takes another path; every output element is written; the box
statistics equal the float64 restatement of the reference's lines (its MeshUtils imports OpenCV and plyfile, which the build image
lacks, so no golden of it could be recorded); and an ObjectInfo feeds the solver, the training targets and ICP as it is."""
import os

import numpy as np
import pytest
import torch

import fps_ref
import render_ref
from conftest import GOLDEN

from ffb6d_amd import _lib, evaluate, objinfo, pose, refine, render, synth, train_data

pytestmark = pytest.mark.gpu

BLOCK = 1024                 # threads of a workgroup of csrc/fps.hip: point i of a set lives in thread i % 1024


def _np(t):
    return t.cpu().numpy()


def assert_same_bits(got, want, what):
    for name, g, w in zip(("idx", "pts", "dist"), got, want):
        g = _np(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(g.view(np.int32), w.view(np.int32)), (what, name, int(np.count_nonzero(g != w)))


@pytest.fixture(scope="module")
def cap(device):
    return objinfo.resident_capacity()


@pytest.fixture(scope="module")
def unequal(cap):
    """unequal sets in one call, an empty one among them: lattice points (ties) around the wave and workgroup sizes, duplicates,
    random points up to the resident capacity; and their restatement, computed once"""
    sizes = [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, cap - 1, cap]
    kinds = ["lattice", "lattice", "lattice", "duplicate", "lattice", "lattice", "duplicate", "lattice", "random", "random"]
    sets = [fps_ref.KINDS[k](n, 1200 + i) for i, (k, n) in enumerate(zip(kinds, sizes))]
    start = np.array([0 if n == 0 else (n - 1) * (i % 3) // 2 for i, n in enumerate(sizes)], np.int32)
    want = {"center": fps_ref.fps_batch(sets, 16, None), "start": fps_ref.fps_batch(sets, 16, start)}
    for arrs in want.values():
        for a in arrs:
            a.setflags(write=False)
    return sets, start, want


def test_reference_sequences_are_reproduced_exactly(device):
    g = np.load(os.path.join(GOLDEN, "fps_ref.npz"))
    for i in range(len(g["n"])):
        pts, m = torch.from_numpy(g[f"pts{i}"]).to(device), int(g["m"][i])
        idx, out = objinfo.farthest_point_sampling(pts, m, start="center")
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (m,) and tuple(out.shape) == (m, 3)
        assert np.array_equal(_np(idx), g[f"ctr{i}"].astype(np.int32)), (i, "init_center")
        assert torch.equal(out, pts[idx.long()])
        rnd = g[f"rnd{i}"].astype(np.int32)
        idx, out = objinfo.farthest_point_sampling(pts, m, start=int(rnd[0]))
        assert np.array_equal(_np(idx), rnd), (i, "given start")
        assert torch.equal(out, pts[idx.long()])


@pytest.mark.parametrize("mode", ["center", "start"])
def test_both_forms_give_the_bits_of_the_restatement(device, unequal, mode):
    sets, start, want = unequal
    mp = evaluate.ModelPoints(sets, device=device)
    st = "center" if mode == "center" else start
    try:
        for form in (1, 2, 0):
            objinfo.set_form(form)
            got = objinfo.farthest_point_sampling(mp, 16, start=st, return_dist=True)
            assert_same_bits(got, want[mode], (mode, form))
        objinfo.set_form(0)
        got = objinfo.farthest_point_sampling(mp, 16, start=torch.from_numpy(start).to(device) if mode == "start" else st, return_dist=True)
        assert_same_bits(got, want[mode], (mode, "device start"))
    finally:
        objinfo.set_form(0)


def test_one_point_above_the_capacity_takes_the_streaming_form(device, cap):
    lib = _lib.load()
    sets = [fps_ref.random_set(cap + 1, 77), fps_ref.lattice_set(300, 78), np.zeros((0, 3), np.float32)]
    want = fps_ref.fps_batch(sets, 16, None)
    mp = evaluate.ModelPoints(sets, device=device)
    assert objinfo.FORM == 0
    assert lib.ffb6d_fps_workspace_bytes(3, cap, 16) == 0 and lib.ffb6d_fps_workspace_bytes(3, cap + 1, 16) > 0       # resident / streaming
    got = objinfo.farthest_point_sampling(mp, 16, start="center", return_dist=True)
    assert_same_bits(got, want, "cap + 1")
    try:
        objinfo.set_form(1)
        with pytest.raises(_lib.FFB6DNativeError, match="capacity"):
            objinfo.farthest_point_sampling(mp, 16, start="center")
    finally:
        objinfo.set_form(0)
    # a dense batch and a single set, the same points: the same picks
    dense = torch.from_numpy(np.stack([sets[0], sets[0][::-1].copy()])).to(device)
    idx, out = objinfo.farthest_point_sampling(dense, 16, start="center")
    assert np.array_equal(_np(idx[0]), want[0][0]) and np.array_equal(_np(out[0]), want[1][0])
    one = objinfo.farthest_point_sampling(dense[1], 16, start="center")
    assert torch.equal(one[0], idx[1]) and torch.equal(one[1], out[1]) and tuple(one[0].shape) == (16,)


def test_identical_and_duplicate_points_fall_back_to_index_zero(device):
    sets = [fps_ref.identical_set(100, 1), fps_ref.duplicate_set(BLOCK + 1, 2), fps_ref.duplicate_set(9, 3), fps_ref.random_set(1, 4)]
    m = 600                                                             # above the 513 distinct points of the largest set
    mp = evaluate.ModelPoints(sets, device=device)
    try:
        for form in (1, 2):
            objinfo.set_form(form)
            for st in ("center", 0, np.array([99, BLOCK, 8, 0])):
                want = fps_ref.fps_batch(sets, m, None if isinstance(st, str) else np.broadcast_to(st, (4,)))
                got = objinfo.farthest_point_sampling(mp, m, start=st, return_dist=True)
                assert_same_bits(got, want, (form, st))
                idx, dist = want[0], want[2]
                assert not idx[0, 1:].any() and not dist[0, 1:].any() and not idx[1, 513:].any() and (dist[1, 1:513] > 0).all()
    finally:
        objinfo.set_form(0)


def test_every_output_element_is_written_and_the_empty_row_is_as_specified(device, unequal):
    """the C ABI itself, on outputs pre-filled with a sentinel no result can hold (an index of -7, NaN)"""
    sets, start, want = unequal
    mp = evaluate.ModelPoints(sets, device=device)
    S, m = len(sets), 16
    lib = _lib.load()
    try:
        for form in (1, 2):
            lib.ffb6d_fps_set_form(form)
            idx = torch.full((S, m), -7, dtype=torch.int32, device=device)
            out = torch.full((S, m, 3), float("nan"), device=device)
            dist = torch.full((S, m), float("nan"), device=device)
            wbytes = lib.ffb6d_fps_workspace_bytes(S, mp.max_points, m)
            ws = torch.full((max(wbytes, 1),), 0xFF, dtype=torch.uint8, device=device)           # NaN as min_dist: must not be read before it is written
            rc = lib.ffb6d_fps_f32(mp.pts.data_ptr(), mp.begin.data_ptr(), S, int(mp.pts.shape[0]), mp.max_points, m, None, idx.data_ptr(),
                                   out.data_ptr(), dist.data_ptr(), ws.data_ptr(), wbytes, torch.cuda.current_stream(device).cuda_stream)
            assert rc == 0, _lib.last_error()
            assert_same_bits((idx, out, dist), want["center"], form)
            assert (idx[0] == -1).all() and not out[0].any() and not dist[0].any()               # the empty set
            assert (idx[1:] >= 0).all() and not torch.isnan(out).any() and not torch.isnan(dist).any()
    finally:
        lib.ffb6d_fps_set_form(0)


def test_box_info_equals_the_float64_restatement(device, unequal):
    sets = list(unequal[0]) + [np.array([[1, -2, 3], [-1, 2, 7], [0, 0, 4]], np.float32), fps_ref.random_set(20000, 9) * 3]
    corners, ctr, radius = (_np(t) for t in objinfo.box_info(evaluate.ModelPoints(sets, device=device)))
    assert corners.shape == (len(sets), 8, 3) and ctr.shape == (len(sets), 3) and radius.shape == (len(sets),)
    for s, p in enumerate(sets):
        c64, m64, r64 = fps_ref.box64(p)
        assert np.array_equal(corners[s], c64), s
        assert np.array_equal(ctr[s], m64.astype(np.float32)), s             # halving is exact: one rounding, that of max + min
        assert abs(radius[s] - r64) <= 1e-6 * r64, (s, radius[s], r64)
        c32, m32, r32 = fps_ref.box(p)
        assert radius[s].view(np.int32) == r32.view(np.int32), s
    assert np.array_equal(ctr[-2], [0, 0, 5]) and radius[-2] == 3 and not corners[0].any() and radius[0] == 0
    one = objinfo.box_info(torch.from_numpy(sets[-1]).to(device))
    assert tuple(one[0].shape) == (8, 3) and tuple(one[1].shape) == (3,) and one[2].dim() == 0
    assert np.array_equal(_np(one[0]), corners[-1]) and np.array_equal(_np(one[1]), ctr[-1]) and float(one[2]) == radius[-1]


@pytest.fixture(scope="module")
def scene_info(device):
    s = render_ref.small_scene()
    meshes = render.PreparedMeshes(s["meshes"], device=device)
    return s, meshes, objinfo.ObjectInfo.from_points(meshes, n_keypoints=8, n_model_points=100)


def test_object_info_of_the_small_scene(device, scene_info):
    s, meshes, info = scene_info
    n_cls = len(s["meshes"])
    assert tuple(info.mesh_kps.shape) == (n_cls, 8, 3) and tuple(info.mesh_ctr.shape) == (n_cls, 3) and tuple(info.r_lst.shape) == (n_cls - 1,)
    assert tuple(info.corners.shape) == (n_cls, 8, 3) and info.mesh_kps.dtype == info.mesh_ctr.dtype == info.r_lst.dtype == torch.float32
    kps, idx = _np(info.mesh_kps), _np(info.kps_idx)
    sets = [np.zeros((0, 3), np.float32) if m is None else np.asarray(m["xyz"], np.float32) for m in s["meshes"]]
    want = fps_ref.fps_batch(sets, 8, None)
    assert np.array_equal(idx, want[0]) and np.array_equal(kps.view(np.int32), want[1].view(np.int32))
    for c, p in enumerate(sets):
        if len(p):
            assert np.array_equal(kps[c], p[idx[c]]), c                       # mesh_kps = pts[idx]
            assert np.array_equal(_np(info.mesh_ctr[c]), fps_ref.box(p)[1]) and _np(info.r_lst)[c - 1] == fps_ref.box(p)[2]
        else:
            assert (idx[c] == -1).all() and not kps[c].any() and not _np(info.mesh_ctr[c]).any()
    # the model clouds: min(n, 100) points per class in FPS order; a class with fewer keeps every point once
    models = info.models
    assert isinstance(models, evaluate.ModelPoints) and models.n_cls == n_cls
    assert np.array_equal(models.counts, [min(len(p), 100) for p in sets]) and np.array_equal(_np(models.begin), np.concatenate([[0], np.cumsum(models.counts)]))
    cloud = _np(models.pts)
    for c, p in enumerate(sets):
        mine = cloud[int(models.begin[c]):int(models.begin[c + 1])]
        if len(p) > 100:
            assert np.array_equal(mine, p[fps_ref.fps(p, 100, None)[0]]), c
        elif len(p):
            order = fps_ref.fps(p, len(p), None)[0]
            first = order[np.sort(np.unique(order, return_index=True)[1])]                      # picks, in the order of first appearance
            assert np.array_equal(mine[:len(first)], p[first]), c
            assert np.array_equal(np.sort(mine.view("f4,f4,f4").ravel()), np.sort(p.view("f4,f4,f4").ravel())), c     # every point, once
    assert objinfo.ObjectInfo.from_points(meshes).models is None


def test_icp_takes_the_model_clouds_and_finds_every_point_on_itself(device, scene_info):
    _, _, info = scene_info
    prepared = refine.PreparedModels(info.models)
    eye = np.eye(4)[None, :3]
    for c in np.nonzero(info.models.counts)[0]:
        own = info.models.pts[int(info.models.begin[c]):int(info.models.begin[c + 1])]
        n = int(own.shape[0])
        mask = torch.full((1, n), int(c), dtype=torch.int32, device=device)
        idx, d2, counts = refine.correspondences(own[None].contiguous(), mask, eye, [0], [int(c)], prepared)
        assert int(counts[0]) == n and not d2[0, :n].any(), c
        assert torch.equal(own[idx[0, :n].long()], own), c


def test_targets_and_solver_take_the_device_tensors_as_they_are(device, scene_info):
    """info.mesh_kps / mesh_ctr / r_lst go in without a conversion and give the bits their host copies give"""
    s, _, info = scene_info
    n_cls, B, N, H, W = len(s["meshes"]), 2, 1024, 16, 64
    rng = np.random.RandomState(11)
    cld = torch.from_numpy(rng.uniform(-0.3, 0.3, (B, N, 3)).astype(np.float32) + np.float32([0, 0, 0.8])).to(device)
    choose = torch.arange(N, device=device).repeat(B, 1)
    labels = rng.choice([0, 1, 2, 5], (B, H, W)).astype(np.int32)
    lab_img = torch.from_numpy(labels).to(device)
    ids = np.array([[1, 2, 5], [5, 0, 1]])
    RTs = np.stack([np.stack([np.concatenate([synth.random_rotation(rng), rng.uniform(-0.1, 0.1, (3, 1)) + [[0], [0], [0.8]]], 1)
                              for _ in range(3)]) for _ in range(B)])
    host = train_data.pose_targets(cld, choose, lab_img, ids, RTs, _np(info.mesh_kps), _np(info.mesh_ctr))
    dev = train_data.pose_targets(cld, choose, lab_img, ids, RTs, info.mesh_kps, info.mesh_ctr)
    assert set(host) == set(dev)
    for k in host:
        assert host[k].dtype == dev[k].dtype and torch.equal(host[k].view(torch.int32) if host[k].dtype == torch.float32 else host[k],
                                                             dev[k].view(torch.int32) if dev[k].dtype == torch.float32 else dev[k]), k
    assert host["kp_targ_ofst"].abs().sum() > 0
    args = (cld, host["labels"].long(), host["ctr_targ_ofst"][:, None], host["kp_targ_ofst"].permute(0, 2, 1, 3).contiguous())
    a = pose.solve_poses(*args, _np(info.mesh_kps), _np(info.mesh_ctr), r_lst=_np(info.r_lst))
    b = pose.solve_poses(*args, info.mesh_kps, info.mesh_ctr, r_lst=info.r_lst)
    assert len(a) == len(b) == B
    for (ca, pa, ka), (cb, pb, kb) in zip(a, b):
        # the two calls differ only in where the model keypoints come from; the solver's own run-to-run reproducibility is not
        # this test's subject, so poses (metres, rotations of norm 1) are compared to 1e-5 instead of bit for bit
        assert len(ca) > 0 and np.array_equal(ca, cb) and np.allclose(pa, pb, rtol=0, atol=1e-5) and np.allclose(ka, kb, rtol=0, atol=1e-5)
