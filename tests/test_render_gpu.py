"""The rasteriser on the device (ffb6d_amd/render.py, csrc/render.hip): every output of the small scene equals the numpy
restatement (tests/render_ref.py) bit for bit in all forms of the raster pass and from run to run, the result does not depend on
the order of faces or instances, full-size frames of occluding spheres are geometrically right, and rendered frames go through the
training-batch builder."""
import numpy as np
import pytest
import torch

import render_ref
from ffb6d_amd import inputs, render, synth, train_data

pytestmark = pytest.mark.gpu

ALL = ("rgb", "depth", "label", "inst", "face", "visible")


@pytest.fixture(scope="module")
def scene():
    s = render_ref.small_scene()
    want = render_ref.render(s["meshes"], s["T"], s["frame_of"], s["class_of"], s["K"], s["B"], s["H"], s["W"])
    for v in want.values():
        v.setflags(write=False)
    return s, want


def draw(s, device, meshes=None, order=None, outputs=ALL):
    """the scene through render.render; the ids go in as device tensors (a frame of 7 and a class of 9 are not host-checked)"""
    order = np.arange(len(s["T"])) if order is None else order
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)           # noqa: E731
    out = render.render(render.PreparedMeshes(s["meshes"] if meshes is None else meshes, device), s["T"][order], t(s["frame_of"][order]),
                        t(s["class_of"][order]), s["K"], s["B"], s["H"], s["W"], outputs=outputs)
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                                        b.view(np.uint32) if b.dtype == np.float32 else b)


@pytest.mark.parametrize("form", [0, 1, -1])
def test_small_scene_equals_the_restatement_as_bits(device, scene, form):
    s, want = scene
    prev = render.set_form(form)
    try:
        got = draw(s, device)
    finally:
        render.set_form(prev)
    for k in ALL:
        assert same_bits(got[k], want[k]), (form, k, int(np.count_nonzero(got[k] != want[k])))


def test_two_runs_give_the_same_bits_and_outputs_are_optional(device, scene):
    s, want = scene
    a, b = draw(s, device), draw(s, device)
    for k in ALL:
        assert same_bits(a[k], b[k]), k
    got = draw(s, device, outputs=("depth", "visible"))
    assert set(got) == {"depth", "visible"} and same_bits(got["depth"], want["depth"]) and same_bits(got["visible"], want["visible"])
    with pytest.raises(ValueError):
        render.render(s["meshes"], s["T"], s["frame_of"], s["class_of"], s["K"], s["B"], s["H"], s["W"])      # host ids are checked


def test_permuting_faces_changes_only_face_and_permuting_instances_only_inst(device, scene):
    s, want = scene
    perm = np.random.RandomState(0).permutation(len(s["meshes"][1]["faces"]))
    meshes = list(s["meshes"])
    meshes[1] = dict(meshes[1], faces=meshes[1]["faces"][perm])
    got = draw(s, device, meshes=meshes)
    for k in ("rgb", "depth", "label", "inst", "visible"):
        assert same_bits(got[k], want[k]), k
    own = np.isin(want["inst"], np.flatnonzero(s["class_of"] == 1)) & (want["inst"] >= 0)
    assert np.array_equal(perm[got["face"][own]], want["face"][own]) and np.array_equal(got["face"][~own], want["face"][~own])
    order = np.array([4, 0, 3, 6, 1, 2, 7, 9, 10, 8])                            # without instance 5, the tied copy of 4
    got = draw(s, device, order=order)
    for k in ("rgb", "depth", "label", "face"):
        assert same_bits(got[k], want[k]), k
    assert np.array_equal(np.where(got["inst"] >= 0, order[np.maximum(got["inst"], 0)], -1), want["inst"])
    assert np.array_equal(got["visible"], want["visible"][order])


def test_full_size_frames_of_occluding_spheres(device):
    """B = 2 frames of 480 x 640, four subdivision-4 icospheres (5120 faces each), in each frame a nearer sphere partly in front
    of a farther one (their depth ranges do not meet).  Also drawn one instance per frame (B = 4) to know each sphere's own
    silhouette."""
    B, H, W = 2, 480, 640
    K = synth.LINEMOD_K
    meshes = [None, synth.sphere_mesh(4, 0.10, seed=1), synth.sphere_mesh(4, 0.08, seed=2)]
    rng = np.random.RandomState(3)
    inst = [(0, 1, render_ref.pose([0.00, 0.02, 1.10], synth.random_rotation(rng))),
            (0, 2, render_ref.pose([0.07, 0.05, 0.80], synth.random_rotation(rng))),      # nearer, overlaps instance 0
            (1, 2, render_ref.pose([-0.15, -0.10, 0.62], synth.random_rotation(rng))),    # nearer, overlaps instance 3
            (1, 1, render_ref.pose([-0.10, -0.05, 0.95], synth.random_rotation(rng)))]
    T, frame_of, class_of = np.stack([t for _, _, t in inst]), [b for b, _, _ in inst], [c for _, c, _ in inst]
    prepared = render.PreparedMeshes(meshes, device)
    got = {}
    for form in (0, 1):
        prev = render.set_form(form)
        try:
            got[form] = render.render(prepared, T, frame_of, class_of, K, B, H, W, outputs=ALL)
        finally:
            render.set_form(prev)
    for k in ALL:
        assert torch.equal(got[0][k], got[1][k]), k
    out = {k: v.cpu().numpy() for k, v in got[0].items()}
    alone = render.render(prepared, T, [0, 1, 2, 3], class_of, K, 4, H, W, outputs=("inst",))["inst"].cpu().numpy() == np.arange(4)[:, None, None]
    # the nearer sphere owns the overlap, the farther one the rest of its own silhouette
    for b, near, far in ((0, 1, 0), (1, 2, 3)):
        both = alone[near] & alone[far]
        assert both.sum() > 500 and (alone[far] & ~both).sum() > 500
        assert (out["inst"][b][alone[near]] == near).all()
        assert (out["inst"][b][alone[far] & ~alone[near]] == far).all()
        assert (out["inst"][b][~(alone[near] | alone[far])] == -1).all()
    assert np.array_equal(out["label"], np.where(out["inst"] >= 0, np.asarray(class_of)[np.maximum(out["inst"], 0)], 0))
    assert np.array_equal(out["visible"], np.bincount(out["inst"][out["inst"] >= 0], minlength=4))
    assert (out["depth"][out["inst"] < 0] == 0).all() and not (out["rgb"] * (out["inst"] < 0)[:, None]).any()
    # back-projected and taken back into the mesh's frame, every pixel lies between the inscribed sphere of the mesh's faces
    # and the sphere through its vertices; 1e-5 m for the float32 depth and cloud at <= 2 m
    cloud = inputs.depth_to_cloud(got[0]["depth"], K).cpu().numpy().astype(np.float64)          # [B,3,H,W]
    for i, (b, c, Ti) in enumerate(inst):
        v, f = meshes[c]["xyz"].astype(np.float64), meshes[c]["faces"]
        n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        r_in = (np.einsum("ij,ij->i", n, v[f[:, 0]]) / np.linalg.norm(n, axis=1)).min()
        r_out = np.linalg.norm(v, axis=1).max()
        assert 0.9 * r_out < r_in < r_out
        p = cloud[b][:, out["inst"][b] == i].T                                    # [n,3] camera frame
        q = (p - Ti[:, 3]) @ Ti[:, :3]                                            # R^T (p - t)
        r = np.linalg.norm(q, axis=1)
        assert len(r) == out["visible"][i] and len(r) > 2000
        assert r.min() >= r_in - 1e-5 and r.max() <= r_out + 1e-5, (i, r.min() - r_in, r.max() - r_out)


def test_rendered_frames_go_through_the_training_batch_builder(device):
    """"fuse": two objects in front of a backdrop in each of two frames; render_synthetic's rgb / depth / label are what
    assemble_training_batch takes, and the labels it samples are the rendered label image at the chosen pixels."""
    B, H, W, n_points = 2, 120, 160, 1024
    K = synth.LINEMOD_K * [[0.25], [0.25], [1.0]]
    meshes = [None, synth.sphere_mesh(3, 0.10, seed=1), synth.sphere_mesh(2, 0.07, seed=2), render_ref.quad_mesh(-2, -2, 2, 2, 0.0, seed=3)]
    inst = [(0, 3, [0.0, 0.0, 1.5]), (0, 1, [-0.05, 0.0, 0.9]), (0, 2, [0.06, 0.03, 0.7]),
            (1, 3, [0.0, 0.0, 1.4]), (1, 1, [0.1, -0.05, 1.0]), (1, 2, [2.0, 0.0, 0.7])]              # the last one is out of view
    T = np.stack([render_ref.pose(t) for _, _, t in inst])
    frame_of, class_of = [b for b, _, _ in inst], [c for _, c, _ in inst]
    rgb, depth, label, ok = train_data.render_synthetic(meshes, T, frame_of, class_of, K, B, H, W, depth_scale=1000.0, min_visible=50)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (B, 3, H, W) and depth.dtype == torch.float32 and label.dtype == torch.int32
    assert ok.cpu().tolist() == [True, True, True, True, True, False]
    plain = render.render(meshes, T, frame_of, class_of, K, B, H, W)
    assert torch.equal(plain["rgb"], rgb) and torch.equal(plain["depth"] * 1000.0, depth) and torch.equal(plain["label"], label)
    assert (label > 0).all() and set(np.unique(label.cpu().numpy())) == {1, 2, 3}
    RTs = np.stack([T[[1, 2]], T[[4, 5]]])
    kps = np.zeros((4, 8, 3), np.float32)
    out = train_data.assemble_training_batch(rgb, depth, label, K, n_points, [[1, 2], [1, 2]], RTs, kps, np.zeros((4, 3), np.float32),
                                             cam_scale=1000.0, seed=5)
    choose = out["choose"].reshape(B, -1).long()
    assert torch.equal(out["labels"], label.reshape(B, -1).gather(1, choose))
    assert torch.equal(out["rgb_labels"], label) and len(torch.unique(out["labels"])) == 3
