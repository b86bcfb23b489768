"""The rasteriser without a GPU (ffb6d_amd/render.py, csrc/render.hip, include/ffb6d_render.h): the library exports the header's
entry points and validates their arguments before any HIP call, the Python layer refuses CPU tensors, and the numpy
restatement the device is held against (tests/render_ref.py) agrees with closed forms: an axis-aligned quad whose covered
set and depth are known exactly, edges and vertices that pass exactly through pixel samples (each such sample is owned once)."""
import itertools

import numpy as np
import pytest
import torch

import render_ref
from ffb6d_amd import synth

ENTRY_POINTS = ("ffb6d_render_workspace_bytes", "ffb6d_render_set_form", "ffb6d_render_f32")
# u = 128 X + 32, v = 128 Y + 24 at Z = 0.5: a pixel coordinate that is a multiple of 1/256 comes from an exact float32 X
K_EXACT = np.array([[64.0, 0.0, 32.0], [0.0, 64.0, 24.0], [0.0, 0.0, 1.0]])
D, H, W = 0.5, 48, 64


def at_pixel(u, v, z=D):
    """the point (metres) that projects to pixel coordinates (u, v) under K_EXACT at depth z"""
    return [(u - 32.0) * z / 64.0, (v - 24.0) * z / 64.0, z]


def one_mesh(points, faces, seed=0):
    xyz = np.asarray(points, np.float32)
    assert np.array_equal(xyz.astype(np.float64), np.asarray(points, np.float64))      # exact in float32
    return dict(xyz=xyz, rgb=np.random.RandomState(seed).randint(0, 256, xyz.shape).astype(np.uint8), faces=np.asarray(faces, np.int32))


def draw(mesh):
    return render_ref.render([None, mesh], [render_ref.pose([0.0, 0.0, 0.0])], [0], [1], K_EXACT, 1, H, W)


def test_library_exports_the_render_entry_points(native_lib):
    from ffb6d_amd import _lib
    for name in ENTRY_POINTS:
        assert hasattr(native_lib, name) and name in _lib.SIGNATURES, name


def test_sizes_and_argument_errors_are_host_logic(native_lib):
    from ffb6d_amd import _lib
    a256 = lambda n: (n + 255) // 256 * 256                                      # noqa: E731
    assert native_lib.ffb6d_render_workspace_bytes(40, 10242, 8, 480, 640) == a256(8 * 8 * 480 * 640) + a256(16 * 40 * 10242)
    assert native_lib.ffb6d_render_workspace_bytes(0, 0, 1, 3, 5) == 256
    for bad in ((1025, 10, 1, 8, 8), (-1, 10, 1, 8, 8), (1, 10, 0, 8, 8), (1, 10, 1, 1 << 16, 1 << 15), (1, -1, 1, 8, 8)):
        assert native_lib.ffb6d_render_workspace_bytes(*bad) == 0, bad
    for form in (1, -1, 0):
        native_lib.ffb6d_render_set_form(form)
    ok = dict(verts=64, colors=64, faces=64, vert_begin=64, face_begin=64, n_cls=3, Vtot=100, Ftot=150, max_verts=60, max_faces=90,
              frame_of=64, class_of=64, T=64, I=4, K=64, B=2, H=48, W=64, z_near=1e-3, rgb=64, depth=None, label=None, inst=None,
              face=None, visible=None, ws=None, ws_bytes=0, stream=None)

    def call(**kw):
        return native_lib.ffb6d_render_f32(*dict(ok, **kw).values())

    assert call(I=1025) == -1 and "bad sizes" in _lib.last_error()
    assert call(W=0) == -1 and "bad sizes" in _lib.last_error()
    assert call(B=1 << 12, H=1 << 10, W=1 << 10) == -1 and "bad sizes" in _lib.last_error()
    assert call(n_cls=0) == -1 and "bad mesh set" in _lib.last_error()
    assert call(max_faces=151) == -1 and "bad mesh set" in _lib.last_error()
    assert call(Ftot=1 << 23, max_faces=(1 << 22) + 1) == -1 and "2^22" in _lib.last_error()
    assert call(z_near=0.0) == -1 and "z_near" in _lib.last_error()
    assert call(rgb=None) == -1 and "no output" in _lib.last_error()
    assert call(colors=None) == -1 and "null pointer" in _lib.last_error()
    assert call(K=None) == -1 and "null pointer" in _lib.last_error()
    assert call() == -3 and "workspace" in _lib.last_error()                      # too small: reported, nothing launched


def test_python_layer_refuses_cpu_tensors_and_bad_requests():
    from ffb6d_amd import _lib, render, train_data
    mesh = synth.sphere_mesh(0)
    T = torch.zeros(1, 3, 4, dtype=torch.float64)
    with pytest.raises(_lib.FFB6DNativeError):
        render.render([None, mesh], T, [0], [1], synth.LINEMOD_K, 1, 48, 64)
    with pytest.raises(_lib.FFB6DNativeError):
        render.render([None, mesh], T.numpy(), [0], torch.ones(1, dtype=torch.int32), synth.LINEMOD_K, 1, 48, 64)
    with pytest.raises(_lib.FFB6DNativeError):
        train_data.render_synthetic([None, mesh], T, [0], [1], synth.LINEMOD_K, 1, 48, 64)
    with pytest.raises(_lib.FFB6DNativeError):
        render.PreparedMeshes([None, mesh], device="cpu")


def test_sphere_mesh_is_a_closed_outward_wound_icosphere():
    for subdiv in (0, 1, 3):
        m = synth.sphere_mesh(subdiv, 0.07, seed=2)
        v, f = m["xyz"].astype(np.float64), m["faces"]
        assert f.shape == (20 * 4 ** subdiv, 3) and v.shape == (10 * 4 ** subdiv + 2, 3) and m["rgb"].dtype == np.uint8
        assert np.abs(np.linalg.norm(v, axis=1) - 0.07).max() < 1e-8
        n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        assert (np.einsum("ij,ij->i", n, v[f].mean(1)) > 0).all()
        edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()       # every edge belongs to two faces
    assert np.array_equal(synth.sphere_mesh(1, seed=4)["rgb"], synth.sphere_mesh(1, seed=4)["rgb"])


def test_a_facing_quad_covers_its_analytic_rectangle_at_its_depth():
    """Corners at pixel coordinates (10.5, 5.5) .. (40.5, 30.5): no sample lies on an edge, so the covered set is the samples
    strictly inside, columns 11..40 and rows 6..30, whatever the ownership rule; the surface is the plane Z = 0.5."""
    c = [at_pixel(10.5, 5.5), at_pixel(40.5, 5.5), at_pixel(40.5, 30.5), at_pixel(10.5, 30.5)]
    want = np.zeros((H, W), bool)
    want[6:31, 11:41] = True
    for faces in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 1], [0, 3, 2]], [[1, 2, 3], [3, 0, 1]]):
        out = draw(one_mesh(c, faces))
        assert np.array_equal(out["inst"][0] == 0, want)
        assert np.array_equal(out["label"][0] == 1, want) and int(out["visible"][0]) == 25 * 30
        d = out["depth"][0]
        assert (d[~want] == 0).all()
        ulp = np.abs(d[want].view(np.int32).astype(np.int64) - int(np.float32(D).view(np.int32)))
        assert ulp.max() <= 1, ulp.max()
        assert (out["face"][0][~want] == -1).all() and set(np.unique(out["face"][0][want])) == {0, 1}
    # constant colour in, the same colour out: the weights of a sample sum to one up to rounding
    m = one_mesh(c, [[0, 1, 2], [0, 2, 3]])
    m["rgb"][:] = [200, 17, 255]
    rgb = draw(m)["rgb"][0]
    assert (rgb[:, want] == np.array([[200], [17], [255]])).all() and not rgb[:, ~want].any()


def test_samples_on_a_shared_edge_belong_to_exactly_one_triangle():
    """A quad with corners ON pixel samples, (8, 8) .. (24, 24): its diagonal and all four sides pass exactly through samples.
    Each triangle is drawn alone, in both vertex orders: the two masks are disjoint, their union is the quad's mask, and the quad
    owns 16 x 16 samples: of two opposite sides exactly one owns its samples."""
    c = [at_pixel(8, 8), at_pixel(24, 8), at_pixel(24, 24), at_pixel(8, 24)]
    quad = draw(one_mesh(c, [[0, 1, 2], [0, 2, 3]]))["inst"][0] == 0
    rows, cols = np.nonzero(quad)
    assert quad.sum() == 256 and rows.max() - rows.min() == 15 and cols.max() - cols.min() == 15
    assert rows.min() in (8, 9) and cols.min() in (8, 9)
    on_diagonal = np.zeros((H, W), bool)
    on_diagonal[np.arange(9, 24), np.arange(9, 24)] = True
    for first, second in itertools.product(([0, 1, 2], [0, 2, 1], [2, 0, 1]), ([0, 2, 3], [0, 3, 2], [3, 2, 0])):
        a = draw(one_mesh(c, [first]))["inst"][0] == 0
        b = draw(one_mesh(c, [second]))["inst"][0] == 0
        assert not (a & b).any() and np.array_equal(a | b, quad), (first, second)
        assert (a & on_diagonal).sum() + (b & on_diagonal).sum() == 15
        assert (a & on_diagonal).sum() in (0, 15)                                 # one triangle owns the whole edge
    # the other diagonal too
    a = draw(one_mesh(c, [[0, 1, 3]]))["inst"][0] == 0
    b = draw(one_mesh(c, [[3, 2, 1]]))["inst"][0] == 0
    assert not (a & b).any() and np.array_equal(a | b, quad)


def test_a_vertex_on_a_sample_is_owned_once_by_the_fan_around_it():
    """A closed fan around a vertex placed exactly on the sample of pixel (row 12, col 16), with horizontal, vertical and
    oblique spokes: drawn one triangle at a time (in alternating vertex orders), every sample is covered at most once, the
    centre exactly once, and the union is what the whole fan covers."""
    rim = [(26, 12), (22.25, 18.5), (16, 20), (9.5, 17), (7, 12), (9, 5.25), (16, 3), (23, 6)]
    pts = [at_pixel(16, 12)] + [at_pixel(u, v) for u, v in rim]
    n = len(rim)
    faces = [[0, 1 + k, 1 + (k + 1) % n] if k % 2 else [0, 1 + (k + 1) % n, 1 + k] for k in range(n)]
    whole = draw(one_mesh(pts, faces))
    count = np.zeros((H, W), np.int64)
    for f in faces:
        count += draw(one_mesh(pts, [f]))["inst"][0] == 0
    assert count.max() == 1 and count[12, 16] == 1
    assert np.array_equal(count == 1, whole["inst"][0] == 0)
    assert whole["depth"][0, 12, 16] == np.float32(D)
    # the spokes through samples: the horizontal and the vertical one are inside the fan, so their samples are owned too
    assert (count[12, 8:26] == 1).all() and (count[4:20, 16] == 1).all()


def test_the_small_scene_is_order_independent_in_the_restatement():
    """Permuting the faces of a mesh changes only `face`; permuting instances that do not tie changes only `inst` / `visible`."""
    s = render_ref.small_scene()
    args = (s["K"], s["B"], s["H"], s["W"])
    base = render_ref.render(s["meshes"], s["T"], s["frame_of"], s["class_of"], *args)
    perm = np.random.RandomState(0).permutation(len(s["meshes"][1]["faces"]))
    meshes = list(s["meshes"])
    meshes[1] = dict(meshes[1], faces=meshes[1]["faces"][perm])
    got = render_ref.render(meshes, s["T"], s["frame_of"], s["class_of"], *args)
    for k in ("rgb", "depth", "label", "inst", "visible"):
        assert np.array_equal(got[k], base[k]), k
    own = np.isin(base["inst"], np.flatnonzero(s["class_of"] == 1)) & (base["inst"] >= 0)
    assert np.array_equal(perm[got["face"][own]], base["face"][own]) and np.array_equal(got["face"][~own], base["face"][~own])
    order = np.array([4, 0, 3, 6, 1, 2, 7, 9, 10, 8])                            # without instance 5, the tied copy of 4
    got = render_ref.render(s["meshes"], s["T"][order], s["frame_of"][order], s["class_of"][order], *args)
    for k in ("rgb", "depth", "label", "face"):
        assert np.array_equal(got[k], base[k]), k
    assert np.array_equal(np.where(got["inst"] >= 0, order[np.maximum(got["inst"], 0)], -1), base["inst"])
    assert np.array_equal(got["visible"], base["visible"][order])
