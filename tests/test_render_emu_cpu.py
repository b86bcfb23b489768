"""csrc/render.hip on the SIMT emulator (tests/simt), without a GPU: the unmodified kernel source compiled for the host and run
through the C ABI of include/ffb6d_render.h on the small scene of tests/render_ref.py.  Every output equals the numpy
restatement bit for bit, in both forms of the raster pass; argument errors return their code and write nothing."""
import numpy as np
import pytest

import render_ref
from tests.simt.build import load, ptr as _p

OUTPUTS = ("rgb", "depth", "label", "inst", "face", "visible")


@pytest.fixture(scope="module")
def emu_render():
    """the emulated library (tests/simt/build.py)"""
    return load()


@pytest.fixture(scope="module")
def scene():
    s = render_ref.small_scene()
    want = render_ref.render(s["meshes"], s["T"], s["frame_of"], s["class_of"], s["K"], s["B"], s["H"], s["W"])
    for v in want.values():
        v.setflags(write=False)
    return s, want


def fresh_outputs(n_inst, B, H, W, fill=7):
    return dict(rgb=np.full((B, 3, H, W), fill, np.uint8), depth=np.full((B, H, W), fill, np.float32),
                label=np.full((B, H, W), fill, np.int32), inst=np.full((B, H, W), fill, np.int32),
                face=np.full((B, H, W), fill, np.int32), visible=np.full(n_inst, fill, np.int32))


def call(lib, pk, s, out, z_near=1e-3, ws=None, **kw):
    """ffb6d_render_f32 with numpy arrays as "device" memory; kw overrides arguments by name"""
    B, H, W, n_inst = s["B"], s["H"], s["W"], len(s["frame_of"])
    a = dict(verts=_p(pk["verts"]), colors=_p(pk["colors"]), faces=_p(pk["faces"]), vert_begin=_p(pk["vert_begin"]),
             face_begin=_p(pk["face_begin"]), n_cls=pk["n_cls"], Vtot=pk["Vtot"], Ftot=pk["Ftot"], max_verts=pk["max_verts"],
             max_faces=pk["max_faces"], frame_of=_p(s["frame_of"]), class_of=_p(s["class_of"]), T=_p(s["T"]), I=n_inst, K=_p(s["K"]),
             B=B, H=H, W=W, z_near=z_near)
    a.update({k: _p(out.get(k)) for k in OUTPUTS})
    a.update(kw)
    if ws is None:
        ws = np.zeros(max(lib.ffb6d_render_workspace_bytes(a["I"], a["max_verts"], a["B"], a["H"], a["W"]), 1), np.uint8)
    a.setdefault("workspace", _p(ws))
    a.setdefault("workspace_bytes", ws.nbytes)
    return lib.ffb6d_render_f32(*a.values(), None)


def assert_same_bits(got, want, what=""):
    for k in OUTPUTS:
        if k in got:
            g, w = got[k], want[k]
            assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
            assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w), \
                (what, k, int(np.count_nonzero(g != w)))


def test_scene_has_what_it_is_meant_to_test(scene):
    s, want = scene
    vis = want["visible"]
    assert (vis[[0, 1, 2, 3, 4, 6]] > 0).all() and (vis[[5, 7, 8, 9, 10]] == 0).all(), vis
    assert (want["inst"][1] >= 0).all() and (want["inst"][0] < 0).any()            # the quad fills frame 1; frame 0 has background
    assert set(np.unique(want["label"])) == {0, 1, 2, 3, 5}
    assert not np.isin(want["face"][want["inst"] == 1], [2, 3, 5]).any()           # the near-plane face and the degenerate ones
    assert 0 < vis[6] < vis[2]                                                     # cut by the border


@pytest.mark.parametrize("form", [0, 1, -1])
def test_every_output_on_the_emulator_equals_the_restatement_as_bits(emu_render, scene, form):
    lib = emu_render
    s, want = scene
    pk = render_ref.pack(s["meshes"])
    out = fresh_outputs(len(s["frame_of"]), s["B"], s["H"], s["W"])
    lib.ffb6d_render_set_form(form)
    try:
        assert call(lib, pk, s, out) == 0, lib.ffb6d_last_error()
    finally:
        lib.ffb6d_render_set_form(0)
    assert_same_bits(out, want, form)


def test_outputs_are_optional_and_tables_are_clamped(emu_render, scene):
    lib = emu_render
    s, want = scene
    pk = render_ref.pack(s["meshes"])
    n_inst = len(s["frame_of"])
    for keep in (("depth",), ("visible",), ("rgb", "face")):
        out = {k: v for k, v in fresh_outputs(n_inst, s["B"], s["H"], s["W"]).items() if k in keep}
        assert call(lib, pk, s, out) == 0, lib.ffb6d_last_error()
        assert_same_bits(out, want, keep)
    # a face that names no vertex of its class is dropped, a table that runs past the arrays is cut: the same as a mesh set
    # without that face / those rows
    meshes = list(s["meshes"])
    bad = dict(meshes[3], faces=np.concatenate([meshes[3]["faces"], [[0, 1, 6], [0, -1, 2]]]).astype(np.int32))
    pk_bad = render_ref.pack(meshes[:3] + [bad] + meshes[4:])
    pk_bad["vert_begin"][-1] += 1000
    pk_bad["face_begin"][-1] += 1000
    out = fresh_outputs(n_inst, s["B"], s["H"], s["W"])
    assert call(lib, pk_bad, s, out) == 0, lib.ffb6d_last_error()
    assert_same_bits(out, want, "bad face")
    # no instances: empty frames
    out = fresh_outputs(0, s["B"], s["H"], s["W"])
    assert call(lib, pk, s, out, I=0) == 0, lib.ffb6d_last_error()
    assert not out["rgb"].any() and not out["depth"].any() and not out["label"].any()
    assert (out["inst"] == -1).all() and (out["face"] == -1).all()


def test_argument_errors_return_their_code_and_leave_the_outputs_untouched(emu_render, scene):
    lib = emu_render
    s, _ = scene
    pk = render_ref.pack(s["meshes"])
    n_inst = len(s["frame_of"])
    small = np.zeros(64, np.uint8)
    cases = [(dict(I=1025), -1, "bad sizes"), (dict(B=0), -1, "bad sizes"), (dict(H=1 << 16, W=1 << 16), -1, "bad sizes"),
             (dict(n_cls=0), -1, "bad mesh set"), (dict(max_verts=pk["Vtot"] + 1), -1, "bad mesh set"),
             (dict(max_faces=(1 << 22) + 1, Ftot=1 << 23), -1, "2^22"), (dict(z_near=0.0), -1, "z_near"),
             (dict(z_near=float("nan")), -1, "z_near"), (dict(T=None), -1, "null pointer"), (dict(faces=None), -1, "null pointer"),
             (dict(rgb=None, depth=None, label=None, inst=None, face=None, visible=None), -1, "no output"),
             (dict(workspace=None), -3, "workspace"), (dict(workspace=_p(small), workspace_bytes=64), -3, "workspace")]
    for kw, code, text in cases:
        out = fresh_outputs(n_inst, s["B"], s["H"], s["W"])
        assert call(lib, pk, s, out, **kw) == code, kw
        assert text in lib.ffb6d_last_error().decode(), (kw, lib.ffb6d_last_error())
        for k, v in out.items():
            assert (v == 7).all(), (kw, k)
    assert not small.any()
