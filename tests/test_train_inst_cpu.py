"""Per-instance pose targets without a GPU (csrc/train_inst.hip, include/ffb6d_train.h: ffb6d_pose_targets_inst): the kernels run
through the SIMT emulator (tests/simt) against the numpy restatement of tests/train_inst_ref.py bit for bit, against the existing
ffb6d_pose_targets where both are defined, and on the case that existing call cannot represent; guard words around every
output, a workspace full of NaN bytes, and every argument error."""
import numpy as np
import pytest

import train_inst_ref as tr
from tests.simt.build import load, ptr as _p

DTYPES = dict(labels=np.int32, inst_of_point=np.int32, kp_targ_ofst=np.float32, ctr_targ_ofst=np.float32, kp_3ds=np.float32,
              ctr_3ds=np.float32, n_points=np.int32)
SENTINEL = 7


@pytest.fixture(scope="module")
def emu_inst():
    """the emulated library (tests/simt/build.py)"""
    return load()


def emu_pose_targets(lib, cld, choose, label_img, cls_ids, RTs, kps, ctr):
    """the existing ffb6d_pose_targets on the same emulator build"""
    B, N = choose.shape
    O, K = cls_ids.shape[1], kps.shape[1]
    out = dict(labels=np.zeros((B, N), np.int32), kp_targ_ofst=np.full((B, N, K, 3), 7, np.float32),
               ctr_targ_ofst=np.full((B, N, 3), 7, np.float32), kp_3ds=np.full((B, O, K, 3), 7, np.float32),
               ctr_3ds=np.full((B, O, 3), 7, np.float32), RTs=np.full((B, O, 3, 4), 7, np.float32),
               cls_ids=np.full((B, O, 1), 7, np.int32))
    rc = lib.ffb6d_pose_targets(_p(cld), _p(choose), int(choose.dtype == np.int64), _p(label_img), int(label_img.dtype == np.uint8),
                                _p(cls_ids), _p(RTs), int(RTs.dtype == np.float64), _p(kps), _p(ctr), len(kps), B, N,
                                label_img[0].size, O, K, _p(out["labels"]), _p(out["kp_targ_ofst"]), _p(out["ctr_targ_ofst"]),
                                _p(out["kp_3ds"]), _p(out["ctr_3ds"]), _p(out["RTs"]), _p(out["cls_ids"]), None)
    return rc, out


def shapes(c):
    B, N = c["choose"].shape
    n_inst, K = len(c["frame_of"]), c["mesh_kps"].shape[1]
    return dict(labels=(B, N), inst_of_point=(B, N), kp_targ_ofst=(B, N, K, 3), ctr_targ_ofst=(B, N, 3), kp_3ds=(n_inst, K, 3),
                ctr_3ds=(n_inst, 3), n_points=(n_inst,))


def guarded(shape, dtype, guard):
    """(whole buffer, view of `shape` `guard` elements into it), everything filled with the sentinel"""
    n = int(np.prod(shape))
    buf = np.full(n + 2 * guard, SENTINEL, dtype)
    return buf, buf[guard:guard + n].reshape(shape)


def guards_intact(buf, guard):
    return (buf[:guard] == SENTINEL).all() and (buf[len(buf) - guard:] == SENTINEL).all()


def emu_call(lib, c, guard=16, ws_bytes=None, **override):
    """One call with guarded outputs and a workspace of NaN bytes (itself guarded) -> (rc, outputs, guards all intact)."""
    B, N = c["choose"].shape
    n_inst, K = len(c["frame_of"]), c["mesh_kps"].shape[1]
    bufs = {k: guarded(s, DTYPES[k], guard) for k, s in shapes(c).items()}
    need = lib.ffb6d_pose_targets_inst_workspace_bytes(n_inst, K)
    ws = np.full(need + 64, 0xFF, np.uint8)                               # all ones: NaN as a double
    ws_view = ws[32:32 + need]
    a = dict(cld=_p(c["cld"]), choose=_p(c["choose"]), choose_i64=int(c["choose"].dtype == np.int64), inst_img=_p(c["inst_img"]),
             frame_of=_p(c["frame_of"]), class_of=_p(c["class_of"]), poses=_p(c["poses"]), mesh_kps=_p(c["mesh_kps"]),
             mesh_ctr=_p(c["mesh_ctr"]), n_cls=len(c["mesh_kps"]), B=B, N=N, HW=c["inst_img"].shape[1], I=n_inst, K=K,
             labels=_p(bufs["labels"][1]), inst_of_point=_p(bufs["inst_of_point"][1]), kp_targ_ofst=_p(bufs["kp_targ_ofst"][1]),
             ctr_targ_ofst=_p(bufs["ctr_targ_ofst"][1]), kp_3ds=_p(bufs["kp_3ds"][1]), ctr_3ds=_p(bufs["ctr_3ds"][1]),
             n_points=_p(bufs["n_points"][1]), workspace=_p(ws_view) if need else None,
             workspace_bytes=need if ws_bytes is None else ws_bytes, stream=None)
    a.update(override)
    rc = lib.ffb6d_pose_targets_inst(*a.values())
    ok = all(guards_intact(b, guard) for b, _ in bufs.values()) and (ws[:32] == 0xFF).all() and (ws[32 + need:] == 0xFF).all()
    return rc, {k: v for k, (_, v) in bufs.items()}, ok


def assert_equal_bits(got, want, what):
    for k in tr.OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), (what, k)


def test_the_case_holds_what_it_is_meant_to_hold():
    c, ref = tr.case_and_reference(70, 8)
    I, HW = 70, tr.H * tr.W
    assert ref["n_points"][3] == 0 and not (c["inst_img"] == 3).any()                       # owns no point
    wrong = (c["inst_img"] == 4) & (np.arange(tr.B)[:, None] != c["frame_of"][4])
    assert wrong.any()                                                                       # painted into another frame
    assert c["class_of"][5] == 0 and c["class_of"][6] == tr.N_CLS and (c["inst_img"] == 5).any() and (c["inst_img"] == 6).any()
    assert not ref["kp_3ds"][5].any() and not ref["kp_3ds"][6].any() and ref["n_points"][5] == 0 and ref["n_points"][6] == 0
    assert (c["inst_img"] == -1).any() and (c["inst_img"] >= I).any()
    assert (c["choose"] == -1).any() and (c["choose"] == HW).any()
    assert ref["n_points"].sum() == (ref["labels"] > 0).sum() == (ref["inst_of_point"] >= 0).sum() > 1000
    assert (ref["n_points"] > 0).sum() > 40
    # a point that samples a wrongly painted pixel belongs to nothing
    b, px = np.argwhere(wrong)[0]
    hit = np.nonzero(c["choose"][b] == px)[0]
    assert all(ref["inst_of_point"][b, n] == -1 for n in hit)


@pytest.mark.parametrize("choose_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("K", [1, 8, 64])
@pytest.mark.parametrize("n_inst", [0, 1, 70])
def test_every_output_equals_the_restatement_bit_for_bit(emu_inst, n_inst, K, choose_dtype):
    c, ref = tr.case_and_reference(n_inst, K)
    c = dict(c, choose=c["choose"].astype(choose_dtype))
    rc, out, ok = emu_call(emu_inst, c)
    assert rc == 0, emu_inst.ffb6d_last_error()
    assert ok, "a guard word or the workspace's surroundings were written"
    assert_equal_bits(out, ref, (n_inst, K, choose_dtype))


def test_offset_rows_that_are_not_16_byte_aligned_take_the_single_float_stores(emu_inst):
    """K = 8 rows are whole 16-byte units, so the aligned buffer above took the wide stores; one guard float in front moves the rows
    off that alignment and the same bits must come out of the other form."""
    c, ref = tr.case_and_reference(70, 8)
    rc, out, ok = emu_call(emu_inst, c, guard=1)
    assert rc == 0 and ok
    assert out["kp_targ_ofst"].ctypes.data % 16 != 0
    assert_equal_bits(out, ref, "unaligned")


def test_one_instance_per_class_and_frame_gives_the_bits_of_pose_targets(emu_inst):
    c, slots = tr.one_per_class_case(K=8)
    rc, out, ok = emu_call(emu_inst, c)
    assert rc == 0 and ok
    rc, old = emu_pose_targets(emu_inst, c["cld"], c["choose"], slots["label_img"], slots["cls_ids"], slots["RTs"], c["mesh_kps"],
                               c["mesh_ctr"])
    assert rc == 0
    assert (out["labels"] > 0).sum() > 1000 and len(set(out["labels"].ravel())) == tr.N_CLS
    for k in ("labels", "kp_targ_ofst", "ctr_targ_ofst"):
        assert np.array_equal(out[k].view(np.int32), old[k].view(np.int32)), k
    for b in range(tr.B):                                                                   # and the posed keypoints, slot by slot
        own = np.nonzero(c["frame_of"] == b)[0]
        assert np.array_equal(out["kp_3ds"][own], old["kp_3ds"][b, :len(own)])
        assert np.array_equal(out["ctr_3ds"][own], old["ctr_3ds"][b, :len(own)])


def test_two_instances_of_one_class_keep_their_own_keypoints_where_pose_targets_gives_both_the_last_slot(emu_inst):
    c, slots = tr.two_of_a_class_case(K=8)
    rc, new, ok = emu_call(emu_inst, c)
    assert rc == 0 and ok
    rc, old = emu_pose_targets(emu_inst, c["cld"], c["choose"], slots["label_img"], slots["cls_ids"], slots["RTs"], c["mesh_kps"],
                               c["mesh_ctr"])
    assert rc == 0
    assert np.array_equal(new["labels"], old["labels"])
    first, second = new["inst_of_point"][0] == 0, new["inst_of_point"][0] == 2              # both of class 2
    assert first.sum() > 100 and second.sum() > 100 and new["n_points"].tolist() == [first.sum(), (new["inst_of_point"][0] == 1).sum(), second.sum()]
    cld = c["cld"][0].astype(np.float64)
    # the gap: pose_targets points every class-2 point at the LAST class-2 slot's keypoints
    assert np.array_equal(old["kp_3ds"][0], new["kp_3ds"])
    for sel in (first, second):
        assert np.allclose(cld[sel][:, None] - old["kp_targ_ofst"][0][sel], new["kp_3ds"][2], atol=1e-6)
        assert np.allclose(cld[sel] - old["ctr_targ_ofst"][0][sel], new["ctr_3ds"][2], atol=1e-6)
    # the new call gives each its own
    assert np.allclose(cld[first][:, None] - new["kp_targ_ofst"][0][first], new["kp_3ds"][0], atol=1e-6)
    assert np.allclose(cld[second][:, None] - new["kp_targ_ofst"][0][second], new["kp_3ds"][2], atol=1e-6)
    assert np.allclose(cld[first] - new["ctr_targ_ofst"][0][first], new["ctr_3ds"][0], atol=1e-6)
    assert np.abs(new["kp_3ds"][0] - new["kp_3ds"][2]).max() > 0.1                           # and they are far apart
    assert np.array_equal(new["kp_targ_ofst"][0][second], old["kp_targ_ofst"][0][second])    # the last slot's points agree
    assert not np.array_equal(new["kp_targ_ofst"][0][first], old["kp_targ_ofst"][0][first])


def test_workspace_query(native_lib):
    f = native_lib.ffb6d_pose_targets_inst_workspace_bytes
    assert f(0, 8) == 0 and f(-1, 8) == 0 and f(4, 0) == 0
    assert f(1, 1) == 256 and f(70, 8) == (70 * 9 * 24 + 255) // 256 * 256 and f(1024, 64) == 1024 * 65 * 24


def test_every_argument_error_returns_its_code_and_writes_nothing(emu_inst):
    c, _ = tr.case_and_reference(70, 8)
    need = emu_inst.ffb6d_pose_targets_inst_workspace_bytes(70, 8)
    bad = [(-1, dict(B=-1)), (-1, dict(N=-1)), (-1, dict(HW=-1)), (-1, dict(n_cls=0)), (-1, dict(K=0)), (-1, dict(K=65)),
           (-1, dict(I=-1)), (-1, dict(I=1025)), (-1, dict(B=65536)), (-3, dict(workspace=None)), (-3, dict(ws_bytes=need - 1)),
           (-3, dict(ws_bytes=0))]
    bad += [(-1, {k: None}) for k in ("cld", "choose", "inst_img", "frame_of", "class_of", "poses", "mesh_kps", "mesh_ctr", "labels",
                                      "inst_of_point", "kp_targ_ofst", "ctr_targ_ofst", "kp_3ds", "ctr_3ds", "n_points")]
    for code, over in bad:
        ws_bytes = over.pop("ws_bytes", None)
        rc, out, ok = emu_call(emu_inst, c, ws_bytes=ws_bytes, **over)
        assert rc == code, (over, rc, emu_inst.ffb6d_last_error())
        assert emu_inst.ffb6d_last_error()
        assert ok and all((v == SENTINEL).all() for v in out.values()), over
    # a workspace that is large enough but not 8-byte aligned
    rc, out, ok = emu_call(emu_inst, c, workspace=_p(np.zeros(need + 16, np.uint8)[4:]))
    assert rc == -3 and all((v == SENTINEL).all() for v in out.values())
    # nothing to do is no error: no instances and no points
    empty = dict(c, cld=c["cld"][:, :0], choose=c["choose"][:, :0], frame_of=c["frame_of"][:0], class_of=c["class_of"][:0],
                 poses=c["poses"][:0])
    rc, out, ok = emu_call(emu_inst, empty)
    assert rc == 0 and ok


def test_python_wrapper_refuses_cpu_tensors_and_bad_host_ids():
    import torch
    from ffb6d_amd import _lib, train_data
    c, _ = tr.case_and_reference(1, 8)
    t = {k: torch.from_numpy(np.array(v)) for k, v in c.items()}
    with pytest.raises(_lib.FFB6DNativeError):
        train_data.pose_targets_instances(t["cld"], t["choose"], t["inst_img"].reshape(tr.B, tr.H, tr.W), c["frame_of"], c["class_of"],
                                          c["poses"], c["mesh_kps"], c["mesh_ctr"])
    for name, hi, vals in (("frame_of", tr.B, [0, tr.B]), ("class_of", tr.N_CLS, [1, -1]), ("class_of", tr.N_CLS, [tr.N_CLS, 1])):
        with pytest.raises(ValueError, match=name):
            train_data._instance_ids(np.asarray(vals), name, hi, "cpu")
    assert train_data._instance_ids(np.asarray([0, 2, 1]), "frame_of", 3, "cpu").dtype == torch.int32
    kp = torch.arange(2 * 5 * 3 * 3, dtype=torch.float32).reshape(2, 5, 3, 3)
    ctr_of, kp_of = train_data.votes_from_targets(dict(kp_targ_ofst=kp, ctr_targ_ofst=kp[:, :, 0]))
    assert tuple(ctr_of.shape) == (2, 1, 5, 3) and tuple(kp_of.shape) == (2, 3, 5, 3)
    assert torch.equal(kp_of[1, 2, 4], kp[1, 4, 2]) and torch.equal(ctr_of[1, 0, 3], kp[1, 3, 0])


def test_instance_scene_keeps_its_promises():
    """synth.make_instance_scene, seed 0 (the scene of the closed loop in tests/test_train_inst_gpu.py), drawn by the numpy
    rasteriser: instance centres at least 4 solver bandwidths and two object radii apart, every instance whole inside the frame and
    unoccluded, meshes without a symmetry, and enough pixels that each instance owns at least 100 of 2048 sampled points."""
    import render_ref
    from ffb6d_amd import pose, synth
    s = synth.make_instance_scene(0)
    again = synth.make_instance_scene(0)
    assert np.array_equal(s["poses"], again["poses"]) and np.array_equal(s["meshes"][1]["xyz"], again["meshes"][1]["xyz"])
    assert s["class_of"].tolist() == [1, 1, 1, 2, 1, 1] and s["frame_of"].tolist() == [0, 0, 0, 0, 1, 1]
    assert s["poses"].dtype == np.float64 and s["frame_of"].dtype == np.int32 and tuple(s["K"].shape) == (2, 3, 3)
    t, radius = s["poses"][:, :, 3], float(s["r_lst"].max())
    assert abs(radius - 0.08) < 1e-6
    for i in range(6):
        for j in range(i):
            if s["frame_of"][i] == s["frame_of"][j]:
                assert np.linalg.norm(t[i] - t[j]) >= max(4 * pose.RADIUS, 2 * radius)
    out = render_ref.render(s["meshes"], s["poses"], s["frame_of"], s["class_of"], s["K"], 2, 120, 160)
    for i in range(6):
        alone = render_ref.render(s["meshes"], s["poses"][i:i + 1], [s["frame_of"][i]], [s["class_of"][i]], s["K"], 2, 120, 160)
        assert out["visible"][i] == alone["visible"][0] > 200                             # nothing hides it
        rows, cols = np.nonzero(alone["depth"][s["frame_of"][i]] > 0)
        assert 0 < rows.min() and rows.max() < 119 and 0 < cols.min() and cols.max() < 159  # the frame's border cuts nothing off
    drawn = (out["depth"] > 0).reshape(2, -1).sum(1)
    share = [2048 * out["visible"][i] / drawn[s["frame_of"][i]] for i in range(6)]
    assert min(share) >= 300, share                                                       # expected points of 2048: far above 100
    for c in (1, 2):                                                                      # no axis flip maps the vertex set onto itself
        v = s["meshes"][c]["xyz"].astype(np.float64)
        for flip in ([-1, 1, 1], [1, -1, 1], [1, 1, -1], [-1, -1, 1], [-1, 1, -1], [1, -1, -1], [-1, -1, -1]):
            d = np.linalg.norm(v[:, None] - (v * flip)[None], axis=2).min(1)
            assert d.max() > 0.05 * radius, (c, flip)
    assert np.array_equal(s["mesh_ctr"][1], (s["meshes"][1]["xyz"].min(0) + s["meshes"][1]["xyz"].max(0)) / 2)
