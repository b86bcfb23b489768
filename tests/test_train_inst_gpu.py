"""Per-instance pose targets on the MI355X (train_data.pose_targets_instances over csrc/train_inst.hip): the bit-equality cases of
tests/test_train_inst_cpu.py on the device, the closed loop scene -> render -> targets -> votes -> pose.solve_instances ->
bop.BOPSceneEval, and the training-batch builder with `instances`.
No training step here: a random-weight forward and backward on these targets (bs = 1, N = 2048, one 480 x 640 frame) took 31 s as a
test of its own, most of it the first use of new convolution shapes, so it is left out; the loss reads labels, kp_targ_ofst and
ctr_targ_ofst, whose shapes and dtypes are those of pose_targets, and tests/test_train_data_gpu.py runs that step."""
import numpy as np
import pytest
import torch

import pose_instances_ref as pref
import train_inst_ref as tr
from ffb6d_amd import bop, evaluate, inputs, pose, render, synth, train_data

pytestmark = pytest.mark.gpu

N_POINTS = 2048
SEED = 3


def _call(c, device, ids_on_device=True):
    c = {k: np.array(v) for k, v in c.items()}                              # the shared case is read-only
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)                                                    # noqa: E731
    ids = (up(c["frame_of"]), up(c["class_of"])) if ids_on_device else (c["frame_of"], c["class_of"])
    out = train_data.pose_targets_instances(up(c["cld"]), up(c["choose"]), up(c["inst_img"].reshape(tr.B, tr.H, tr.W)), *ids,
                                            c["poses"], c["mesh_kps"], c["mesh_ctr"])
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- bit equality -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("choose_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("K", [1, 8, 64])
@pytest.mark.parametrize("n_inst", [0, 1, 70])
def test_every_output_equals_the_restatement_bit_for_bit(device, n_inst, K, choose_dtype):
    """The cases of the emulator test (bad frames and classes, indices past the list, choose entries outside the image, N = 1061)
    on the device; the ids go up as device tensors, which the wrapper does not read back and the kernel must not index with."""
    c, ref = tr.case_and_reference(n_inst, K)
    out = _call(dict(c, choose=c["choose"].astype(choose_dtype)), device)
    assert set(out) == set(tr.OUTPUTS)
    for k in tr.OUTPUTS:
        assert out[k].dtype == ref[k].dtype and out[k].shape == ref[k].shape, k
        assert np.array_equal(out[k].view(np.int32), ref[k].view(np.int32)), k


def test_one_instance_per_class_and_frame_gives_the_bits_of_pose_targets(device):
    c, slots = tr.one_per_class_case(K=8)
    new = _call(c, device, ids_on_device=False)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)                                                    # noqa: E731
    old = train_data.pose_targets(up(c["cld"]), up(c["choose"]), up(slots["label_img"].reshape(tr.B, tr.H, tr.W)), slots["cls_ids"],
                                  slots["RTs"], c["mesh_kps"], c["mesh_ctr"])
    assert (new["labels"] > 0).sum() > 1000
    for k in ("labels", "kp_targ_ofst", "ctr_targ_ofst"):
        assert np.array_equal(new[k].view(np.int32), old[k].cpu().numpy().view(np.int32)), k


def test_host_ids_out_of_range_raise_before_anything_is_launched(device):
    c, _ = tr.case_and_reference(70, 8)                                    # holds class n_cls
    with pytest.raises(ValueError, match="class_of"):
        _call(c, device, ids_on_device=False)
    with pytest.raises(ValueError, match="frame_of"):
        _call(dict(c, frame_of=np.full(70, tr.B, np.int32)), device, ids_on_device=False)
    with pytest.raises(ValueError, match="poses"):
        _call(dict(c, poses=c["poses"][:5]), device)


# ---- the closed loop --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop(device):
    """2 frames of 120 x 160: three instances of class 1 and one of class 2 in frame 0, two of class 1 in frame 1, rendered,
    sampled (N = 2048) and labelled per instance; plus the same frames through assemble_training_batch(instances=...)."""
    s = synth.make_instance_scene(0)
    assert s["class_of"].tolist() == [1, 1, 1, 2, 1, 1] and s["frame_of"].tolist() == [0, 0, 0, 0, 1, 1] and (s["B"], s["H"], s["W"]) == (2, 120, 160)
    meshes = render.PreparedMeshes(s["meshes"], device)
    rgb, depth, label, ok, inst = train_data.render_synthetic(meshes, s["poses"], s["frame_of"], s["class_of"], s["K"], 2, 120, 160,
                                                               return_inst=True)
    nrm = inputs.depth_normal(depth * 1000.0, s["K"][0, 0, 0], s["K"][0, 1, 1])
    dpt_xyz = inputs.depth_to_cloud(depth, s["K"])
    pts = inputs.sample_points(depth, N_POINTS, dpt_xyz, rgb, nrm, seed=SEED)
    tg = train_data.pose_targets_instances(pts["cld"], pts["choose"], inst, s["frame_of"], s["class_of"], s["poses"], s["mesh_kps"],
                                           s["mesh_ctr"])
    batch = train_data.assemble_training_batch(rgb, depth, label, s["K"], N_POINTS, None, None, s["mesh_kps"], s["mesh_ctr"], normals=nrm,
                                               seed=SEED, instances=dict(inst_img=inst, frame_of=s["frame_of"], class_of=s["class_of"],
                                                                         poses=s["poses"]))
    return dict(s=s, meshes=meshes, rgb=rgb, depth=depth, label=label, inst=inst, nrm=nrm, cld=pts["cld"], choose=pts["choose"], tg=tg,
                batch=batch)


def _add(v, T, G):
    T, G = np.asarray(T, np.float64), np.asarray(G, np.float64)
    return float(np.linalg.norm((v @ T[:, :3].T + T[:, 3]) - (v @ G[:, :3].T + G[:, 3]), axis=1).mean())


def _match(s, rows):
    """rows: (frame, class, RT) of the estimates -> for each the ground-truth instance of its (frame, class) with the nearest
    centre, and the ADD against it over the mesh vertices"""
    out = []
    for b, c, T in rows:
        cand = [i for i in range(len(s["frame_of"])) if s["frame_of"][i] == b and s["class_of"][i] == c]
        i = min(cand, key=lambda i: np.linalg.norm(s["poses"][i][:, 3] - np.asarray(T)[:, 3]))
        out.append((i, _add(s["meshes"][c]["xyz"].astype(np.float64), T, s["poses"][i])))
    return out


def test_render_synthetic_hands_out_the_instance_image(loop):
    s = loop["s"]
    plain = train_data.render_synthetic(loop["meshes"], s["poses"], s["frame_of"], s["class_of"], s["K"], 2, 120, 160)
    assert len(plain) == 4 and torch.equal(plain[0], loop["rgb"]) and torch.equal(plain[2], loop["label"])
    inst = loop["inst"]
    assert inst.dtype == torch.int32 and tuple(inst.shape) == (2, 120, 160)
    cls = torch.from_numpy(np.concatenate([s["class_of"], [0]])).to(inst.device)           # -1 -> the spare entry: background
    assert torch.equal(cls[inst.long()].int(), loop["label"])


def test_scene_to_targets_to_votes_to_solver_to_scene_evaluator(loop, device):
    """The loop that the per-instance targets close.  Every instance owns at least 100 of the 2048 sampled points (a condition of
    the scene, checked, not measured); pose.solve_instances on the votes of a perfect network finds every instance exactly once;
    its ADD stays within 10 x the ADD of the numpy solver (tests/pose_instances_ref.solve_instances) on the same votes, which only
    float rounding of cld - (cld - kp) separates from exact; bop.BOPSceneEval on these estimates and the batch's gt_* rows reports
    recall 1.0 on all three errors.
    Measured on an MI355X (scene seed 0, sampling seed 3): the numpy solver's largest ADD over the six instances 1.53e-07 m, the
    device solver's 3.91e-07 m (bar: 1.53e-06 m); the instances own 480, 634, 409, 525, 1032 and 1016 points."""
    s, tg = loop["s"], loop["tg"]
    n_points = tg["n_points"].cpu().numpy()
    print("n_points", n_points.tolist())
    assert (n_points >= 100).all(), n_points
    assert int(n_points.sum()) == int((tg["labels"] > 0).sum()) == 2 * N_POINTS       # only objects have depth: every point is owned
    ctr_of, kp_of = train_data.votes_from_targets(tg)
    got = pose.solve_instances(loop["cld"], tg["labels"], ctr_of, kp_of, s["mesh_kps"], s["mesh_ctr"], max_instances=4)
    frm, cls, T = got["est_frame"].cpu().numpy(), got["est_class"].cpu().numpy(), got["est_RT"].cpu().numpy()
    print("estimates", list(zip(frm.tolist(), cls.tolist())), "n_inside", got["n_inside"].cpu().tolist())
    found = _match(s, zip(frm, cls, T))
    assert sorted(i for i, _ in found) == list(range(6)), found                        # every instance exactly once
    assert got["n_inside"].cpu().numpy().tolist() == [int(n_points[i]) for i, _ in found]
    # the bar: the numpy solver on the same votes
    rows = pref.solve_instances(loop["cld"].cpu().numpy(), tg["labels"].cpu().numpy(), ctr_of.cpu().numpy(), kp_of.cpu().numpy(),
                                s["mesh_kps"], s["mesh_ctr"], 4)
    ref_found = _match(s, [(r["frame"], r["cls"], r["RT"]) for r in rows])
    assert sorted(i for i, _ in ref_found) == list(range(6))
    ref_add, dev_add = max(a for _, a in ref_found), max(a for _, a in found)
    print("largest ADD: numpy solver", ref_add, "device solver", dev_add)
    assert dev_add <= 10.0 * ref_add, (dev_add, ref_add)
    # the scene evaluator, fed with the batch's ground truth
    b = loop["batch"]
    assert torch.equal(b["gt_RT"].cpu(), torch.from_numpy(s["poses"])) and b["gt_class"].cpu().tolist() == s["class_of"].tolist()
    models = evaluate.ModelPoints([np.zeros((0, 3), np.float32) if m is None else m["xyz"] for m in s["meshes"]], device)
    ev = bop.BOPSceneEval(models, loop["meshes"], bop.SymmetrySets([None] * 3, device), s["diameters"])
    m = ev.add_batch(loop["depth"], s["K"], got["est_RT"], got["est_class"], got["est_frame"], got["est_score"], b["gt_RT"],
                     b["gt_class"], b["gt_frame"])
    assert m["valid"].all()
    out = ev.cal_ar()
    print("recall", {k: out[k] for k in ("ar_vsd", "ar_mssd", "ar_mspd")})
    assert out["n_targets"] == 6 and out["ar_vsd"] == 1.0 and out["ar_mssd"] == 1.0 and out["ar_mspd"] == 1.0


def test_class_label_targets_cannot_separate_the_instances(loop):
    """What the feature is for: the same scene through pose_targets (the class image, one slot per instance) points every class-1
    point of frame 0 at the last class-1 slot, and the solver then finds one instance of class 1 there, not three."""
    s = loop["s"]
    cls_ids, RTs = np.zeros((2, 4), np.int32), np.zeros((2, 4, 3, 4))
    for b in range(2):
        own = np.nonzero(s["frame_of"] == b)[0]
        cls_ids[b, :len(own)], RTs[b, :len(own)] = s["class_of"][own], s["poses"][own]
    old = train_data.pose_targets(loop["cld"], loop["choose"], loop["label"], cls_ids, RTs, s["mesh_kps"], s["mesh_ctr"])
    assert torch.equal(old["labels"], loop["tg"]["labels"])
    ctr_of, kp_of = train_data.votes_from_targets(old)
    got = pose.solve_instances(loop["cld"], old["labels"], ctr_of, kp_of, s["mesh_kps"], s["mesh_ctr"], max_instances=4)
    frm, cls, T = got["est_frame"].cpu().numpy(), got["est_class"].cpu().numpy(), got["est_RT"].cpu().numpy()
    sel = (frm == 0) & (cls == 1)
    assert sel.sum() < 3
    hit = {i for i, add in _match(s, zip(frm[sel], cls[sel], T[sel])) if add < 1e-3}
    assert hit == {2}                                                                  # the last class-1 slot of frame 0, and only it


# ---- the batch builder ------------------------------------------------------------------------------------------
def test_builder_with_instances_returns_the_instance_targets_and_the_ground_truth(loop):
    b, tg, s = loop["batch"], loop["tg"], loop["s"]
    for k in ("inst_labels", "n_points_inst", "gt_RT", "gt_class", "gt_frame", "labels", "rgb_labels", "kp_targ_ofst", "ctr_targ_ofst",
              "kp_3ds", "ctr_3ds", "choose", "cld_rgb_nrm"):
        assert b[k].is_cuda, k
    assert "inst_of_point" not in b and "n_points" not in b
    assert torch.equal(b["choose"], loop["choose"])                                    # the same sampling key: the same points
    for k, t in (("labels", "labels"), ("inst_labels", "inst_of_point"), ("n_points_inst", "n_points"), ("kp_targ_ofst", "kp_targ_ofst"),
                 ("ctr_targ_ofst", "ctr_targ_ofst"), ("kp_3ds", "kp_3ds"), ("ctr_3ds", "ctr_3ds")):
        assert torch.equal(b[k], tg[t]), k
    assert b["gt_RT"].dtype == torch.float64 and tuple(b["gt_RT"].shape) == (6, 3, 4)
    assert b["gt_class"].dtype == torch.int32 and b["gt_frame"].cpu().tolist() == s["frame_of"].tolist()
    assert torch.equal(b["rgb_labels"], loop["label"])
    # the points' instances are the instance image at the chosen pixels, and their classes the class image there
    choose = b["choose"].reshape(2, -1).long()
    assert torch.equal(b["inst_labels"], loop["inst"].reshape(2, -1).gather(1, choose))
    assert torch.equal(b["labels"], loop["label"].reshape(2, -1).gather(1, choose))


def test_builder_without_instances_is_what_it_was(loop):
    """assemble_inputs, then pose_targets, then rgb_labels: the same keys and the same bits as before `instances` existed."""
    s = loop["s"]
    cls_ids, RTs = np.array([[1, 2], [1, 0]], np.int32), np.stack([s["poses"][[2, 3]], s["poses"][[5, 5]]])
    got = train_data.assemble_training_batch(loop["rgb"], loop["depth"], loop["label"], s["K"], N_POINTS, cls_ids, RTs, s["mesh_kps"],
                                             s["mesh_ctr"], normals=loop["nrm"], seed=SEED)
    inp = inputs.assemble_inputs(loop["rgb"], loop["depth"], loop["nrm"], s["K"], N_POINTS, seed=SEED, min_points=0)
    tg = train_data.pose_targets(inp["cld_xyz0"], inp["choose"], loop["label"], cls_ids, RTs, s["mesh_kps"], s["mesh_ctr"])
    assert set(got) == set(inp) | set(tg) | {"rgb_labels"}
    assert set(tg) == {"labels", "kp_targ_ofst", "ctr_targ_ofst", "kp_3ds", "ctr_3ds", "RTs", "cls_ids"}
    for k, v in list(inp.items()) + list(tg.items()):
        assert torch.equal(got[k], v), k
    assert torch.equal(got["rgb_labels"], loop["label"])

