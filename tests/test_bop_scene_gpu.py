"""ffb6d_amd.bop's scene evaluation on the device against the numpy restatement (tests/bop_scene_ref.py): instance visibility
(every integer, the float64 fraction as bits, the mask), instance_info through the rasteriser, the greedy matching, and
BOPSceneEval against BOPEval on a batch where the two must agree exactly."""
import numpy as np
import pytest
import torch

import bop_ref
import bop_scene_ref as ref
import render_ref
from ffb6d_amd import bop, evaluate, render

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def host(t):
    return t.cpu().numpy()


# ---- visibility ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def image_cases():
    """per frame size: the 3-row case with a bad frame id in the middle row and its reference, computed once"""
    out = {}
    for size in bop_ref.VSD_IMAGE_SIZES:
        v = ref.visib_image_case(*size, Q=3, bad_row=1)
        v["want"] = ref.visib(v["depth_test"], v["depth_obj"], v["frame_of"], v["K"], v["delta"])
        for a in v["want"]:
            a.setflags(write=False)
        out[size] = v
    return out


@pytest.mark.parametrize("masks", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("size", bop_ref.VSD_IMAGE_SIZES, ids=lambda hw: "%dx%d" % hw)
def test_visibility_equals_the_restatement_as_bits(device, image_cases, size, masks):
    """97 x 131: single floats and bytes, 4 runs; 96 x 132: 16-byte accesses and 4-byte mask stores; 480 x 641: 76 runs with a tail,
    more than the 64 lanes that combine a row's records.  Q = 0, 1 and 3, the middle row of the three with a bad frame id."""
    v = image_cases[size]
    want_i, want_f, want_m = v["want"]
    assert (want_i[[0, 2], 0] > want_i[[0, 2], 2]).all() and (want_i[[0, 2], 2] > 0).all() and 0 < want_i[0, 3] < want_i[0, 1]
    assert np.isnan(want_f[1]) and not want_m[1].any() and len({tuple(r) for r in want_i}) == 3
    up = lambda k, n: torch.from_numpy(np.ascontiguousarray(v[k][:n])).to(device)    # noqa: E731
    test, Kd = torch.from_numpy(v["depth_test"]).to(device), torch.from_numpy(v["K"]).to(device)
    for Q in (0, 1, 3):
        info, fract, mask = bop.visib_compare(test, up("depth_obj", Q), up("frame_of", Q), Kd, delta=v["delta"], masks=masks)
        assert info.dtype == torch.int32 and fract.dtype == torch.float64 and tuple(info.shape) == (Q, 12) and (mask is None) == (not masks)
        assert np.array_equal(host(info), want_i[:Q]), (Q, host(info), want_i[:Q])
        assert np.array_equal(bits(host(fract)), bits(want_f[:Q])), (Q, host(fract), want_f[:Q])
        if masks:
            assert mask.dtype == torch.uint8 and np.array_equal(host(mask), want_m[:Q]), Q
    # in place, over outputs that hold something else
    out = (torch.full((3, 12), 7, dtype=torch.int32, device=device), torch.full((3,), 7.0, dtype=torch.float64, device=device),
           torch.full((3,) + size, 7, dtype=torch.uint8, device=device) if masks else None)
    got = bop.visib_compare(test, up("depth_obj", 3), up("frame_of", 3), Kd, delta=v["delta"], out=out)
    assert got[0] is out[0] and np.array_equal(host(out[0]), want_i) and np.array_equal(bits(host(out[1])), bits(want_f))
    if masks:
        assert np.array_equal(host(out[2]), want_m)


def test_instance_info_equals_the_reference_render_and_does_not_depend_on_the_chunking(device):
    v = bop_ref.vsd_case(48, 64)
    H, W = 48, 64
    meshes = render.PreparedMeshes(v["meshes"], device)
    with pytest.raises(ValueError, match="class_of"):                            # host class ids are checked (row 7 names class 9)
        bop.instance_info(v["depth_test"], v["gt_T"], v["class_of"], v["frame_of"], v["K"], meshes)
    depth = bop_ref.render_alone(v["meshes"], v["gt_T"], v["class_of"], v["frame_of"], v["K"], H, W)
    bad_cls = (v["class_of"] < 0) | (v["class_of"] >= len(v["meshes"]))
    want_i, want_f, want_m = ref.visib(v["depth_test"], depth, np.where(bad_cls, -1, v["frame_of"]), v["K"], v["delta"])
    assert bad_cls[7] and np.isnan(want_f[[7, 8]]).all() and (want_i[:4, 2] > 0).all() and want_i[4, 0] == 0 and want_f[4] == 0.0
    assert (want_i[:4, 0] > want_i[:4, 2]).any()
    cls_dev = torch.from_numpy(v["class_of"]).to(device)                         # device ids are not read back: a NaN row
    whole = bop.instance_info(v["depth_test"], v["gt_T"], cls_dev, v["frame_of"], v["K"], meshes, delta=v["delta"], masks=True)
    names = ("px_count_all", "px_count_valid", "px_count_visib", "px_count_support")
    for k, name in enumerate(names):
        assert np.array_equal(host(whole[name]), want_i[:, k]), name
    assert np.array_equal(host(whole["bbox_obj"]), want_i[:, 4:8]) and np.array_equal(host(whole["bbox_visib"]), want_i[:, 8:12])
    assert np.array_equal(bits(host(whole["visib_fract"])), bits(want_f)) and np.array_equal(host(whole["mask_visib"]), want_m)
    for chunk in (1, 4):
        part = bop.instance_info(v["depth_test"], v["gt_T"], cls_dev, v["frame_of"], v["K"], meshes, delta=v["delta"], masks=True, chunk_rows=chunk)
        assert set(part) == set(whole)
        for name in whole:
            assert np.array_equal(bits(host(part[name])), bits(host(whole[name]))), (chunk, name)
    assert "mask_visib" not in bop.instance_info(v["depth_test"], v["gt_T"][:2], v["class_of"][:2], v["frame_of"][:2], v["K"], meshes)


# ---- matching -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_col,n_thr", [(1, 1), (10, 11), (16, 16)], ids=["1", "110", "256"])
def test_matching_equals_the_restatement_and_its_two_tables_agree(device, n_col, n_thr):
    """Groups of 0, 1, 2, 7 and 64 estimates and instances mixed in one call; errors and scores with planted ties and NaNs."""
    c = ref.match_case(n_col, n_thr)
    tb = c["tables"]
    assert {int(n) for n in np.diff(tb["est_begin"])} == {0, 1, 2, 3, 7, 64} and {int(n) for n in np.diff(tb["gt_begin"])} == {0, 1, 2, 3, 7, 64}
    want_e, want_g = ref.match(tb, c["err"], c["score"], c["thr"], c["max_ests"])
    assert (want_e >= 0).any() and (want_e == -1).any() and np.isnan(c["err"]).any() and np.isnan(c["score"]).any()
    dev_in = [torch.from_numpy(c[k]).to(device) for k in ("err", "score")]
    est_gt, gt_est = bop.match(dev_in[0], dev_in[1], tb, c["thr"], c["max_ests"])     # thresholds and max_ests as host data: uploaded
    assert est_gt.dtype == torch.int32 and tuple(est_gt.shape) == want_e.shape and tuple(gt_est.shape) == want_g.shape
    e, g = host(est_gt), host(gt_est)
    assert np.array_equal(e, want_e) and np.array_equal(g, want_g)
    # the two tables say the same thing: instance t of a group was taken by estimate e exactly when e took t
    for grp in range(len(tb["est_begin"]) - 1):
        e0, t0 = tb["est_begin"][grp], tb["gt_begin"][grp]
        eg, gg = e[e0:tb["est_begin"][grp + 1]], g[t0:tb["gt_begin"][grp + 1]]
        for local, row in enumerate(eg):
            took = row >= 0
            cfg = np.argwhere(took)
            assert (gg[row[took], cfg[:, 0], cfg[:, 1]] == local).all()
        assert (gg >= 0).sum() == (eg >= 0).sum()
    # device tensors in, the same bytes out of a second call; without max_ests
    e2, g2 = bop.match(dev_in[0], dev_in[1], tb, torch.from_numpy(c["thr"]).to(device), torch.from_numpy(c["max_ests"]).to(device))
    assert torch.equal(e2, est_gt) and torch.equal(g2, gt_est)
    want_e, want_g = ref.match(tb, c["err"], c["score"], c["thr"], None)
    e3, g3 = bop.match(dev_in[0], dev_in[1], tb, c["thr"])
    assert np.array_equal(host(e3), want_e) and np.array_equal(host(g3), want_g)


def test_match_refuses_tables_the_host_check_refuses(device):
    from ffb6d_amd import _lib
    c = ref.match_case(1, 1, ((2, 2), (1, 1)))
    bad = dict(c["tables"], pair_begin=np.array([0, 3, 5], np.int64))
    with pytest.raises(_lib.FFB6DNativeError, match="pair_begin"):
        bop.match(c["err"], c["score"], bad, c["thr"])
    with pytest.raises(_lib.FFB6DNativeError, match="at most 64"):
        bop.match(np.zeros((65, 1)), np.zeros(65, np.float32), ref.group_tables(((65, 1),)), np.ones((1, 1)))
    empty = bop.match(np.zeros((0, 1)), np.zeros(0, np.float32), ref.group_tables(()), np.zeros((0, 1)))
    assert tuple(empty[0].shape) == (0, 1, 1) and tuple(empty[1].shape) == (0, 1, 1)


# ---- BOPSceneEval -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(device):
    v = bop_ref.vsd_case(48, 64)
    models = [np.zeros((0, 3), np.float32) if m is None else m["xyz"] for m in v["meshes"]]
    flip = np.diag([1.0, 1.0, -1.0, 1.0])
    syms = [None, bop.symmetry_transforms(continuous=[((0, 0, 1), (0, 0, 0))], max_disc_step=0.4), None, None, None,
            bop.symmetry_transforms(discrete=[flip])]
    v["args"] = (evaluate.ModelPoints(models, device), render.PreparedMeshes(v["meshes"], device), bop.SymmetrySets(syms, device), v["diameters"])
    return v


def test_scene_eval_equals_bop_eval_on_a_one_to_one_all_visible_batch(scene):
    v = scene
    rows = np.arange(4)                                                          # (frame, class) = (0,1), (0,5), (1,1), (1,5): one instance per group
    assert len({(int(f), int(c)) for f, c in zip(v["frame_of"][rows], v["class_of"][rows])}) == 4
    depth = bop_ref.render_alone(v["meshes"], v["gt_T"][rows], v["class_of"][rows], v["frame_of"][rows], v["K"], 48, 64)
    _, fract, _ = ref.visib(v["depth_test"], depth, v["frame_of"][rows], v["K"], v["delta"])
    assert (fract >= 0.1).all(), fract                                           # every instance is a target
    est, gt, cls, frm = v["est_T"][rows], v["gt_T"][rows], v["class_of"][rows], v["frame_of"][rows]
    plain = bop.BOPEval(*v["args"], delta=v["delta"])
    plain.add_batch(v["depth_test"], est, gt, cls, frm, v["K"])
    want = plain.cal_ar()
    ev = bop.BOPSceneEval(*v["args"], delta=v["delta"])
    order = np.array([2, 0, 3, 1])                                               # the estimates in another order than the instances
    ev.add_batch(v["depth_test"][:1], v["K"][:1], est[[1, 0]], cls[[1, 0]], frm[[1, 0]], [0.3, 0.9], gt[:2], cls[:2], frm[:2])      # two batches
    ev.add_batch(v["depth_test"], v["K"], est[order][[0, 2]], cls[order][[0, 2]], frm[order][[0, 2]], None, gt[2:], cls[2:], frm[2:])
    got = ev.cal_ar()
    assert 0 < want["ar"] < 1 and want["n"] == 4
    for key in want:
        assert got[key] == want[key], (key, got[key], want[key])
    assert got["n_targets"] == 4 and got["n_ignored"] == 0
    assert ev.cal_ar() == got                                                    # asking twice gives the same answer


def test_an_occluded_instance_is_ignored_and_a_duplicate_estimate_is_unmatched(scene, device):
    v = scene
    H, W = 48, 64
    P = render_ref.pose
    # frame 0: instance A (class 1) and B (class 5) of the shared case, and C (class 1) behind an occluder that covers all of it
    gt = np.stack([v["gt_T"][0], v["gt_T"][1], P([-0.2, -0.12, 0.6])])
    gcls, gfrm = np.array([1, 5, 1], np.int32), np.zeros(3, np.int32)
    depth = bop_ref.render_alone(v["meshes"], gt, gcls, gfrm, v["K"], H, W)
    x, y, w, h = ref.visib_row(np.zeros((H, W), np.float32), depth[2], v["K"][0], v["delta"])[0][4:8]
    assert w > 2 and h > 2
    test = np.zeros((1, H, W), np.float32)                                       # no measurement: visible
    test[0, y:y + h, x:x + w] = 0.2                                              # in front of C
    _, fract, _ = ref.visib(test, depth, gfrm, v["K"], v["delta"])
    assert fract[0] >= 0.1 and fract[1] >= 0.1 and fract[2] == 0.0, fract
    # estimates: A's, a duplicate of it with a lower score, B's
    est = np.stack([v["est_T"][0], v["est_T"][0], v["est_T"][1]])
    ecls, efrm, score = np.array([1, 1, 5], np.int32), np.zeros(3, np.int32), np.array([0.9, 0.4, 0.7], np.float32)
    ev = bop.BOPSceneEval(*v["args"], delta=v["delta"])
    m = ev.add_batch(test, v["K"][:1], est, ecls, efrm, score, gt, gcls, gfrm)
    assert np.array_equal(bits(host(m["visib_fract"])), bits(fract))
    g = m["groups"]
    assert g["est_order"].tolist() == [0, 1, 2] and g["gt_order"].tolist() == [0, 2, 1] and host(m["valid"]).tolist() == [True, False, True]
    for k in ("vsd", "mssd", "mspd"):
        e, t = host(m["est_gt"][k]), host(m["gt_est"][k])
        assert (e[1] == -1).all(), k                                            # the duplicate: one valid target, so only the best estimate is considered
        assert (e[0] == 0).any() and ((e[0] == 0) | (e[0] == -1)).all(), k       # the better-scored copy takes A where its error is below the threshold
        assert (t[1] == -1).all() and np.array_equal(t[0] == 0, e[0] == 0), k    # nobody takes C
    got = ev.cal_ar()
    assert got["n_targets"] == 2 and got["n_ignored"] == 1 and got["n"] == 2 and got["n_lst"][1] == 1 and got["n_lst"][5] == 1
    for k in ("vsd", "mssd", "mspd"):
        assert 0 < got["ar_" + k] <= 1 and got["precision_" + k] == got["ar_" + k], k          # 2 targets, 2 considered estimates
