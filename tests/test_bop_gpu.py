"""ffb6d_amd.bop on the device against the numpy restatement (tests/bop_ref.py): the squared MSSD / MSPD, the VSD counts and vsd
equal it bit for bit; mssd / mspd after the wrapper's sqrt are within 1 ulp of np.sqrt of the reference squares (any faithful
square root is); a row's result does not depend on Q or on the other rows; the chunked vsd equals the unchunked one."""
import numpy as np
import pytest
import torch

import bop_ref
from ffb6d_amd import bop, evaluate, render

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def case(device):
    c = bop_ref.mssd_case()
    c["model_points"] = evaluate.ModelPoints(c["models"], device)
    c["sets"] = bop.SymmetrySets(c["syms"], device)
    c["no_sets"] = bop.SymmetrySets([None] * 5, device)
    for name in ("rows", "bad"):
        r = c[name]
        r["want"] = bop_ref.mssd_mspd2(c["models"], c["syms"], r["class_of"], r["frame_of"], r["est_T"], r["gt_T"], c["K"])
        for v in r["want"]:
            v.setflags(write=False)
    return c


def squares(c, rows, sets=None, **kw):
    s2, p2 = bop.mssd2_mspd2(rows["est_T"], rows["gt_T"], rows["class_of"], rows["frame_of"], c["K"], c["model_points"],
                             c["sets"] if sets is None else sets, **kw)
    return (None if s2 is None else host(s2)), (None if p2 is None else host(p2))


@pytest.mark.parametrize("which", ["rows", "bad"])
def test_squared_mssd_and_mspd_equal_the_restatement_as_bits(case, which):
    rows = case[which]
    assert [len(s) for s in case["sets"].sets] == [1, 1, 315, 2, 9] and case["sets"].max_syms == 315
    s2, p2 = squares(case, rows)
    want_s, want_p = rows["want"]
    assert np.array_equal(bits(s2), bits(want_s)), (s2, want_s)
    assert np.array_equal(bits(p2), bits(want_p)), (p2, want_p)
    if which == "bad":
        assert np.isnan(want_s[[0, 1, 2, 3, 4, 5, 6, 9]]).all() and np.isfinite(want_s[[7, 8]]).all()
        assert want_p[7] == np.inf and np.isfinite(want_p[8])
    only_s, none = squares(case, rows, outputs=("mssd",))
    assert none is None and np.array_equal(bits(only_s), bits(want_s))
    none, only_p = squares(case, rows, outputs=("mspd",))
    assert none is None and np.array_equal(bits(only_p), bits(want_p))


@pytest.mark.parametrize("which", ["rows", "bad"])
def test_mssd_and_mspd_are_within_one_ulp_of_the_square_root_of_the_reference_squares(case, which):
    rows = case[which]
    mssd, mspd = bop.mssd_mspd(rows["est_T"], rows["gt_T"], rows["class_of"], rows["frame_of"], case["K"], case["model_points"], case["sets"])
    assert mssd.dtype == torch.float64 and mspd.dtype == torch.float64 and mssd.is_cuda
    for got, want2 in ((host(mssd), rows["want"][0]), (host(mspd), rows["want"][1])):
        want = np.sqrt(want2)
        fin = np.isfinite(want)
        print(which, "max |got - sqrt(ref)| / spacing:", (np.abs(got[fin] - want[fin]) / np.spacing(want[fin])).max() if fin.any() else None)
        assert (np.abs(got[fin] - want[fin]) <= np.spacing(want[fin])).all()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == np.inf, want == np.inf)


def test_a_row_scores_the_same_alone_and_inside_a_batch(case):
    rows = case["rows"]
    want_s, want_p = rows["want"]
    for q in range(len(rows["class_of"])):
        one = {k: rows[k][q:q + 1] for k in ("class_of", "frame_of", "est_T", "gt_T")}
        s2, p2 = squares(case, one)
        assert bits(s2)[0] == bits(want_s)[q] and bits(p2)[0] == bits(want_p)[q], q
    # reversed, and between bad rows
    bad = case["bad"]
    mix = {k: np.concatenate([bad[k][:5], rows[k][::-1], bad[k][5:]]) for k in ("class_of", "frame_of", "est_T", "gt_T")}
    s2, p2 = squares(case, mix)
    assert np.array_equal(bits(s2[5:12]), bits(want_s[::-1])) and np.array_equal(bits(p2[5:12]), bits(want_p[::-1]))


def test_without_symmetry_sets_every_class_is_scored_with_the_identity(case):
    rows = case["rows"]
    want = bop_ref.mssd_mspd2(case["models"], [[bop_ref.IDENTITY]] * 5, rows["class_of"], rows["frame_of"], rows["est_T"], rows["gt_T"], case["K"])
    s2, p2 = squares(case, rows, sets=case["no_sets"])
    assert np.array_equal(bits(s2), bits(want[0])) and np.array_equal(bits(p2), bits(want[1]))
    assert (want[0][[1, 4, 5]] > 10 * rows["want"][0][[1, 4, 5]]).all()         # the rows near a symmetric copy: the set matters


def test_classes_of_several_point_chunks_with_the_farthest_point_in_the_last_one(device):
    """More than the 1024 points of one workgroup, no multiple of it (2500, 1025) and exactly 1024."""
    c = bop_ref.chunk_case()
    rows = c["rows"]
    want = bop_ref.mssd_mspd2(c["models"], c["syms"], rows["class_of"], rows["frame_of"], rows["est_T"], rows["gt_T"], c["K"])
    inner = bop_ref.mssd_mspd2(c["inner"], c["syms"], rows["class_of"], rows["frame_of"], rows["est_T"], rows["gt_T"], c["K"])
    assert (want[0] > 4 * inner[0]).all() and (want[1] > inner[1]).all()          # the last point of the last chunk decides
    models, sets = evaluate.ModelPoints(c["models"], device), bop.SymmetrySets(c["syms"], device)
    assert models.max_points == 2500
    s2, p2 = bop.mssd2_mspd2(rows["est_T"], rows["gt_T"], rows["class_of"], rows["frame_of"], c["K"], models, sets)
    assert np.array_equal(bits(host(s2)), bits(want[0])), (s2, want[0])
    assert np.array_equal(bits(host(p2)), bits(want[1])), (p2, want[1])


def test_a_batch_larger_than_one_library_call_is_split(device, monkeypatch):
    c = bop_ref.mssd_case()
    rows = c["rows"]
    want = bop_ref.mssd_mspd2(c["models"], c["syms"], rows["class_of"], rows["frame_of"], rows["est_T"], rows["gt_T"], c["K"])
    monkeypatch.setattr(bop, "MAX_ROWS", 3)                                      # 7 rows: calls of 3, 3 and 1
    s2, p2 = bop.mssd2_mspd2(rows["est_T"], rows["gt_T"], rows["class_of"], rows["frame_of"], c["K"], evaluate.ModelPoints(c["models"], device),
                             bop.SymmetrySets(c["syms"], device))
    assert np.array_equal(bits(host(s2)), bits(want[0])) and np.array_equal(bits(host(p2)), bits(want[1]))


# ---- VSD ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(37, 53), (48, 64)], ids=["37x53", "48x64"])
def vsd_case(request, device):
    H, W = request.param
    v = bop_ref.vsd_case(H, W)
    v["prepared"] = render.PreparedMeshes(v["meshes"], device)
    for name in ("est", "gt"):
        v["depth_" + name] = bop_ref.render_alone(v["meshes"], v[name + "_T"], v["class_of"], v["frame_of"], v["K"], H, W)
    return v


def device_vsd(v, taus, **kw):
    err, counts = bop.vsd(v["depth_test"], v["est_T"], v["gt_T"], v["class_of"], v["frame_of"], v["K"], v["prepared"], v["diameters"],
                          delta=v["delta"], taus=taus, **kw)
    return host(err), host(counts)


@pytest.mark.parametrize("n_tau", [1, 10, 16])
def test_vsd_and_its_counts_equal_the_restatement_as_bits(vsd_case, n_tau):
    v, taus = vsd_case, bop_ref.TAU_SETS[n_tau]
    want_c, want_v = bop_ref.vsd(v["depth_test"], v["depth_est"], v["depth_gt"], v["class_of"], v["frame_of"], v["K"], v["diameters"],
                                 v["delta"], taus)
    assert want_c[3, 0] > 0 and want_c[3, 1] == 0 and (want_v[3] == 1.0).all()                  # the estimate misses: union from gt alone
    assert want_c[4, 0] == 0 and (want_v[4] == 1.0).all()                                       # both renders empty
    assert (want_c[:3, 1] > 0).all() and np.isnan(want_v[7:]).all()
    err, counts = device_vsd(v, taus)
    assert err.dtype == np.float64 and counts.dtype == np.int32
    assert np.array_equal(counts, want_c), (counts, want_c)
    assert np.array_equal(bits(err), bits(want_v)), (err, want_v)


def test_the_chunked_vsd_equals_the_unchunked_one(vsd_case):
    v = vsd_case
    err, counts = device_vsd(v, bop_ref.TAUS10)
    for chunk in (1, 4):
        e, c = device_vsd(v, bop_ref.TAUS10, chunk_rows=chunk)
        assert np.array_equal(c, counts) and np.array_equal(bits(e), bits(err)), chunk
    assert bop.rows_per_chunk(480, 640) == 54 and bop.rows_per_chunk(48, 64) == 512 and bop.rows_per_chunk(8192, 8192) == 1


@pytest.mark.parametrize("size", bop_ref.VSD_IMAGE_SIZES, ids=lambda hw: "%dx%d" % hw)
def test_frames_of_several_pixel_runs_equal_the_restatement_as_bits(device, size):
    """The comparison alone on synthetic depth images: more than the 4096 pixels of one workgroup, no multiple of it, odd and a
    multiple of 4; 480 x 641 has more runs (76) than the 64 lanes that add a row's partial counts."""
    v = bop_ref.vsd_image_case(*size, Q=2 if size[0] * size[1] > 100000 else 3)
    want_c, want_v = bop_ref.vsd(v["depth_test"], v["depth_est"], v["depth_gt"], v["class_of"], v["frame_of"], v["K"], v["diameters"],
                                 v["delta"], bop_ref.TAUS10)
    assert (want_c[:, 1] > 0).all() and (want_c[:, 0] > want_c[:, 1]).all() and (want_c[:, 2] > want_c[:, -1]).all()
    up = lambda k: torch.from_numpy(v[k]).to(device)                             # noqa: E731
    taus = torch.from_numpy(bop_ref.TAUS10.astype(np.float32)).to(device)        # a device tensor is used as it is
    err, counts = bop.vsd_compare(up("depth_test"), up("depth_est"), up("depth_gt"), up("class_of"), up("frame_of"), up("K"), up("diameters"),
                                  delta=v["delta"], taus=taus)
    assert np.array_equal(host(counts), want_c), (host(counts), want_c)
    assert np.array_equal(bits(host(err)), bits(want_v)), (host(err), want_v)
    err2, counts2 = bop.vsd_compare(up("depth_test"), up("depth_est"), up("depth_gt"), up("class_of"), up("frame_of"), up("K"), up("diameters"),
                                    delta=v["delta"], taus=bop_ref.TAUS10)
    assert torch.equal(counts2, counts) and torch.equal(err2, err)


def test_no_taus_and_too_many_are_refused(vsd_case):
    v = vsd_case
    for taus in ([], np.linspace(0.01, 0.5, 17)):
        with pytest.raises(ValueError, match="taus"):
            device_vsd(v, taus)


def test_bop_eval_accumulates_the_average_recall_of_the_reference_errors(device):
    v = bop_ref.vsd_case(48, 64)
    good = np.arange(7)                                                          # BOPEval validates host class ids
    sub = {k: v[k][good] for k in ("class_of", "frame_of", "est_T", "gt_T")}
    models = [np.zeros((0, 3), np.float32) if m is None else m["xyz"] for m in v["meshes"]]
    flip = np.diag([1.0, 1.0, -1.0, 1.0])
    syms = [None, bop.symmetry_transforms(continuous=[((0, 0, 1), (0, 0, 0))], max_disc_step=0.4), None, None, None,
            bop.symmetry_transforms(discrete=[flip])]
    ev = bop.BOPEval(evaluate.ModelPoints(models, device), render.PreparedMeshes(v["meshes"], device), bop.SymmetrySets(syms, device),
                     v["diameters"], delta=v["delta"])
    found = np.array([True, True, False, True, True, True, True])
    ev.add_batch(v["depth_test"], sub["est_T"][:4], sub["gt_T"][:4], sub["class_of"][:4], sub["frame_of"][:4], v["K"], found=found[:4])
    ev.add_batch(v["depth_test"], sub["est_T"][4:], sub["gt_T"][4:], sub["class_of"][4:], sub["frame_of"][4:], v["K"])
    got = ev.cal_ar()
    sets = [s if s is not None else [bop_ref.IDENTITY] for s in syms]
    s2, p2 = bop_ref.mssd_mspd2(models, sets, sub["class_of"], sub["frame_of"], sub["est_T"], sub["gt_T"], v["K"])
    d_est = bop_ref.render_alone(v["meshes"], sub["est_T"], sub["class_of"], sub["frame_of"], v["K"], 48, 64)
    d_gt = bop_ref.render_alone(v["meshes"], sub["gt_T"], sub["class_of"], sub["frame_of"], v["K"], 48, 64)
    _, err = bop_ref.vsd(v["depth_test"], d_est, d_gt, sub["class_of"], sub["frame_of"], v["K"], v["diameters"], v["delta"], bop.VSD_TAUS)
    mssd, mspd = np.sqrt(s2), np.sqrt(p2)
    mssd[~found], mspd[~found], err[~found] = np.inf, np.inf, np.inf
    want = bop.average_recall(err, mssd, mspd, v["diameters"].astype(np.float64)[sub["class_of"]], 64)
    assert got["n"] == 7 and got["n_lst"][1] == 3 and got["n_lst"][5] == 2 and got["n_lst"][2] == 0
    for k in ("ar", "ar_vsd", "ar_mssd", "ar_mspd"):
        assert got[k] == want[k], (k, got[k], want[k])
        assert got[k + "_lst"][0] == got[k] and len(got[k + "_lst"]) == 6
    assert 0 < got["ar"] < 1
    assert ev.cal_ar() == got                                                    # asking twice gives the same answer
