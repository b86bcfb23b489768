"""csrc/bop_eval.hip on the SIMT emulator (tests/simt), without a GPU: the unmodified kernel source, with errors.hip and render.hip,
compiled for the host and run through the C ABI of include/ffb6d_bop.h.  mssd2, mspd2, the counts and vsd equal the numpy
restatement (tests/bop_ref.py) bit for bit; argument errors return their code and write nothing; guard values around the outputs
stay intact."""
import numpy as np
import pytest

import bop_ref
import render_ref
from tests.simt.build import load, ptr as _p

GUARD = 8                       # guard entries on either side of an output


@pytest.fixture(scope="module")
def emu_bop():
    """the emulated library (tests/simt/build.py)"""
    return load()


@pytest.fixture(scope="module")
def case():
    c = bop_ref.mssd_case()
    c["tables"] = bop_ref.pack_tables(c["models"], c["syms"])
    for name in ("rows", "bad"):
        r = c[name]
        r["want"] = bop_ref.mssd_mspd2(c["models"], c["syms"], r["class_of"], r["frame_of"], r["est_T"], r["gt_T"], c["K"])
        for v in r["want"]:
            v.setflags(write=False)
    return c


def guarded(shape, dtype, fill):
    """(whole array, view of the output inside it)"""
    n = int(np.prod(shape))
    whole = np.full(n + 2 * GUARD, fill, dtype)
    return whole, whole[GUARD:GUARD + n].reshape(shape)


def guards_intact(whole, fill):
    return (whole[:GUARD] == fill).all() and (whole[-GUARD:] == fill).all()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32 if a.dtype == np.float32 else a.dtype)


def call_mssd(lib, tb, rows, cam, out_s, out_p, ws=None, **kw):
    """ffb6d_bop_mssd_mspd_f64 with numpy arrays as "device" memory; kw overrides arguments by name"""
    a = dict(model_pts=_p(tb["pts"]), model_begin=_p(tb["begin"]), n_cls=tb["n_cls"], total=tb["total"], max_points=tb["max_points"],
             sym_R=_p(tb["sym_R"]), sym_t=_p(tb["sym_t"]), sym_begin=_p(tb["sym_begin"]), Stot=tb["Stot"], max_syms=tb["max_syms"],
             class_of=_p(rows["class_of"]), frame_of=_p(rows["frame_of"]), est_T=_p(rows["est_T"]), gt_T=_p(rows["gt_T"]),
             Q=len(rows["class_of"]), K=_p(cam), B=len(cam), mssd2=_p(out_s), mspd2=_p(out_p))
    a.update(kw)
    if ws is None:
        ws = np.full(max(lib.ffb6d_bop_mssd_mspd_workspace_bytes(a["Q"], a["max_points"], a["max_syms"]), 8) // 8, np.nan)   # dirty
    a.setdefault("workspace", _p(ws))
    a.setdefault("workspace_bytes", ws.nbytes)
    return lib.ffb6d_bop_mssd_mspd_f64(*a.values(), None)


def sub_rows(rows, idx):
    return {k: np.ascontiguousarray(rows[k][idx]) for k in ("class_of", "frame_of", "est_T", "gt_T")}


@pytest.mark.parametrize("which", ["rows", "bad"])
def test_mssd2_and_mspd2_on_the_emulator_equal_the_restatement_as_bits(emu_bop, case, which):
    lib, rows = emu_bop, case[which]
    Q = len(rows["class_of"])
    ws_, s2 = guarded((Q,), np.float64, 7.0)
    wp_, p2 = guarded((Q,), np.float64, 7.0)
    assert call_mssd(lib, case["tables"], rows, case["K"], s2, p2) == 0, lib.ffb6d_last_error()
    want_s, want_p = rows["want"]
    assert np.array_equal(bits(s2), bits(want_s)), (s2, want_s)
    assert np.array_equal(bits(p2), bits(want_p)), (p2, want_p)
    assert guards_intact(ws_, 7.0) and guards_intact(wp_, 7.0)
    if which == "rows":
        assert np.isfinite(want_s).all() and (want_s > 0).all() and np.isfinite(want_p).all()
    # either output alone
    _, only = guarded((Q,), np.float64, 7.0)
    assert call_mssd(lib, case["tables"], rows, case["K"], only, None) == 0
    assert np.array_equal(bits(only), bits(want_s))
    assert call_mssd(lib, case["tables"], rows, case["K"], None, only) == 0
    assert np.array_equal(bits(only), bits(want_p))


def test_a_row_alone_equals_the_row_in_its_batch_and_empty_tables_mean_the_identity(emu_bop, case):
    lib, rows = emu_bop, case["rows"]
    for q in (0, 1, 3):
        one = sub_rows(rows, [q])
        s2, p2 = np.zeros(1), np.zeros(1)
        assert call_mssd(lib, case["tables"], one, case["K"], s2, p2) == 0
        assert bits(s2)[0] == bits(rows["want"][0])[q] and bits(p2)[0] == bits(rows["want"][1])[q]
    # no symmetry entries at all (Stot = 0, null tables) = the identity alone for every class; tables that run past the arrays are cut
    none = [[] for _ in case["syms"]]
    tb = bop_ref.pack_tables(case["models"], none)
    want = bop_ref.mssd_mspd2(case["models"], none, rows["class_of"], rows["frame_of"], rows["est_T"], rows["gt_T"], case["K"])
    explicit = bop_ref.mssd_mspd2(case["models"], [[bop_ref.IDENTITY]] * 5, rows["class_of"], rows["frame_of"], rows["est_T"], rows["gt_T"],
                                  case["K"])
    assert np.array_equal(bits(want[0]), bits(explicit[0])) and np.array_equal(bits(want[1]), bits(explicit[1]))
    Q = len(rows["class_of"])
    s2, p2 = np.zeros(Q), np.zeros(Q)
    assert call_mssd(lib, tb, rows, case["K"], s2, p2, sym_R=None, sym_t=None) == 0, lib.ffb6d_last_error()
    assert np.array_equal(bits(s2), bits(want[0])) and np.array_equal(bits(p2), bits(want[1]))
    wild = dict(case["tables"], begin=case["tables"]["begin"].copy(), sym_begin=case["tables"]["sym_begin"].copy())
    wild["begin"][-1] += 10 ** 12
    wild["sym_begin"][-1] += 10 ** 12
    assert call_mssd(lib, wild, rows, case["K"], s2, p2) == 0
    assert np.array_equal(bits(s2), bits(rows["want"][0])) and np.array_equal(bits(p2), bits(rows["want"][1]))


def test_classes_of_several_point_chunks_with_the_farthest_point_in_the_last_one(emu_bop):
    """More than the 1024 points of one workgroup, no multiple of it: the chunk index into the workspace, the max over the chunks
    of the second launch and a tail in a workgroup that is not the first."""
    lib, c = emu_bop, bop_ref.chunk_case()
    rows = c["rows"]
    want = bop_ref.mssd_mspd2(c["models"], c["syms"], rows["class_of"], rows["frame_of"], rows["est_T"], rows["gt_T"], c["K"])
    inner = bop_ref.mssd_mspd2(c["inner"], c["syms"], rows["class_of"], rows["frame_of"], rows["est_T"], rows["gt_T"], c["K"])
    assert (want[0] > 4 * inner[0]).all() and (want[1] > inner[1]).all()          # the last point of the last chunk decides
    tb = bop_ref.pack_tables(c["models"], c["syms"])
    assert tb["max_points"] == 2500
    Q = len(rows["class_of"])
    ws_, s2 = guarded((Q,), np.float64, 7.0)
    wp_, p2 = guarded((Q,), np.float64, 7.0)
    assert call_mssd(lib, tb, rows, c["K"], s2, p2) == 0, lib.ffb6d_last_error()
    assert np.array_equal(bits(s2), bits(want[0])), (s2, want[0])
    assert np.array_equal(bits(p2), bits(want[1])), (p2, want[1])
    assert guards_intact(ws_, 7.0) and guards_intact(wp_, 7.0)
    # max_points cuts every class: the same as the classes without the points beyond it
    cut = [m[:1500] for m in c["models"]]
    want_cut = bop_ref.mssd_mspd2(cut, c["syms"], rows["class_of"], rows["frame_of"], rows["est_T"], rows["gt_T"], c["K"])
    assert call_mssd(lib, tb, rows, c["K"], s2, p2, max_points=1500) == 0, lib.ffb6d_last_error()
    assert np.array_equal(bits(s2), bits(want_cut[0])) and np.array_equal(bits(p2), bits(want_cut[1]))


def test_mssd_argument_errors_return_their_code_and_write_nothing(emu_bop, case):
    lib, rows, tb = emu_bop, case["rows"], case["tables"]
    Q = len(rows["class_of"])
    small = np.zeros(8)
    cases = [(dict(Q=-1), -1, "bad sizes"), (dict(Q=65536), -1, "bad sizes"), (dict(n_cls=0), -1, "bad sizes"), (dict(B=0), -1, "bad sizes"),
             (dict(max_points=tb["total"] + 1), -1, "bad tables"), (dict(max_syms=tb["Stot"] + 1), -1, "bad tables"),
             (dict(max_points=-1), -1, "bad tables"), (dict(mssd2=None, mspd2=None), -1, "no output"), (dict(est_T=None), -1, "null pointer"),
             (dict(sym_R=None), -1, "null pointer"), (dict(K=None), -1, "null pointer"), (dict(workspace=None), -3, "workspace"),
             (dict(workspace=_p(small), workspace_bytes=64), -3, "workspace")]
    for kw, code, text in cases:
        s2, p2 = np.full(Q, 7.0), np.full(Q, 7.0)
        assert call_mssd(lib, tb, rows, case["K"], s2, p2, **kw) == code, kw
        assert text in lib.ffb6d_last_error().decode(), (kw, lib.ffb6d_last_error())
        assert (s2 == 7).all() and (p2 == 7).all(), kw
    assert not small.any()
    assert lib.ffb6d_bop_mssd_mspd_workspace_bytes(0, 10, 1) == 0 and lib.ffb6d_bop_mssd_mspd_workspace_bytes(3, 0, 1) == 0
    assert lib.ffb6d_bop_mssd_mspd_workspace_bytes(3, 1025, 9) == 3 * 16 * 2 * 16


# ---- VSD ----------------------------------------------------------------------------------------------------------------------
def emu_render_alone(lib, pk, v, T):
    """Row q's model alone in frame q, through the emulated rasteriser"""
    Q, H, W = len(v["class_of"]), v["H"], v["W"]
    Kq = np.ascontiguousarray(np.stack([v["K"][min(max(int(b), 0), v["B"] - 1)] for b in v["frame_of"]]))
    frames = np.arange(Q, dtype=np.int32)
    depth = np.full((Q, H, W), 7, np.float32)
    ws = np.zeros(max(lib.ffb6d_render_workspace_bytes(Q, pk["max_verts"], Q, H, W), 1), np.uint8)
    T = np.ascontiguousarray(T)
    rc = lib.ffb6d_render_f32(_p(pk["verts"]), _p(pk["colors"]), _p(pk["faces"]), _p(pk["vert_begin"]), _p(pk["face_begin"]), pk["n_cls"],
                              pk["Vtot"], pk["Ftot"], pk["max_verts"], pk["max_faces"], _p(frames), _p(v["class_of"]), _p(T), Q, _p(Kq), Q, H, W,
                              1e-3, None, _p(depth), None, None, None, None, _p(ws), ws.nbytes, None)
    assert rc == 0, lib.ffb6d_last_error()
    return depth


@pytest.fixture(scope="module", params=[(37, 53), (48, 64)], ids=["37x53", "48x64"])
def vsd_case(request, emu_bop):
    H, W = request.param
    v = bop_ref.vsd_case(H, W)
    pk = render_ref.pack(v["meshes"])
    for name in ("est", "gt"):
        v["depth_" + name] = emu_render_alone(emu_bop, pk, v, v[name + "_T"])
        want = bop_ref.render_alone(v["meshes"], v[name + "_T"], v["class_of"], v["frame_of"], v["K"], H, W)
        assert np.array_equal(bits(v["depth_" + name]), bits(want)), name
        v["depth_" + name].setflags(write=False)
    return v


def call_vsd(lib, v, taus, out_counts, out_vsd, ws=None, **kw):
    taus = np.ascontiguousarray(taus, np.float32)
    a = dict(depth_test=_p(v["depth_test"]), depth_est=_p(v["depth_est"]), depth_gt=_p(v["depth_gt"]), class_of=_p(v["class_of"]),
             frame_of=_p(v["frame_of"]), Q=len(v["class_of"]), K=_p(v["K"]), B=v["B"], H=v["H"], W=v["W"], diameter=_p(v["diameters"]),
             n_cls=len(v["diameters"]), delta=v["delta"], taus=_p(taus), n_tau=len(taus), counts=_p(out_counts), vsd=_p(out_vsd))
    a.update(kw)
    if ws is None:
        ws = np.full(max(lib.ffb6d_bop_vsd_workspace_bytes(a["Q"], a["H"], a["W"]), 4) // 4, -12345, np.int32)             # dirty
    a.setdefault("workspace", _p(ws))
    a.setdefault("workspace_bytes", ws.nbytes)
    return lib.ffb6d_bop_vsd_f32(*a.values(), None)


@pytest.mark.parametrize("n_tau", [1, 10, 16])
def test_counts_and_vsd_on_the_emulator_equal_the_restatement_as_bits(emu_bop, vsd_case, n_tau):
    lib, v = emu_bop, vsd_case
    taus = bop_ref.TAU_SETS[n_tau]
    Q = len(v["class_of"])
    want_c, want_v = bop_ref.vsd(v["depth_test"], v["depth_est"], v["depth_gt"], v["class_of"], v["frame_of"], v["K"], v["diameters"],
                                 v["delta"], taus)
    # the case holds what it is meant to test
    assert (want_c[:3, 1] > 0).all() and (want_c[:3, 0] > want_c[:3, 1]).all()                  # inter and union-only pixels
    assert want_c[3, 0] > 0 and want_c[3, 1] == 0 and (want_v[3] == 1.0).all()                  # the estimate misses: union from gt alone
    assert want_c[4, 0] == 0 and (want_v[4] == 1.0).all()                                       # both renders empty
    assert np.isnan(want_v[7:]).all() and not want_c[7:].any()                                  # bad class / frame id
    if n_tau > 1:
        assert (np.diff(want_c[:3, 2:], axis=1) <= 0).all() and (want_c[:3, 2] > want_c[:3, -1]).any()
    wc_, counts = guarded((Q, 2 + n_tau), np.int32, 7)
    wv_, vsd = guarded((Q, n_tau), np.float64, 7.0)
    assert call_vsd(lib, v, taus, counts, vsd) == 0, lib.ffb6d_last_error()
    assert np.array_equal(counts, want_c), (counts, want_c)
    assert np.array_equal(bits(vsd), bits(want_v)), (vsd, want_v)
    assert guards_intact(wc_, 7) and guards_intact(wv_, 7.0)


@pytest.mark.parametrize("size", bop_ref.VSD_IMAGE_SIZES, ids=lambda hw: "%dx%d" % hw)
def test_frames_of_several_pixel_runs_equal_the_restatement_as_bits(emu_bop, size):
    """More than the 4096 pixels of one workgroup, no multiple of it, odd and a multiple of 4; 480 x 641 has more runs (76) than the
    64 lanes that add a row's partial counts."""
    lib = emu_bop
    v = bop_ref.vsd_image_case(*size, Q=2 if size[0] * size[1] > 100000 else 3)
    assert size[0] * size[1] > 4096 and (size[0] * size[1]) % 4096 != 0
    taus = bop_ref.TAUS10
    Q = len(v["class_of"])
    want_c, want_v = bop_ref.vsd(v["depth_test"], v["depth_est"], v["depth_gt"], v["class_of"], v["frame_of"], v["K"], v["diameters"],
                                 v["delta"], taus)
    assert (want_c[:, 1] > 0).all() and (want_c[:, 0] > want_c[:, 1]).all() and (want_c[:, 2] > want_c[:, -1]).all()
    assert len({tuple(r) for r in want_c}) == Q                                  # rows differ
    wc_, counts = guarded((Q, 12), np.int32, 7)
    wv_, vsd = guarded((Q, 10), np.float64, 7.0)
    assert call_vsd(lib, v, taus, counts, vsd) == 0, lib.ffb6d_last_error()
    assert np.array_equal(counts, want_c), (counts, want_c)
    assert np.array_equal(bits(vsd), bits(want_v)), (vsd, want_v)
    assert guards_intact(wc_, 7) and guards_intact(wv_, 7.0)


def test_vsd_argument_errors_return_their_code_and_write_nothing(emu_bop, vsd_case):
    lib, v = emu_bop, vsd_case
    Q = len(v["class_of"])
    small = np.zeros(16, np.int32)
    cases = [(dict(n_tau=0), -1, "n_tau"), (dict(n_tau=17), -1, "n_tau"), (dict(Q=-1), -1, "bad sizes"), (dict(Q=65536), -1, "bad sizes"),
             (dict(H=0), -1, "bad sizes"), (dict(H=1 << 16, W=1 << 15), -1, "bad sizes"), (dict(B=0), -1, "bad sizes"),
             (dict(n_cls=0), -1, "bad sizes"), (dict(depth_gt=None), -1, "null pointer"), (dict(counts=None), -1, "null pointer"),
             (dict(vsd=None), -1, "null pointer"), (dict(workspace=None), -3, "workspace"),
             (dict(workspace=_p(small), workspace_bytes=64), -3, "workspace")]
    taus = np.linspace(0.02, 0.5, 17)                                            # 17 entries behind the pointer: n_tau decides
    for kw, code, text in cases:
        counts, vsd = np.full((Q, 19), 7, np.int32), np.full((Q, 17), 7.0)
        assert call_vsd(lib, v, taus, counts, vsd, **dict(dict(n_tau=10), **kw)) == code, kw
        assert text in lib.ffb6d_last_error().decode(), (kw, lib.ffb6d_last_error())
        assert (counts == 7).all() and (vsd == 7).all(), kw
    assert not small.any()
    assert lib.ffb6d_bop_vsd_workspace_bytes(0, 4, 4) == 0 and lib.ffb6d_bop_vsd_workspace_bytes(2, 64, 65) == 512    # 2 rows x 2 runs x 18 x 4 = 288
