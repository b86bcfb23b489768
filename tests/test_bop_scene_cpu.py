"""BOP scene evaluation without a GPU (include/ffb6d_bop_scene.h): the numpy restatement (tests/bop_scene_ref.py) against closed
forms and hand-worked matchings, and the unmodified csrc/bop_scene.hip on the SIMT emulator (tests/simt) through the C ABI: every
output equals the restatement as bits, guard values around the outputs stay intact, a poisoned workspace changes nothing, argument
errors return their code and write nothing."""
import numpy as np
import pytest

import bop_scene_ref as ref
import render_ref
from test_bop_emu_cpu import _p, bits, emu_render_alone, guarded, guards_intact
from tests.simt.build import load

# a camera whose principal point is the pixel (row 12, column 16) of a 24 x 32 frame, and a rectangle at depth 1 whose edges project
# to the half pixels 4.5 / 20.5 (columns 5 .. 20) and 2.5 / 12.5 (rows 3 .. 12): 160 pixels whatever the rasteriser's tie rule
H, W = 24, 32
K = np.array([[64.0, 0.0, 16.0], [0.0, 64.0, 12.0], [0.0, 0.0, 1.0]])
RECT = render_ref.quad_mesh((4.5 - 16) / 64, (2.5 - 12) / 64, (20.5 - 16) / 64, (12.5 - 12) / 64, 1.0)
DELTA = 0.015


@pytest.fixture(scope="module")
def rect_depth():
    d = render_ref.render([None, RECT], [render_ref.pose([0, 0, 0])], [0], [1], K, 1, H, W)["depth"][0]
    d.setflags(write=False)
    return d


# ---- the restatement against closed forms -------------------------------------------------------------------------------------
def test_a_fronto_parallel_rectangle_over_an_empty_test_image_is_wholly_visible(rect_depth):
    assert np.array_equal(np.argwhere(rect_depth > 0).min(0), [3, 5]) and np.array_equal(np.argwhere(rect_depth > 0).max(0), [12, 20])
    info, fract, mask = ref.visib_row(np.zeros((H, W), np.float32), rect_depth, K, DELTA)
    assert info.tolist() == [160, 0, 160, 0, 5, 3, 16, 10, 5, 3, 16, 10] and fract == 1.0          # dt == 0 is visible, not valid
    assert mask.dtype == np.uint8 and np.array_equal(mask, (rect_depth > 0).astype(np.uint8))


def test_an_occluder_over_the_left_half_halves_the_visible_count_and_shifts_the_box(rect_depth):
    test = np.zeros((H, W), np.float32)
    test[:, :13] = 0.5                                                           # nearer than 1 - delta along every ray: columns 5 .. 12 hidden
    info, fract, mask = ref.visib_row(test, rect_depth, K, DELTA)
    assert info.tolist() == [160, 80, 80, 0, 5, 3, 16, 10, 13, 3, 8, 10] and fract == 0.5
    assert not mask[:, :13].any() and mask[3:13, 13:21].all()
    test[:, 13:] = rect_depth[:, 13:]                                            # the measured depth IS the surface on the right: supported
    info, _, _ = ref.visib_row(test, rect_depth, K, DELTA)
    assert info.tolist()[:4] == [160, 160, 80, 80]
    test[:, 13:] = 3.0                                                           # far behind: visible (the object is in front), not supported
    assert ref.visib_row(test, rect_depth, K, DELTA)[0].tolist()[:4] == [160, 160, 80, 0]


def test_a_difference_of_exactly_delta_is_visible_and_supported():
    """At the principal point X = Y = 0, so dist(z) = sqrt(z * z) = z: 1 - 0.75 = 0.25 is exact in float32."""
    obj, test = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    obj[12, 16] = 1.0
    for t, want in ((0.75, [1, 1, 1, 1]), (np.nextafter(np.float32(0.75), np.float32(0)), [1, 1, 0, 0]),
                    (1.25, [1, 1, 1, 1]), (np.nextafter(np.float32(1.25), np.float32(2)), [1, 1, 1, 0])):
        test[12, 16] = t
        info, fract, _ = ref.visib_row(test, obj, K, 0.25)
        assert info.tolist()[:4] == want, t
        assert info.tolist()[4:8] == [16, 12, 1, 1] and info.tolist()[8:] == ([16, 12, 1, 1] if want[2] else [-1] * 4)
        assert fract == float(want[2])


@pytest.mark.parametrize("value", [-1.0, np.nan, np.inf, -np.inf, 0.0])
def test_a_test_depth_that_is_no_measurement_leaves_the_pixel_visible_and_not_valid(rect_depth, value):
    test = np.full((H, W), value, np.float32)
    info, fract, _ = ref.visib_row(test, rect_depth, K, DELTA)
    assert info.tolist() == [160, 0, 160, 0, 5, 3, 16, 10, 5, 3, 16, 10] and fract == 1.0
    obj = np.where(rect_depth > 0, np.float32(value), np.float32(0))             # the same values in the object image: nothing drawn
    info, fract, mask = ref.visib_row(np.zeros((H, W), np.float32), obj, K, DELTA)
    assert info.tolist() == [0] * 4 + [-1] * 8 and fract == 0.0 and not mask.any()


def test_a_hidden_object_has_fraction_zero_and_no_box_and_a_large_one_fills_the_frame(rect_depth):
    info, fract, mask = ref.visib_row(np.full((H, W), 0.5, np.float32), rect_depth, K, DELTA)
    assert info.tolist() == [160, 160, 0, 0, 5, 3, 16, 10, -1, -1, -1, -1] and fract == 0.0 and not mask.any()
    big = render_ref.render([None, render_ref.quad_mesh(-2, -2, 2, 2, 1.0)], [render_ref.pose([0, 0, 0])], [0], [1], K, 1, H, W)["depth"][0]
    info, fract, _ = ref.visib_row(np.zeros((H, W), np.float32), big, K, DELTA)
    assert info.tolist() == [H * W, 0, H * W, 0, 0, 0, W, H, 0, 0, W, H] and fract == 1.0
    info, fract, mask = ref.visib(np.zeros((1, H, W), np.float32), big[None], [1], K[None], DELTA)      # a bad frame id
    assert info[0].tolist() == [0] * 4 + [-1] * 8 and np.isnan(fract[0]) and not mask.any()


# ---- matching by hand ---------------------------------------------------------------------------------------------------------
def one(err, score, thr, max_ests=0):
    """a single error column and threshold -> est_gt [E], gt_est [T] as lists"""
    e, t = ref.match_group(np.asarray(err, np.float64)[:, :, None], score, [thr], max_ests)
    return e[:, 0, 0].tolist(), t[:, 0, 0].tolist()


def test_greedy_by_score_is_not_the_best_assignment():
    err = [[0.1, 0.2], [0.15, 9.0]]              # the better-scored estimate 0 takes instance 0, which was the only one estimate 1 could take
    assert one(err, [0.9, 0.8], 1.0) == ([0, -1], [0, -1])
    assert one(err, [0.8, 0.9], 1.0) == ([1, 0], [1, 0])                         # the other order: both are matched


def test_ties_nans_equality_and_max_ests():
    assert one([[0.3, 0.3], [0.3, 0.3]], [0.5, 0.5], 1.0) == ([0, 1], [0, 1])   # score tie: the lower estimate first; error tie: the lower instance
    assert one([[0.3, 0.3], [0.3, 0.3]], [0.5, 0.6], 1.0) == ([1, 0], [1, 0])
    assert one([[np.nan, 0.3], [0.1, 0.2]], [0.9, 0.1], 1.0) == ([1, 0], [1, 0])                          # a NaN error never matches
    assert one([[0.1, 0.2], [0.1, 0.2]], [np.nan, 0.1], 1.0) == ([1, 0], [1, 0])                          # a NaN score goes last
    assert one([[0.1, 0.2], [0.1, 0.2]], [np.nan, -np.inf], 1.0) == ([0, 1], [0, 1])                      # ... and ties with -inf
    assert one([[0.5]], [1.0], 0.5) == ([-1], [-1]) and one([[0.5]], [1.0], np.nextafter(0.5, 1)) == ([0], [0])      # equality is no match
    assert one([[np.inf]], [1.0], np.inf) == ([-1], [-1])
    assert one([[0.1, 0.2], [0.1, 0.2]], [0.1, 0.9], 1.0, max_ests=1) == ([-1, 0], [1, -1])             # only the best estimate is considered
    assert one([[0.1, 0.2], [0.1, 0.2]], [0.1, 0.9], 1.0, max_ests=2) == ([1, 0], [1, 0])
    assert one([[0.1, 0.2], [0.1, 0.2]], [0.1, 0.9], 1.0, max_ests=5) == ([1, 0], [1, 0])


def test_empty_groups_and_single_pairs():
    e, t = ref.match_group(np.zeros((0, 3, 2)), [], [0.5, 1.0])
    assert e.shape == (0, 2, 2) and t.shape == (3, 2, 2) and (t == -1).all()
    e, t = ref.match_group(np.zeros((3, 0, 2)), [1, 2, 3], [0.5, 1.0])
    assert t.shape == (0, 2, 2) and e.shape == (3, 2, 2) and (e == -1).all()
    rng = np.random.RandomState(0)
    err, thr = rng.rand(1, 1, 10), rng.rand(10)
    err[0, 0, 3] = np.nan
    e, t = ref.match_group(err, [0.3], thr)
    want = np.where(err[0, 0][:, None] < thr[None, :], 0, -1)                    # for a 1 x 1 group the result is err < thr
    assert np.array_equal(e[0], want) and np.array_equal(t[0], want) and (want == 0).any() and (want == -1).any()


def test_pair_rows_groups_by_frame_and_class():
    from ffb6d_amd import bop
    g = bop.pair_rows(est_class=[5, 1, 1, 2, 1], est_frame=[0, 1, 0, 0, 0], gt_class=[1, 1, 5, 7], gt_frame=[0, 0, 0, 1])
    assert list(zip(g["group_frame"], g["group_class"])) == [(0, 1), (0, 2), (0, 5), (1, 1), (1, 7)]
    assert g["est_begin"].tolist() == [0, 2, 3, 4, 5, 5] and g["gt_begin"].tolist() == [0, 2, 2, 3, 3, 4] and g["pair_begin"].tolist() == [0, 4, 4, 5, 5, 5]
    assert g["est_order"].tolist() == [2, 4, 3, 0, 1] and g["gt_order"].tolist() == [0, 1, 2, 3]
    assert g["pair_est"].tolist() == [2, 2, 4, 4, 0] and g["pair_gt"].tolist() == [0, 1, 0, 1, 2] and g["pair_group"].tolist() == [0, 0, 0, 0, 2]
    assert g["est_begin"].dtype == np.int32 and g["pair_begin"].dtype == np.int64


# ---- the unmodified kernels on the SIMT emulator ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu_scene():
    """the emulated library (tests/simt/build.py)"""
    return load()


def call_visib(lib, v, out_info, out_fract, out_mask, ws=None, **kw):
    a = dict(depth_test=_p(v["depth_test"]), depth_obj=_p(v["depth_obj"]), frame_of=_p(v["frame_of"]), Q=len(v["frame_of"]), K=_p(v["K"]),
             B=v["B"], H=v["H"], W=v["W"], delta=v["delta"], info=_p(out_info), visib_fract=_p(out_fract), mask_visib=_p(out_mask))
    a.update(kw)
    if ws is None:
        ws = np.full(max(lib.ffb6d_bop_visib_workspace_bytes(a["Q"], a["H"], a["W"]), 4) // 4, -12345, np.int32)            # dirty
    a.setdefault("workspace", _p(ws))
    a.setdefault("workspace_bytes", ws.nbytes)
    return lib.ffb6d_bop_visib_f32(*a.values(), None)


# 5 x 7 and 67 x 63: odd, single floats (the second with two runs and a tail); 8 x 8: 16-byte accesses; 65 x 64: 16-byte accesses, two runs
@pytest.mark.parametrize("size", [(5, 7), (8, 8), (65, 64), (67, 63)], ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("masks", [False, True], ids=["nomask", "mask"])
def test_visibility_on_the_emulator_equals_the_restatement_as_bits(emu_scene, size, masks):
    lib = emu_scene
    v = ref.visib_image_case(*size, Q=3, bad_row=1)
    Q, HW = 3, size[0] * size[1]
    want_i, want_f, want_m = ref.visib(v["depth_test"], v["depth_obj"], v["frame_of"], v["K"], v["delta"])
    # the case holds what it tests: hidden and visible pixels in both good rows, supported ones in row 0 (row 2 lies behind its frame's surface)
    assert (want_i[[0, 2], 0] > want_i[[0, 2], 2]).all() and (want_i[[0, 2], 2] > 0).all() and 0 < want_i[0, 3] < want_i[0, 1] and np.isnan(want_f[1])
    wi_, info = guarded((Q, 12), np.int32, 7)
    wf_, fract = guarded((Q,), np.float64, 7.0)
    wm_, mask = guarded((Q,) + size, np.uint8, 7)
    assert call_visib(lib, v, info, fract, mask if masks else None) == 0, lib.ffb6d_last_error()
    assert np.array_equal(info, want_i), (info, want_i)
    assert np.array_equal(bits(fract), bits(want_f))
    assert guards_intact(wi_, 7) and guards_intact(wf_, 7.0) and guards_intact(wm_, 7)
    assert np.array_equal(mask, want_m) if masks else (mask == 7).all()
    # the workspace a previous call left behind, poisoned: the same outputs
    n = lib.ffb6d_bop_visib_workspace_bytes(Q, *size) // 4
    assert n * 4 == (Q * -(-HW // 4096) * 12 * 4 + 255) // 256 * 256
    ws = np.full(n + 2 * 8, 7, np.int32)
    assert call_visib(lib, v, info, fract, None, workspace=ws[8:].ctypes.data, workspace_bytes=4 * n) == 0
    ws[8:8 + n] = np.iinfo(np.int32).max
    info[:], fract[:] = 5, 5.0
    assert call_visib(lib, v, info, fract, None, workspace=ws[8:].ctypes.data, workspace_bytes=4 * n) == 0
    assert np.array_equal(info, want_i) and np.array_equal(bits(fract), bits(want_f)) and (ws[:8] == 7).all() and (ws[-8:] == 7).all()
    # an unaligned mask or image takes the scalar path: the same outputs
    if masks and HW % 4 == 0:
        odd = np.full(Q * HW + 9, 7, np.uint8)
        assert call_visib(lib, v, info, fract, None, mask_visib=odd[1:].ctypes.data) == 0
        assert np.array_equal(odd[1:1 + Q * HW].reshape(want_m.shape), want_m) and odd[0] == 7 and (odd[1 + Q * HW:] == 7).all()


def test_a_rendered_rectangle_on_the_emulator_gives_the_closed_form(emu_scene, rect_depth):
    lib = emu_scene
    v = dict(class_of=np.array([1], np.int32), frame_of=np.array([0], np.int32), K=K[None].copy(), B=1, H=H, W=W, delta=DELTA)
    depth = emu_render_alone(lib, render_ref.pack([None, RECT]), v, render_ref.pose([0, 0, 0])[None])
    assert np.array_equal(bits(depth[0]), bits(rect_depth))
    test = np.zeros((1, H, W), np.float32)
    test[:, :, :13] = 0.5
    v.update(depth_obj=depth, depth_test=test)
    info, fract, mask = np.zeros((1, 12), np.int32), np.zeros(1), np.zeros((1, H, W), np.uint8)
    assert call_visib(lib, v, info, fract, mask) == 0, lib.ffb6d_last_error()
    assert info[0].tolist() == [160, 80, 80, 0, 5, 3, 16, 10, 13, 3, 8, 10] and fract[0] == 0.5 and mask.sum() == 80
    assert call_visib(lib, v, info, fract, mask, Q=0, info=None) == 0            # nothing to do


def test_visibility_argument_errors_return_their_code_and_write_nothing(emu_scene):
    lib = emu_scene
    v = ref.visib_image_case(8, 8, Q=3)
    small = np.zeros(16, np.int32)
    cases = [(dict(Q=-1), -1, "bad sizes"), (dict(Q=65536), -1, "bad sizes"), (dict(H=0), -1, "bad sizes"), (dict(W=-3), -1, "bad sizes"),
             (dict(H=1 << 16, W=1 << 15), -1, "bad sizes"), (dict(B=0), -1, "bad sizes"), (dict(depth_obj=None), -1, "null pointer"),
             (dict(info=None), -1, "null pointer"), (dict(visib_fract=None), -1, "null pointer"), (dict(workspace=None), -3, "workspace"),
             (dict(workspace=_p(small), workspace_bytes=64), -3, "workspace")]
    for kw, code, text in cases:
        info, fract, mask = np.full((3, 12), 7, np.int32), np.full(3, 7.0), np.full((3, 8, 8), 7, np.uint8)
        assert call_visib(lib, v, info, fract, mask, **kw) == code, kw
        assert text in lib.ffb6d_last_error().decode(), (kw, lib.ffb6d_last_error())
        assert (info == 7).all() and (fract == 7).all() and (mask == 7).all(), kw
    assert not small.any()
    assert lib.ffb6d_bop_visib_workspace_bytes(0, 4, 4) == 0 and lib.ffb6d_bop_visib_workspace_bytes(2, 64, 65) == 256     # 2 x 2 x 12 x 4 = 192


def call_match(lib, c, out_est_gt, out_gt_est, **kw):
    tb = c["tables"]
    a = dict(est_begin=_p(tb["est_begin"]), gt_begin=_p(tb["gt_begin"]), pair_begin=_p(tb["pair_begin"]), G=len(tb["est_begin"]) - 1,
             Etot=int(tb["est_begin"][-1]), Gtot=int(tb["gt_begin"][-1]), Npairs=int(tb["pair_begin"][-1]), err=_p(c["err"]), n_col=c["n_col"],
             score=_p(c["score"]), thr=_p(c["thr"]), n_thr=c["n_thr"], max_ests=_p(c["max_ests"]), est_gt=_p(out_est_gt), gt_est=_p(out_gt_est),
             workspace=None, workspace_bytes=0)
    a.update(kw)
    return lib.ffb6d_bop_match_f64(*a.values(), None)


def check_tables(lib, tb, max_ests=None, n_col=1, n_thr=1, **kw):
    a = dict(est_begin=_p(tb["est_begin"]), gt_begin=_p(tb["gt_begin"]), pair_begin=_p(tb["pair_begin"]), max_ests=_p(max_ests),
             G=len(tb["est_begin"]) - 1, Etot=int(tb["est_begin"][-1]), Gtot=int(tb["gt_begin"][-1]), Npairs=int(tb["pair_begin"][-1]),
             n_col=n_col, n_thr=n_thr)
    a.update(kw)
    return lib.ffb6d_bop_match_check(*a.values())


@pytest.mark.parametrize("n_col,n_thr,with_max", [(1, 1, True), (1, 10, False), (10, 10, True), (16, 16, True)])
def test_matching_on_the_emulator_equals_the_restatement(emu_scene, n_col, n_thr, with_max):
    lib = emu_scene
    sizes = ref.GROUP_SIZES if n_col * n_thr <= 100 else ((2, 2), (0, 1), (7, 3), (3, 0), (9, 9))
    c = ref.match_case(n_col, n_thr, sizes, with_max=with_max)
    tb = c["tables"]
    assert check_tables(lib, tb, c["max_ests"], n_col, n_thr) == 0, lib.ffb6d_last_error()
    want_e, want_g = ref.match(tb, c["err"], c["score"], c["thr"], c["max_ests"])
    assert (want_e >= -1).all() and (want_g >= -1).all() and (want_e >= 0).any() and (want_e == -1).any()
    we_, est_gt = guarded(want_e.shape, np.int32, 7)
    wg_, gt_est = guarded(want_g.shape, np.int32, 7)
    assert call_match(lib, c, est_gt, gt_est) == 0, lib.ffb6d_last_error()
    assert np.array_equal(est_gt, want_e) and np.array_equal(gt_est, want_g)
    assert guards_intact(we_, 7) and guards_intact(wg_, 7)
    assert lib.ffb6d_bop_match_workspace_bytes(len(sizes), n_col, n_thr) == 0


def test_match_check_refuses_bad_tables_and_the_kernel_does_not_follow_them(emu_scene):
    lib = emu_scene
    c = ref.match_case(2, 3, ((2, 2), (3, 1), (1, 4)))
    tb = c["tables"]
    assert check_tables(lib, tb, c["max_ests"], 2, 3) == 0
    assert check_tables(lib, ref.group_tables(((64, 64), (0, 0))), None) == 0

    def changed(key, at, value):
        out = {k: v.copy() for k, v in tb.items()}
        out[key][at] = value
        return out

    for bad, text in ((changed("est_begin", 1, 6), "monotone"), (changed("gt_begin", 2, 1), "monotone"), (changed("pair_begin", 1, 5), "pair_begin"),
                      (changed("pair_begin", 0, 1), "begin at 0"), (ref.group_tables(((65, 1),)), "at most 64"), (ref.group_tables(((1, 65),)), "at most 64")):
        assert check_tables(lib, bad) == -1, text
        assert text in lib.ffb6d_last_error().decode(), (text, lib.ffb6d_last_error())
    assert check_tables(lib, tb, np.array([0, -1, 2], np.int32)) == -1 and "max_ests" in lib.ffb6d_last_error().decode()
    assert check_tables(lib, tb, n_col=17) == -1 and check_tables(lib, tb, n_thr=0) == -1 and check_tables(lib, tb, Etot=5) == -1
    assert check_tables(lib, tb, est_begin=None) == -1 and "null pointer" in lib.ffb6d_last_error().decode()
    # the kernel, given the tables the check refuses: the broken group is -1, its neighbours are matched, the guards stay
    want_e, want_g = ref.match(tb, c["err"], c["score"], c["thr"], c["max_ests"])
    for bad in (changed("pair_begin", 1, 5), changed("pair_begin", 2, 10 ** 12), changed("pair_begin", 1, -3)):
        we_, est_gt = guarded(want_e.shape, np.int32, 7)
        wg_, gt_est = guarded(want_g.shape, np.int32, 7)
        assert call_match(lib, dict(c, tables=bad), est_gt, gt_est) == 0
        assert guards_intact(we_, 7) and guards_intact(wg_, 7)
        broken = [g for g in range(3) if bad["pair_begin"][g + 1] - bad["pair_begin"][g] != (4, 3, 4)[g] or bad["pair_begin"][g] != tb["pair_begin"][g]]
        for g in range(3):
            e = slice(tb["est_begin"][g], tb["est_begin"][g + 1])
            assert (est_gt[e] == -1).all() if g in broken else np.array_equal(est_gt[e], want_e[e]), (g, broken)
    many = ref.group_tables(((65, 1), (1, 1)))                                   # 65 estimates: the group is -1 in at most 64 entries, nothing else
    cm = dict(tables=many, err=np.zeros((66, 1)), score=np.ones(66, np.float32), thr=np.ones((2, 1)), n_col=1, n_thr=1, max_ests=None)
    we_, est_gt = guarded((66, 1, 1), np.int32, 7)
    wg_, gt_est = guarded((2, 1, 1), np.int32, 7)
    assert call_match(lib, cm, est_gt, gt_est) == 0
    assert (est_gt[:64] == -1).all() and est_gt[64, 0, 0] == 7 and est_gt[65, 0, 0] == 0 and gt_est[:, 0, 0].tolist() == [-1, 0]
    assert guards_intact(we_, 7) and guards_intact(wg_, 7)


def test_match_argument_errors_return_their_code_and_write_nothing(emu_scene):
    lib = emu_scene
    c = ref.match_case(2, 3, ((2, 2), (3, 1)))
    for kw, text in ((dict(G=-1), "bad sizes"), (dict(Etot=-1), "bad sizes"), (dict(Gtot=1 << 31), "bad sizes"), (dict(n_col=0), "n_col"),
                     (dict(n_col=17), "n_col"), (dict(n_thr=17), "n_col"), (dict(err=None), "null pointer"), (dict(thr=None), "null pointer"),
                     (dict(score=None), "null pointer"), (dict(gt_est=None), "null pointer"), (dict(pair_begin=None), "null pointer")):
        est_gt, gt_est = np.full((5, 2, 3), 7, np.int32), np.full((3, 2, 3), 7, np.int32)
        assert call_match(lib, c, est_gt, gt_est, **kw) == -1, kw
        assert text in lib.ffb6d_last_error().decode(), (kw, lib.ffb6d_last_error())
        assert (est_gt == 7).all() and (gt_est == 7).all(), kw
    assert call_match(lib, c, None, None, G=0) == 0                              # nothing to do
