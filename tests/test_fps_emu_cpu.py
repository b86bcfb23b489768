"""csrc/fps.hip on the SIMT emulator (tests/simt), without a GPU: the unmodified kernel source compiled for the host and run through
the C ABI of include/ffb6d_fps.h.  Sets of n in {0, 1, 63, 64, 65, 300} go in one call, lattice points and duplicates, with m = 8
and with m above every n; both forms are forced in turn and both start modes are run.  idx, out_pts and out_dist equal the numpy
restatement (tests/fps_ref.py) bit for bit; argument errors return their code and write nothing.  The box statistics are held
against the restatement and against hand-computed vectors: the reference's MeshUtils imports OpenCV and plyfile, which the build
image lacks, so nothing of it can be run to record a golden."""
import numpy as np
import pytest

import fps_ref
from tests.simt.build import load, ptr as _p

SIZES = (0, 1, 63, 64, 65, 300)
FILL = 7


@pytest.fixture(scope="module")
def emu_fps():
    """the emulated library (tests/simt/build.py)"""
    return load()


@pytest.fixture(scope="module")
def sets():
    """lattice sets and duplicate sets of every size, an empty one among them"""
    out = [fps_ref.lattice_set(n, 900 + n) for n in SIZES] + [fps_ref.duplicate_set(n, 950 + n) for n in SIZES[1:]]
    for a in out:
        a.setflags(write=False)
    return out


def fresh(S, m):
    return dict(idx=np.full((S, m), FILL, np.int32), out_pts=np.full((S, m, 3), FILL, np.float32),
                out_dist=np.full((S, m), FILL, np.float32))


def call(lib, sets, samples, start, out, ws=None, **kw):
    """ffb6d_fps_f32 with numpy arrays as "device" memory; kw overrides arguments by name"""
    pts, begin = fps_ref.pack(sets)
    a = dict(pts=_p(pts), begin=_p(begin), S=len(sets), total=int(begin[-1]), max_n=max(len(s) for s in sets), m=samples,
             start=_p(start), idx=_p(out.get("idx")), out_pts=_p(out.get("out_pts")), out_dist=_p(out.get("out_dist")))
    a.update(kw)
    if ws is None:
        ws = np.zeros(max(lib.ffb6d_fps_workspace_bytes(a["S"], a["max_n"], a["m"]), 1), np.uint8)
    a.setdefault("workspace", _p(ws))
    a.setdefault("workspace_bytes", ws.nbytes)
    return lib.ffb6d_fps_f32(*a.values(), None)


def assert_same_bits(got, want, what):
    for k, w in zip(("idx", "out_pts", "out_dist"), want):
        if k in got:
            g = got[k]
            assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
            assert np.array_equal(g.view(np.int32), w.view(np.int32)), (what, k, int(np.count_nonzero(g != w)))


def test_the_sets_have_what_they_are_meant_to_test(sets):
    idx, _, dist = fps_ref.fps_batch(sets, 8)
    assert (idx[0] == -1).all() and not dist[0].any()                          # the empty set
    assert (idx[1] == 0).all()                                                 # one point: the index-0 rule from the second pick on
    d = sets[-1]
    assert len(d) == 300 and np.array_equal(d[:150], d[150:])
    idx, _, dist = fps_ref.fps_batch(sets, 301)
    assert (dist[-1][150:] == 0).all() and (idx[-1][150:] == 0).all() and (dist[-1][1:150] > 0).all()      # 150 distinct points, then index 0
    lat = fps_ref.fps(sets[5], 8, None)[2]
    assert len(np.unique(lat)) < len(lat)                                      # ties among the lattice's distances


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("mode", ["center", "start"])
@pytest.mark.parametrize("m", [8, 301])
def test_every_output_on_the_emulator_equals_the_restatement_as_bits(emu_fps, sets, form, mode, m):
    """m = 301 is above every n; the emulator's time goes with sets x m, so that run keeps one duplicate set (n = 65: 33 distinct
    points, then the index-0 rule) next to the lattice sets of every size"""
    lib = emu_fps
    if m > 8:
        sets = sets[:len(SIZES)] + [s for s in sets[len(SIZES):] if len(s) == 65]
    start = None if mode == "center" else np.array([max(len(s) - 1, 0) * (i % 3) // 2 for i, s in enumerate(sets)], np.int32)
    want = fps_ref.fps_batch(sets, m, start)
    out = fresh(len(sets), m)
    lib.ffb6d_fps_set_form(form)
    try:
        assert call(lib, sets, m, start, out) == 0, lib.ffb6d_last_error()
    finally:
        lib.ffb6d_fps_set_form(0)
    assert_same_bits(out, want, (form, mode, m))


@pytest.mark.parametrize("form", [1, 2])
def test_sets_of_more_than_two_points_per_lane(emu_fps, form):
    """above 2048 points the resident form keeps 8 points per lane instead of 2: another instance of the kernel"""
    lib = emu_fps
    big = [fps_ref.lattice_set(2049, 31), fps_ref.duplicate_set(2500, 32)]
    for start in (None, np.array([2048, 1250], np.int32)):
        out = fresh(2, 6)
        lib.ffb6d_fps_set_form(form)
        try:
            assert call(lib, big, 6, start, out) == 0, lib.ffb6d_last_error()
        finally:
            lib.ffb6d_fps_set_form(0)
        assert_same_bits(out, fps_ref.fps_batch(big, 6, start), (form, start))


def test_outputs_are_optional_tables_are_clamped_and_starts_too(emu_fps, sets):
    lib = emu_fps
    want = fps_ref.fps_batch(sets, 8)
    for keep in (("idx",), ("out_pts",), ("out_dist", "idx")):
        out = {k: v for k, v in fresh(len(sets), 8).items() if k in keep}
        assert call(lib, sets, 8, None, out) == 0, lib.ffb6d_last_error()
        assert_same_bits(out, want, keep)
    # a table that runs past the array is cut at `total`, a set above max_n at max_n, a start outside the set is clamped into it
    pts, begin = fps_ref.pack(sets)
    begin = begin.copy()
    begin[-1] += 1000
    out = fresh(len(sets), 8)
    assert call(lib, sets, 8, None, out, begin=_p(begin)) == 0, lib.ffb6d_last_error()
    assert_same_bits(out, want, "long table")
    cut = [s[:100] for s in sets]
    for form in (1, 2):
        out = fresh(len(sets), 8)
        lib.ffb6d_fps_set_form(form)
        try:
            assert call(lib, sets, 8, None, out, max_n=100) == 0, lib.ffb6d_last_error()
        finally:
            lib.ffb6d_fps_set_form(0)
        assert_same_bits(out, fps_ref.fps_batch(cut, 8), ("max_n", form))
    start = np.array([-5 if i % 2 else 10 ** 6 for i in range(len(sets))], np.int32)
    out = fresh(len(sets), 8)
    assert call(lib, sets, 8, start, out) == 0, lib.ffb6d_last_error()
    assert_same_bits(out, fps_ref.fps_batch(sets, 8, start), "start")


def test_argument_errors_return_their_code_and_leave_the_outputs_untouched(emu_fps, sets):
    lib = emu_fps
    assert lib.ffb6d_fps_resident_capacity() >= 8192
    assert lib.ffb6d_fps_workspace_bytes(3, 300, 8) == 0 and lib.ffb6d_fps_workspace_bytes(0, 300, 8) == 0
    small = np.zeros(64, np.uint8)
    cap = lib.ffb6d_fps_resident_capacity()
    cases = [(0, dict(m=0), -1, "bad sizes"), (0, dict(S=0), -1, "bad sizes"), (0, dict(max_n=-1), -1, "bad sizes"),
             (0, dict(max_n=1 << 31), -1, "bad sizes"), (0, dict(total=-1), -1, "bad sizes"), (0, dict(begin=None), -1, "null pointer"),
             (0, dict(pts=None), -1, "null pointer"), (0, dict(idx=None, out_pts=None, out_dist=None), -1, "no output"),
             (1, dict(max_n=cap + 1), -1, "resident capacity"),
             (2, dict(workspace=None), -3, "workspace"), (2, dict(workspace=_p(small), workspace_bytes=64), -3, "workspace")]
    for form, kw, code, text in cases:
        out = fresh(len(sets), 8)
        lib.ffb6d_fps_set_form(form)
        try:
            assert lib.ffb6d_fps_workspace_bytes(len(sets), 300, 8) == (len(sets) * 300 * 4 + 255) // 256 * 256 * (form == 2)
            assert call(lib, sets, 8, None, out, **kw) == code, kw
        finally:
            lib.ffb6d_fps_set_form(0)
        assert text in lib.ffb6d_last_error().decode(), (kw, lib.ffb6d_last_error())
        for k, v in out.items():
            assert (v == FILL).all(), (kw, k)
    assert not small.any()
    pts, begin = fps_ref.pack(sets)
    box = [np.full((len(sets), 8, 3), FILL, np.float32), np.full((len(sets), 3), FILL, np.float32), np.full(len(sets), FILL, np.float32)]
    for kw in (dict(S=0), dict(total=-1), dict(begin=None), dict(pts=None), dict(out=None)):
        a = dict(pts=_p(pts), begin=_p(begin), S=len(sets), total=int(begin[-1]))
        a.update({k: v for k, v in kw.items() if k != "out"})
        outs = [None] * 3 if "out" in kw else [_p(b) for b in box]
        assert lib.ffb6d_box_info_f32(*a.values(), *outs, None) == -1, kw
        assert all((b == FILL).all() for b in box), kw


def test_box_statistics_equal_the_restatement_and_hand_computed_vectors(emu_fps, sets):
    lib = emu_fps
    hand = np.array([[1, -2, 3], [-1, 2, 7], [0, 0, 4]], np.float32)           # box [-1,1] x [-2,2] x [3,7]
    all_sets = list(sets) + [hand]
    pts, begin = fps_ref.pack(all_sets)
    S = len(all_sets)
    corners, ctr, radius = np.full((S, 8, 3), FILL, np.float32), np.full((S, 3), FILL, np.float32), np.full(S, FILL, np.float32)
    assert lib.ffb6d_box_info_f32(_p(pts), _p(begin), S, int(begin[-1]), _p(corners), _p(ctr), _p(radius), None) == 0, lib.ffb6d_last_error()
    for s, p in enumerate(all_sets):
        c, m, r = fps_ref.box(p)
        assert np.array_equal(corners[s], c) and np.array_equal(ctr[s], m) and radius[s].view(np.int32) == r.view(np.int32), s
        c64, m64, r64 = fps_ref.box64(p)
        assert np.array_equal(corners[s], c64) and np.array_equal(ctr[s], m64.astype(np.float32)) and abs(radius[s] - r64) <= 1e-6 * r64, s
    assert np.array_equal(corners[-1], [[-1, -2, 3], [-1, -2, 7], [-1, 2, 3], [-1, 2, 7], [1, -2, 3], [1, -2, 7], [1, 2, 3], [1, 2, 7]])
    assert np.array_equal(ctr[-1], [0, 0, 5]) and radius[-1] == np.float32(3)  # diagonal (2, 4, 4): length 6
    assert not corners[0].any() and not ctr[0].any() and radius[0] == 0        # the empty set
    # each output alone
    only = np.full(S, FILL, np.float32)
    assert lib.ffb6d_box_info_f32(_p(pts), _p(begin), S, int(begin[-1]), None, None, _p(only), None) == 0
    assert np.array_equal(only, radius)
