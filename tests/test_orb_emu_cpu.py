"""csrc/orb.hip on the SIMT emulator (tests/simt), without a GPU: the unmodified kernel source compiled for the host and run through
the C ABI of include/ffb6d_orb.h.  Three frames of different content go in one call (isolated dots, uniform noise, a second noise
image); 48 x 64 and 37 x 53 pixels, 1 and 3 levels, edge 4, quotas above and well below the candidate counts, so that the top-n
cut and its tie rule are exercised.  count, kps and resp, the lifted slots and the compacted point sets equal the numpy restatement
(tests/orb_ref.py) bit for bit; argument errors return their code and write nothing."""
import numpy as np
import pytest

import orb_ref
from tests.simt.build import load, ptr as _p

FILL = 7


@pytest.fixture(scope="module")
def emu_orb():
    """the emulated library (tests/simt/build.py)"""
    return load()


def fresh(F, Q):
    return dict(count=np.full(F, FILL, np.int32), kps=np.full((F, Q, 5), FILL, np.int32), resp=np.full((F, Q), FILL, np.int64))


def call(lib, frames_u8, levels, thr, border, quotas, out, ws=None, **kw):
    """ffb6d_orb_detect_u8 with numpy arrays as "device" memory; kw overrides arguments by name"""
    F, _, H, W = frames_u8.shape
    quota = np.ascontiguousarray(quotas, np.int32)
    a = dict(rgb=_p(frames_u8), F=F, H=H, W=W, n_levels=levels, fast_threshold=thr, edge=border, quota=_p(quota), count=_p(out["count"]),
             kps=_p(out["kps"]), resp=_p(out["resp"]))
    a.update(kw)
    if ws is None:
        ws = np.zeros(max(lib.ffb6d_orb_workspace_bytes(F, H, W, levels), 1), np.uint8)
    a.setdefault("workspace", _p(ws))
    a.setdefault("workspace_bytes", ws.nbytes)
    return lib.ffb6d_orb_detect_u8(*a.values(), None)


def assert_same(got, want, what):
    for k, w in zip(("count", "kps", "resp"), want):
        g = got[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        assert np.array_equal(g, w), (what, k, int(np.count_nonzero(g != w)))


CASES = orb_ref.CASES


@pytest.mark.parametrize("size,L,quota", CASES)
def test_the_detector_on_the_emulator_equals_the_restatement_as_bits(emu_orb, size, L, quota):
    rgb = orb_ref.frames(*size)
    count, kps, resp, n_cand = orb_ref.detect(rgb, L, 20, 4, quota, want_counts=True)
    if size == (48, 64):
        assert n_cand[0, 0] == 6 and n_cand[1, 0] > 100 and n_cand[2, 0] > 100              # the noise frames: a few hundred candidates
    if min(quota) < 20:
        assert (n_cand[1:, :] > np.asarray(quota)[None]).any()                              # the cut is exercised
    if max(quota) >= 200:
        assert (n_cand[:, 0] < max(quota)).all()                                            # and so are rows past count
    out = fresh(len(rgb), int(sum(quota)))
    assert call(emu_orb, rgb, L, 20, 4, quota, out) == 0, emu_orb.ffb6d_last_error()
    assert_same(out, (count, kps, resp), (size, L, quota))


@pytest.mark.parametrize("quota", [50, 3200])
def test_more_candidates_than_a_workgroup_has_threads_and_than_one_chunk_holds(emu_orb, quota):
    """160 x 220 noise: about 3000 candidates on one level, 35 tiles with partial ones at two sides"""
    rgb = orb_ref.noise_rgb(160, 220, 21)[None]
    count, kps, resp, n_cand = orb_ref.detect(rgb, 1, 20, 4, (quota,), want_counts=True)
    assert 2048 < n_cand[0, 0] < 3200
    out = fresh(1, quota)
    assert call(emu_orb, rgb, 1, 20, 4, (quota,), out) == 0, emu_orb.ffb6d_last_error()
    assert_same(out, (count, kps, resp), quota)


def test_thousands_of_equal_responses_are_cut_by_pixel_index(emu_orb):
    """2401 identical dots, more than one LDS chunk: the cut among equal responses is by pixel index alone"""
    rgb = orb_ref.as_rgb(orb_ref.lattice_dots_image())[None].copy()
    count, kps, resp, n_cand = orb_ref.detect(rgb, 1, 20, 4, (100,), want_counts=True)
    assert n_cand[0, 0] == 49 * 49 and count[0] == 100 and len(set(resp[0].tolist())) == 1
    assert kps[0, :3, :2].tolist() == [[5, 5], [13, 5], [21, 5]] and kps[0, 49, :2].tolist() == [5, 13]
    out = fresh(1, 100)
    assert call(emu_orb, rgb, 1, 20, 4, (100,), out) == 0, emu_orb.ffb6d_last_error()
    assert_same(out, (count, kps, resp), "lattice")


def test_equal_responses_are_ordered_by_pixel_index_and_cut_there(emu_orb):
    """the two 200-dots tie: with a quota of 2 the cut falls between them"""
    rgb = orb_ref.as_rgb(orb_ref.dots_image())[None].copy()
    for q in (2, 3):
        want = orb_ref.detect(rgb, 1, 20, 4, (q,))
        assert want[1][0, 1].tolist() == [10, 10, 0, 10, 10] and want[0][0] == q
        out = fresh(1, q)
        assert call(emu_orb, rgb, 1, 20, 4, (q,), out) == 0, emu_orb.ffb6d_last_error()
        assert_same(out, want, q)


def run_lift(lib, kps, count, depth, visible, T, K, min_pixels, S, V):
    F, Q = kps.shape[:2]
    H, W = depth.shape[1:]
    slot_pts, slot_ok = np.full((F, Q, 3), FILL, np.float32), np.full((F, Q), FILL, np.int32)
    rc = lib.ffb6d_orb_lift_f32(_p(kps), _p(count), _p(depth), _p(visible), _p(T), F, Q, H, W, K[0, 0], K[1, 1], K[0, 2], K[1, 2], min_pixels,
                                _p(slot_pts), _p(slot_ok), None)
    assert rc == 0, lib.ffb6d_last_error()
    pts, begin, n_found = np.full((F * Q, 3), FILL, np.float32), np.full(S + 1, FILL, np.int64), np.full(S, FILL, np.int32)
    rc = lib.ffb6d_orb_compact_f32(_p(slot_pts), _p(slot_ok), S, V, Q, _p(pts), _p(begin), _p(n_found), None)
    assert rc == 0, lib.ffb6d_last_error()
    return slot_pts, slot_ok, pts, begin, n_found


@pytest.mark.parametrize("S,V", [(2, 2), (4, 1), (1, 4)])
def test_lift_and_compaction_equal_the_restatement_as_bits(emu_orb, S, V):
    kps, count, depth, visible, T, K = orb_ref.lift_case()
    want_pts, want_ok = orb_ref.lift(kps, count, depth, visible, T, K, 50)
    assert want_ok[0].tolist() == [1, 0, 1, 1, 0] + [1] * 7 and want_ok[1].tolist() == [0] + [1] * 5 + [0] * 6      # dropped rows
    assert not want_ok[2:].any()                                                   # below min_pixels, and no keypoints
    slot_pts, slot_ok, pts, begin, n_found = run_lift(emu_orb, kps, count, depth, visible, T, K, 50, S, V)
    assert np.array_equal(slot_ok, want_ok) and np.array_equal(slot_pts.view(np.int32), want_pts.view(np.int32))
    w_pts, w_begin, w_found = orb_ref.compact(want_pts, want_ok, S, V)
    assert np.array_equal(n_found, w_found) and np.array_equal(begin, w_begin)
    assert np.array_equal(pts.view(np.int32), w_pts.view(np.int32))
    assert n_found.tolist() == {(2, 2): [15, 0], (4, 1): [10, 5, 0, 0], (1, 4): [15]}[(S, V)]


def test_compaction_of_more_rows_than_a_workgroup_has_threads(emu_orb):
    """V * Q = 700 rows per object: three rounds of the ordered scan, the last one partial"""
    rs = np.random.RandomState(3)
    S, V, Q = 3, 2, 350
    slot_ok = (rs.uniform(size=(S * V, Q)) < 0.4).astype(np.int32)
    slot_ok[2:4] = 0                                                               # an object with no point
    slot_pts = rs.normal(size=(S * V, Q, 3)).astype(np.float32)
    pts, begin, n_found = np.full((S * V * Q, 3), FILL, np.float32), np.full(S + 1, FILL, np.int64), np.full(S, FILL, np.int32)
    assert emu_orb.ffb6d_orb_compact_f32(_p(slot_pts), _p(slot_ok), S, V, Q, _p(pts), _p(begin), _p(n_found), None) == 0
    w_pts, w_begin, w_found = orb_ref.compact(slot_pts, slot_ok, S, V)
    assert w_found[1] == 0 and np.array_equal(n_found, w_found) and np.array_equal(begin, w_begin)
    assert np.array_equal(pts.view(np.int32), w_pts.view(np.int32))


def test_argument_errors_return_their_code_and_leave_the_outputs_untouched(emu_orb):
    lib = emu_orb
    rgb = orb_ref.frames(48, 64)
    quota = (16, 8, 4)
    need = lib.ffb6d_orb_workspace_bytes(3, 48, 64, 3)
    sizes = orb_ref.level_sizes(48, 64, 3)
    a256 = lambda n: (n + 255) // 256 * 256                                                                       # noqa: E731
    cand = sum(3 * ((h + 1) // 2) * ((w + 1) // 2) for h, w in sizes)
    assert need == sum(a256(3 * h * w) for h, w in sizes) + a256(4 * 3 * 3) + a256(8 * cand) + a256(4 * cand)
    assert lib.ffb6d_orb_workspace_bytes(0, 48, 64, 3) == 0 and lib.ffb6d_orb_workspace_bytes(3, 48, 64, 9) == 0
    short = np.zeros(need - 1, np.uint8)
    negative, none = np.array([4, -1, 4], np.int32), np.zeros(3, np.int32)
    cases = [(dict(edge=3), -1, "edge"), (dict(n_levels=0), -1, "bad sizes"), (dict(n_levels=9), -1, "bad sizes"),
             (dict(F=0), -1, "bad sizes"), (dict(H=3), -1, "bad sizes"), (dict(fast_threshold=-1), -1, "fast_threshold"),
             (dict(rgb=None), -1, "null pointer"), (dict(quota=None), -1, "null pointer"), (dict(count=None), -1, "null pointer"),
             (dict(quota=_p(negative)), -1, "quota"), (dict(quota=_p(none)), -1, "quota"),
             (dict(workspace=None), -3, "workspace"), (dict(workspace=_p(short), workspace_bytes=short.nbytes), -3, "workspace")]
    for kw, code, text in cases:
        out = fresh(3, sum(quota))
        assert call(lib, rgb, 3, 20, 4, quota, out, **kw) == code, kw
        assert text in lib.ffb6d_last_error().decode(), (kw, lib.ffb6d_last_error())
        for k, v in out.items():
            assert (v == FILL).all(), (kw, k)
    assert not short.any()
    # the workspace of exactly the stated size is enough
    out = fresh(3, sum(quota))
    exact = np.zeros(need, np.uint8)
    assert call(lib, rgb, 3, 20, 4, quota, out, ws=exact) == 0, lib.ffb6d_last_error()
    assert_same(out, orb_ref.detect(rgb, 3, 20, 4, quota), "exact workspace")
    kps, count, depth, visible, T, K = orb_ref.lift_case()
    F, Q = kps.shape[:2]
    slot_pts, slot_ok = np.full((F, Q, 3), FILL, np.float32), np.full((F, Q), FILL, np.int32)
    for kw in (dict(F=0), dict(Q=0), dict(fx=0.0), dict(kps=None), dict(slot_ok=None)):
        a = dict(kps=_p(kps), count=_p(count), depth=_p(depth), visible=_p(visible), T=_p(T), F=F, Q=Q, H=24, W=32, fx=K[0, 0], fy=K[1, 1],
                 cx=K[0, 2], cy=K[1, 2], min_pixels=50, slot_pts=_p(slot_pts), slot_ok=_p(slot_ok))
        a.update(kw)
        assert lib.ffb6d_orb_lift_f32(*a.values(), None) == -1, kw
        assert (slot_pts == FILL).all() and (slot_ok == FILL).all(), kw
    pts, begin, n_found = np.full((F * Q, 3), FILL, np.float32), np.full(3, FILL, np.int64), np.full(2, FILL, np.int32)
    for kw in (dict(S=0), dict(V=0), dict(Q=0), dict(pts=None), dict(begin=None)):
        a = dict(slot_pts=_p(slot_pts), slot_ok=_p(slot_ok), S=2, V=2, Q=Q, pts=_p(pts), begin=_p(begin), n_found=_p(n_found))
        a.update(kw)
        assert lib.ffb6d_orb_compact_f32(*a.values(), None) == -1, kw
        assert (pts == FILL).all() and (begin == FILL).all() and (n_found == FILL).all(), kw
