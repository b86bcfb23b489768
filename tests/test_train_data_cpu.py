"""Training samples without a GPU (ffb6d_amd/train_data.py, csrc/train_data.hip): the host parameter draws against the draw
log of the reference's own rgb_add_noise (tests/golden/train_small.json, make_golden_train.py), the motion-blur tap lists, and
the four kernels run through the SIMT emulator (tests/simt) on tiny inputs against the reference's own get_pose_gt_info
(tests/golden/train_small.npz) and the restatements of tests/train_data_ref.py."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from ffb6d_amd import train_data
from tests.simt.build import load, ptr as _p
from train_data_ref import filter_ref, hsv_jitter_ref, pose_targets_ref

spec = importlib.util.spec_from_file_location("make_golden_train", os.path.join(GOLDEN, "make_golden_train.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def draw_logs():
    with open(os.path.join(GOLDEN, "train_small.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "train_small.npz"))


# ---- host draws -------------------------------------------------------------------------------------------------
def _draws(log):
    out = []
    for e in log:
        if e[0] == "randn":
            break
        if e[0] in ("rand", "randint"):
            out.append(e)
    return out


@pytest.mark.parametrize("flavour", ["ycb", "linemod"])
def test_host_draws_equal_the_reference_draw_log(draw_logs, flavour):
    stages = set()
    for seed, log in draw_logs[flavour].items():
        mine = []
        p = train_data.draw_noise_params(gen.LoggingRandomState(int(seed), mine), flavour)
        want = _draws(log)
        got = [e for e in mine if e[0] in ("rand", "randint")]
        assert got[:len(want)] == want, (seed, got, want)
        if flavour == "ycb":
            assert any(e[0] == "randn" for e in log) and p["noise_sigma"] == want[-1][2]
            assert len(got) == len(want) + 1                              # + the extra-noise decision
        else:
            assert got == want and p["noise_sigma"] == 0 and not p["extra_noise"]
        cv = [e for e in log if e[0] in ("filter2D", "GaussianBlur", "line")]
        if p["sharpen"] is not None:
            stages.add("sharpen")
            k = np.array(cv.pop(0)[1])
            dy, dx, w = train_data.sharpen_taps(p["sharpen"])
            assert np.array_equal(k[dy + 1, dx + 1], w) and len(w) == 9
        if p["motion"] is not None:
            stages.add("motion")
            angle, length = p["motion"]
            rad = np.deg2rad(angle)
            a = int(max(abs(np.cos(rad)), abs(np.sin(rad))) * length * 2)
            if a > 0:
                line = cv.pop(0)
                assert line[0] == "line" and line[1] == [a, a] and line[2] == [a // 2, a // 2]
                assert line[3] == [int(np.cos(rad) * length + a // 2), int(np.sin(rad) * length + a // 2)]
                assert cv.pop(0)[0] == "filter2D"
        if p["gauss"] is not None:
            stages.add("gauss")
            e = cv.pop(0)
            assert e[0] == "GaussianBlur" and e[1] == [p["gauss"][0]] * 2 and e[2] == p["gauss"][1]
        assert not cv
        if p["hsv"] is not None:
            stages.add("hsv")
    assert stages >= {"hsv", "motion", "gauss"}


# ---- motion blur taps -------------------------------------------------------------------------------------------
def _set(taps):
    return sorted((int(a), int(b)) for a, b in zip(taps[0], taps[1]))


def test_motion_blur_taps_exact_sets():
    L = 3
    assert _set(train_data.motion_blur_taps(0, L)) == [(0, dx) for dx in range(L)]           # end point clipped at x = a
    assert _set(train_data.motion_blur_taps(90, L)) == [(dy, 0) for dy in range(L)]
    assert _set(train_data.motion_blur_taps(180, L)) == [(0, dx) for dx in range(-L, 1)]
    # cos(270 deg) * 3 + 3 truncates to 2: the line runs from the anchor to (2, 0), 8-connected
    assert _set(train_data.motion_blur_taps(270, L)) == [(-3, -1), (-2, -1), (-1, 0), (0, 0)]
    assert _set(train_data.motion_blur_taps(45, L)) == [(0, 0), (1, 1)]                       # (4, 4) clipped to (3, 3)
    for a in (0, 90, 180, 270, 45):
        w = train_data.motion_blur_taps(a, L)[2]
        assert np.all(w == 1.0 / len(w))


def test_motion_blur_taps_whole_range():
    for angle in range(360):
        for length in range(1, 16):
            dy, dx, w = train_data.motion_blur_taps(angle, length)
            rad = np.deg2rad(angle)
            a = int(max(abs(np.cos(rad)), abs(np.sin(rad))) * length * 2)
            assert 1 <= len(w) <= train_data.MAX_TAPS
            assert abs(w.sum() - 1.0) < 1e-12
            assert np.all((dy + a // 2 >= 0) & (dy + a // 2 < a) & (dx + a // 2 >= 0) & (dx + a // 2 < a))
            assert (0, 0) in _set((dy, dx))                                                     # starts at the anchor
            pts = set(_set((dy, dx)))
            if len(pts) > 1:                                                                    # 8-connected
                for y, x in pts:
                    assert any((y + u, x + v) in pts for u in (-1, 0, 1) for v in (-1, 0, 1) if u or v), (angle, length)


def test_motion_blur_taps_identity_when_the_kernel_is_empty():
    for angle, length in ((0, 0), (45, 0), (30, 0.2)):
        dy, dx, w = train_data.motion_blur_taps(angle, length)
        assert list(dy) == [0] and list(dx) == [0] and list(w) == [1.0]


# ---- the kernels on the SIMT emulator ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu_train():
    """the emulated library (tests/simt/build.py)"""
    return load()


def emu_pose_targets(lib, cld, choose, label_img, cls_ids, RTs, kps, ctr):
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


def golden_inputs(flavour, i, n_objects):
    """The case of make_golden_train as the C ABI takes it: the points' labels as a 16 x 16 label image with choose = 0..255."""
    c = gen.pose_case(flavour, i)
    ids = np.zeros((1, n_objects), np.int32)
    ids[0, :len(c["cls_ids"])] = c["cls_ids"]
    RT = np.zeros((1, n_objects, 3, 4))
    RT[0, :len(c["cls_ids"])] = c["RT"]
    return c, dict(cld=c["cld"][None], choose=np.arange(gen.N_POINTS, dtype=np.int64)[None],
                   label_img=c["labels"].reshape(1, 16, 16), cls_ids=ids, RTs=RT, kps=c["mesh_kps"], ctr=c["mesh_ctr"])


def ulp_close(got, want):
    want32 = want.astype(np.float32)
    return np.all(np.abs(got.astype(np.float64) - want32.astype(np.float64)) <= np.spacing(np.abs(want32)).astype(np.float64))


def test_pose_targets_on_the_emulator_match_the_reference(emu_train, golden):
    for flavour, tag, n, n_obj in (("ycb", "ycb", 3, 22), ("linemod", "lm", 2, 2)):
        for i in range(n):
            c, a = golden_inputs(flavour, i, n_obj)
            rc, out = emu_pose_targets(emu_train, **a)
            assert rc == 0, emu_train.ffb6d_last_error()
            g = {k: golden[f"{tag}{i}/{k}"] for k in ("RTs", "kp_3ds", "ctr_3ds", "cls_ids", "kp_targ_ofst", "ctr_targ_ofst")}
            assert np.array_equal(out["labels"][0], c["labels"].astype(np.int32))
            assert np.array_equal(out["cls_ids"][0], g["cls_ids"].astype(np.int32))
            assert np.array_equal(out["RTs"][0], g["RTs"].astype(np.float32))
            for k in ("kp_3ds", "ctr_3ds", "kp_targ_ofst", "ctr_targ_ofst"):
                assert ulp_close(out[k][0], g[k]), (flavour, i, k)
            empty = g["cls_ids"][:, 0] == 0
            assert not out["kp_3ds"][0][empty].any() and not out["RTs"][0][empty].any()


def test_pose_targets_on_the_emulator_treat_bad_device_ids_as_empty(emu_train):
    c, a = golden_inputs("ycb", 1, 4)
    a["cls_ids"][0, 2:] = [99, -4]                                          # never an index
    rc, out = emu_pose_targets(emu_train, **a)
    assert rc == 0
    assert list(out["cls_ids"][0, :, 0]) == [5, 9, 0, 0] and not out["RTs"][0, 2:].any()
    want = pose_targets_ref(c["cld"], c["labels"], [5, 9], c["RT"], c["mesh_kps"], c["mesh_ctr"])
    assert ulp_close(out["kp_targ_ofst"][0], want["kp_targ_ofst"])
    a["cls_ids"] = np.zeros((1, 65), np.int32)
    a["RTs"] = np.zeros((1, 65, 3, 4))
    rc, out = emu_pose_targets(emu_train, **a)
    assert rc != 0 and "O = 65" in emu_train.ffb6d_last_error().decode()
    assert np.all(out["labels"] == 0) and np.all(out["kp_3ds"] == 7)        # nothing written


def test_hsv_on_the_emulator_matches_the_restatement(emu_train):
    rng = np.random.RandomState(5)
    H, W = 9, 13                                                            # H*W odd: the scalar path
    for (fs, fv), shape in (((1.3, 1.2), (2, 3, 16, 16)), ((0.8, 1.1), (2, 3, H, W))):
        img = rng.randint(0, 256, shape).astype(np.uint8)
        img[0, :, 0, :4] = [[0, 50, 255, 7]] * 3                            # greys
        fsfv = np.array([[fs, fv], [-1.0, 0.0]])
        out = np.zeros_like(img)
        assert emu_train.ffb6d_rgb_hsv_jitter(_p(img), _p(fsfv), _p(out), shape[0], shape[2], shape[3], None) == 0
        want = hsv_jitter_ref(img[0, 0], img[0, 1], img[0, 2], fs, fv)
        for c in range(3):
            assert np.array_equal(out[0, c], want[c]), (fs, fv, c)
        assert np.array_equal(out[1], img[1])                               # frame without the stage
        assert np.all(out[0, 0, 0, :4] == out[0, 1, 0, :4]) and np.all(out[0, 1, 0, :4] == out[0, 2, 0, :4])


def _frames(taps_per_frame, sigma=0.0, extra=0.0):
    fr = np.zeros(len(taps_per_frame), train_data.STENCIL_FRAME)
    for b, taps in enumerate(taps_per_frame):
        train_data._fill_frame(fr[b], taps)
        fr[b]["sigma"], fr[b]["extra_sigma"] = sigma, extra
    return fr


def test_stencil_on_the_emulator_within_one_level(emu_train):
    rng = np.random.RandomState(6)
    for H, W in ((20, 72), (7, 9)):                                         # two tiles with borders; the scalar path
        taps = [train_data.sharpen_taps(10.3), train_data.motion_blur_taps(200, 9), train_data.gaussian_taps(5, 0.7), None]
        img = rng.randint(0, 256, (len(taps), 3, H, W)).astype(np.uint8)
        fr = _frames(taps)
        out = np.zeros_like(img)
        assert emu_train.ffb6d_rgb_stencil(_p(img), _p(fr), 1, _p(out), len(taps), H, W, None) == 0
        for b, t in enumerate(taps):
            if t is None:
                assert np.array_equal(out[b], img[b])
                continue
            want = np.clip(np.rint(filter_ref(img[b], t)), 0, 255)
            assert np.abs(out[b].astype(np.int64) - want).max() <= 1, (H, W, b)


def test_noise_on_the_emulator_is_keyed_and_truncates(emu_train):
    img = np.full((2, 3, 8, 8), 128, np.uint8)
    fr = _frames([None, None], sigma=10.0)
    a, b = np.zeros_like(img), np.zeros_like(img)
    emu_train.ffb6d_rgb_stencil(_p(img), _p(fr), 11, _p(a), 2, 8, 8, None)
    emu_train.ffb6d_rgb_stencil(_p(img), _p(fr), 11, _p(b), 2, 8, 8, None)
    assert np.array_equal(a, b) and not np.array_equal(a[0], a[1])
    emu_train.ffb6d_rgb_stencil(_p(img), _p(fr), 12, _p(b), 2, 8, 8, None)
    assert not np.array_equal(a, b)
    fr0 = _frames([None, None])
    emu_train.ffb6d_rgb_stencil(_p(img), _p(fr0), 11, _p(b), 2, 8, 8, None)
    assert np.array_equal(b, img)


def test_add_real_back_on_the_emulator(emu_train):
    rng = np.random.RandomState(8)
    B, H, W = 3, 5, 7
    rgb = rng.randint(0, 256, (B, 3, H, W)).astype(np.uint8)
    back = rng.randint(0, 256, (B, 3, H, W)).astype(np.uint8)
    lab = rng.randint(0, 3, (B, H, W)).astype(np.uint8)
    dep = np.where(rng.rand(B, H, W) < 0.3, 0, rng.rand(B, H, W)).astype(np.float32)
    bdep = rng.rand(B, H, W).astype(np.float32)
    for flavour, bmask in ((0, rng.randint(0, 3, (B, H, W)).astype(np.int32)), (1, rng.choice([0, 255], (B, H, W)).astype(np.uint8))):
        flags = np.array([1, 0, 1], np.uint8)
        o_rgb, o_dep = np.zeros_like(rgb), np.zeros_like(dep)
        rc = emu_train.ffb6d_add_real_back(_p(rgb), _p(lab), 1, _p(dep), _p(back), _p(bdep), _p(bmask), int(bmask.dtype == np.uint8),
                                           flavour, _p(flags), _p(o_rgb), _p(o_dep), B, H * W, None)
        assert rc == 0
        keep = (bmask <= 0) if flavour == 0 else (bmask < 255)
        want_rgb = np.where((lab <= 0)[:, None] & (flags[:, None, None, None] > 0), back * keep[:, None], rgb)
        assert np.array_equal(o_rgb, want_rgb)
        assert np.array_equal(o_dep, np.where(dep > 1e-6, dep, bdep * keep.astype(np.float32)))
