"""ColorJitter without a GPU: the numpy restatement of the rule (tests/color_jitter_ref.py) equals the committed goldens, which are
PILLOW's outputs (tests/golden/color_jitter.npz, written by tests/golden/make_golden_jitter.py), byte for byte; where PIL imports,
it also equals the live library on all 2^24 colours for each single operation and on a few hundred random chains, and the recorded
colour-cube digests are those of the live library.  The host side of ffb6d_amd.train_data: draws, records, symbols."""
import ctypes
import hashlib
import itertools
import json
import os

import numpy as np
import pytest
import torch

import color_jitter_ref as ref
from ffb6d_amd import _lib, train_data

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_jitter.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    imgs = [z[f"img_{i}"] for i in range(len(meta["images"]))]
    cases = [(imgs[c["img"]], c["params"], z[f"out_{k}"], c["what"]) for k, c in enumerate(meta["cases"])]
    return dict(meta=meta, images=dict(zip(meta["images"], imgs)), cases=cases)


@pytest.fixture(scope="module")
def cube():
    c = ref.colour_cube()
    c.setflags(write=False)
    return c


def test_the_goldens_hold_the_cases_they_are_meant_to_hold(golden):
    cases = golden["cases"]
    full = [tuple(p["order"]) for _, p, _, _ in cases if p and len(ref.chain(p)) == 4]
    assert set(full) == set(itertools.permutations(range(4)))                           # every order; contrast in every position
    assert {len(ref.chain(p)) for _, p, _, _ in cases} == {0, 1, 2, 3, 4}
    assert any(p is None for _, p, _, _ in cases)
    for key in ("brightness", "contrast", "saturation"):
        vals = [p[key] for _, p, _, _ in cases if p and p.get(key) is not None]
        assert 0.0 in vals and 1.0 in vals and any(0 < v < 1 for v in vals) and any(v > 1 for v in vals), key
    assert {-0.05, 0.05, -0.5, 0.5} <= {p["hue"] for _, p, _, _ in cases if p and p.get("hue") is not None}
    assert {im.shape[1:] for im in golden["images"].values()} >= {(1, 1), (1, 2), (3, 5), (37, 53), (64, 64)}
    const, white, half = (golden["images"][k] for k in ("constant", "white", "half"))
    assert (const == const[:, :1, :1]).all() and white.min() >= 236
    assert ref.luminance(half).tolist() == [[10, 11]] and ref.contrast_mean(half) == 11  # mean 10.5 rounds up
    assert [c["params"] for c in golden["meta"]["cube"]] == [dict(order=[3], hue=-0.05), dict(order=[3], hue=0.05),
                                                            dict(order=[2], saturation=0.8), dict(order=[2], saturation=1.2)]
    assert ref.hue_shift(-0.05) == 244 and ref.hue_shift(0.05) == 12 and ref.hue_shift(0.5) == 127 and ref.hue_shift(-0.5) == 129
    assert os.path.getsize(GOLDEN) < 64 * 1024


def test_the_restatement_equals_the_goldens_byte_for_byte(golden):
    for img, params, want, what in golden["cases"]:
        got = ref.color_jitter(img, params)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (what, params, img.shape)


def test_the_restatement_equals_live_pillow_on_the_whole_colour_cube(cube, golden):
    pytest.importorskip("PIL")
    recorded = {json.dumps(c["params"]): c["sha256"] for c in golden["meta"]["cube"]}
    singles = [dict(order=[3], hue=-0.05), dict(order=[3], hue=0.05), dict(order=[2], saturation=0.8), dict(order=[2], saturation=1.2),
               dict(order=[0], brightness=1.2), dict(order=[1], contrast=0.8)]
    for params in singles:
        want = ref.pil_color_jitter(cube, params)
        got = ref.color_jitter(cube, params)
        diff = (got != want).any(0)
        assert not diff.any(), (params, int(diff.sum()), cube[:, diff][:, :4].T.tolist())
        if json.dumps(params) in recorded:
            assert hashlib.sha256(want.tobytes()).hexdigest() == recorded[json.dumps(params)], params


def test_the_restatement_equals_live_pillow_on_random_chains():
    pytest.importorskip("PIL")
    rng = np.random.RandomState(0)
    for k in range(300):
        img = rng.randint(0, 256, (3, rng.randint(1, 9), rng.randint(1, 9))).astype(np.uint8)
        if k % 4 == 1:
            img[:] = img[:, :1, :1]                                                      # constant
        elif k % 4 == 2:
            img = (img // 64 * 85).astype(np.uint8)                                      # coarsely quantised
        elif k % 4 == 3:
            img = np.maximum(img, 230).astype(np.uint8)                                  # near white
        p = dict(order=rng.permutation(4).tolist())
        for key, lo, hi in (("brightness", 0, 2.5), ("contrast", 0, 2.5), ("saturation", 0, 2.5), ("hue", -0.5, 0.5)):
            if rng.rand() < 0.8:
                p[key] = float(rng.uniform(lo, hi))
        assert np.array_equal(ref.color_jitter(img, p), ref.pil_color_jitter(img, p)), (k, p, img.tolist())


def test_draw_jitter_params_stays_in_its_ranges_and_follows_the_seed():
    g = torch.Generator().manual_seed(5)
    draws = [train_data.draw_jitter_params(g) for _ in range(200)]
    for p in draws:
        assert sorted(p["order"]) == [0, 1, 2, 3]
        assert all(0.8 <= p[k] <= 1.2 for k in ("brightness", "contrast", "saturation")) and -0.05 <= p["hue"] <= 0.05
    assert len({p["order"] for p in draws}) > 12 and len({p["hue"] for p in draws}) == 200
    assert np.mean([p["brightness"] for p in draws]) == pytest.approx(1.0, abs=0.03)     # sigma of the mean: 0.115 / sqrt(200) = 0.008
    again = torch.Generator().manual_seed(5)
    assert [train_data.draw_jitter_params(again) for _ in range(200)] == draws
    assert train_data.draw_jitter_params(torch.Generator().manual_seed(6)) != draws[0]
    p = train_data.draw_jitter_params(torch.Generator().manual_seed(7), brightness=1.5, contrast=0, saturation=None, hue=0.5)
    assert set(p) == {"order", "brightness", "hue"} and 0.0 <= p["brightness"] <= 2.5 and -0.5 <= p["hue"] <= 0.5
    with pytest.raises(ValueError):
        train_data.draw_jitter_params(g, hue=0.6)


def test_records_follow_the_order_and_skip_missing_operations():
    rec = train_data.jitter_records([None, dict(order=(3, 1, 0, 2), contrast=1.25, hue=-0.05, saturation=None),
                                     dict(brightness=0.5, contrast=0.75, saturation=1.5, hue=0.5)])
    assert train_data.JITTER_FRAME.itemsize == 40 and rec.dtype == train_data.JITTER_FRAME
    assert rec[0]["n_ops"] == 0
    assert rec[1]["n_ops"] == 2 and rec[1]["op"][:2].tolist() == [3, 1] and rec[1]["alpha"][1] == np.float32(1.25) and rec[1]["hue_shift"] == 244
    assert rec[2]["n_ops"] == 4 and rec[2]["op"].tolist() == [0, 1, 2, 3] and rec[2]["alpha"][:3].tolist() == [0.5, 0.75, 1.5]
    assert rec[2]["hue_shift"] == 127
    for bad in (dict(order=(4,), hue=0.1), dict(order=(3,), hue=0.51), dict(order=(0, 1, 2, 3, 0), brightness=1.0)):
        with pytest.raises(ValueError):
            train_data.jitter_records([bad])


def test_the_c_symbols_exist_with_their_signatures_and_refuse_bad_records():
    lib = _lib.load()
    vp, i32, i64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    want = {"ffb6d_jitter_frames_check": (i32, [vp, i32]), "ffb6d_color_jitter_workspace_bytes": (sz, [i32, i64, i64]),
            "ffb6d_color_jitter_u8": (i32, [vp, vp, vp, i32, i64, i64, vp, sz, vp])}
    for name, (res, args) in want.items():
        assert _lib.SIGNATURES[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    assert lib.ffb6d_color_jitter_workspace_bytes(8, 480, 640) == (8 * 75 * 8 + 255) // 256 * 256
    assert lib.ffb6d_color_jitter_workspace_bytes(0, 480, 640) == 0
    rec = train_data.jitter_records([dict(order=(0, 1, 2, 3), brightness=1.1, contrast=0.9, saturation=1.0, hue=0.02)] * 2)
    assert lib.ffb6d_jitter_frames_check(rec.ctypes.data, 2) == 0
    for field, value in (("op", [1, 1, 2, 3]), ("op", [0, 1, 2, 7]), ("alpha", [1.0, -1.0, 1.0, 0.0]), ("alpha", [np.inf, 1, 1, 0]),
                         ("alpha", [1, 1, np.nan, 0]), ("n_ops", 5)):
        bad = rec.copy()
        bad[1][field] = value
        assert lib.ffb6d_jitter_frames_check(bad.ctypes.data, 2) == -1, (field, value)
        assert b"frame 1" in lib.ffb6d_last_error()
    # the wrapper refuses them before anything reaches a device, and refuses CPU tensors like the rest of the module
    with pytest.raises(_lib.FFB6DNativeError):
        train_data.color_jitter(torch.zeros((1, 3, 4, 4), dtype=torch.uint8), [None])
