"""ColorJitter on the device (ffb6d_amd.train_data.color_jitter over csrc/color_jitter.hip), held to PILLOW's bytes: every golden
case of tests/golden/color_jitter.npz bit for bit (the cases of one image go as one batch; the 64 x 64 image also from device
pointers that are 4 bytes and 1 byte off the allocator's alignment, so each access width runs on the hardware), the image of all
2^24 colours against the recorded SHA-256 digests of Pillow's output, mixed batches at 37 x 53 and 480 x 640 against the numpy
restatement (tests/color_jitter_ref.py, itself held to Pillow by tests/test_color_jitter_cpu.py), and the builder's new argument."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import color_jitter_ref as ref
from ffb6d_amd import _lib, inputs, synth, train_data

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_jitter.npz")
MIXED = [None,
         dict(order=(3, 0, 2, 1), brightness=1.15, saturation=0.85, hue=-0.05),                    # no contrast
         dict(order=(1, 0, 2, 3), brightness=0.9, contrast=1.2, saturation=1.1, hue=0.03),          # contrast first
         dict(order=(0, 3, 1, 2), brightness=1.2, contrast=0.8, saturation=0.9, hue=0.05),          # ... third
         dict(order=(2, 3, 0, 1), brightness=0.8, contrast=1.1, saturation=1.2, hue=-0.02)]         # ... last


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    imgs = [z[f"img_{i}"] for i in range(len(meta["images"]))]
    by_image = {}
    for k, c in enumerate(meta["cases"]):
        by_image.setdefault(c["img"], []).append((c["params"], z[f"out_{k}"]))
    return dict(meta=meta, images=imgs, by_image=by_image)


def at_offset(a, offset, device):
    """`a` on the device, `offset` bytes behind the start of an allocation"""
    buf = torch.empty(a.size + 64, dtype=torch.uint8, device=device)
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 64 == offset
    return view


def first_differences(src, got, want, n=5):
    """up to n (input colour, got, want) triples where two [3,...] images differ"""
    d = (got != want).any(0)
    at = [(slice(None),) + tuple(i) for i in zip(*(ix[:n] for ix in np.nonzero(d)))]
    return int(d.sum()), [(src[i].tolist(), got[i].tolist(), want[i].tolist()) for i in at]


def test_golden_cases_are_pillows_bytes(device, golden):
    for i, cases in golden["by_image"].items():
        img = golden["images"][i]
        offsets = (0, 4, 1) if img.shape[1:] == (64, 64) else (0,)
        for offset in offsets:
            rgb = at_offset(np.stack([img] * len(cases)), offset, device)
            got = train_data.color_jitter(rgb, [p for p, _ in cases]).cpu().numpy()
            assert got.dtype == np.uint8 and got.shape == rgb.shape
            for b, (params, want) in enumerate(cases):
                assert np.array_equal(got[b], want), (golden["meta"]["images"][i], offset, params, first_differences(img, got[b], want))


@pytest.mark.parametrize("H,W", [(37, 53), (480, 640)])
def test_a_mixed_batch_equals_the_restatement(device, H, W):
    rgb = np.random.RandomState(H).randint(0, 256, (5, 3, H, W)).astype(np.uint8)
    x = torch.from_numpy(rgb).to(device)
    got = train_data.color_jitter(x, MIXED)
    again = train_data.color_jitter(x, MIXED)
    assert torch.equal(got, again)                                                     # two runs of one call: equal bytes
    assert torch.equal(x, torch.from_numpy(rgb).to(device))                            # the input is left alone
    got = got.cpu().numpy()
    want = ref.color_jitter_batch(rgb, MIXED)
    for b in range(5):
        assert np.array_equal(got[b], want[b]), (b, MIXED[b], first_differences(rgb[b], got[b], want[b]))


def test_the_colour_cube_has_pillows_digests(device, golden):
    cube = ref.colour_cube()
    x = torch.from_numpy(cube[None]).to(device)
    assert len(golden["meta"]["cube"]) == 4
    for c in golden["meta"]["cube"]:
        got = train_data.color_jitter(x, [c["params"]])[0].cpu().numpy()
        if hashlib.sha256(got.tobytes()).hexdigest() != c["sha256"]:
            want = ref.color_jitter(cube, c["params"])                                  # only to say where: the digest is the check
            pytest.fail(f"{c['params']}: digest differs from Pillow's; against the restatement: {first_differences(cube, got, want)}")


def test_bad_parameters_and_cpu_tensors_are_refused(device):
    x = torch.zeros((1, 3, 4, 4), dtype=torch.uint8, device=device)
    for bad in (dict(order=(0, 0), brightness=1.0), dict(order=(1,), contrast=-0.1), dict(order=(2,), saturation=float("nan")),
                dict(order=(0,), brightness=float("inf")), dict(order=(3,), hue=0.6)):
        with pytest.raises((ValueError, _lib.FFB6DNativeError)):
            train_data.color_jitter(x, [bad])
    with pytest.raises(ValueError):
        train_data.color_jitter(x, [None, None])
    if device.type == "cuda":
        with pytest.raises(_lib.FFB6DNativeError):
            train_data.color_jitter(x.cpu(), [None])
    assert train_data.color_jitter(x[:0], []).shape == (0, 3, 4, 4)


def test_the_builder_jitters_first_and_none_leaves_it_as_it_was(device):
    B, H, W = 2, 120, 160
    fr = synth.make_batch(31, B, n_points=1024, height=H, width=W)
    rgb = torch.from_numpy(fr["rgb"]).to(device)
    depth = torch.from_numpy(np.ascontiguousarray(fr["dpt_xyz"][:, 2])).to(device)
    nrm = torch.from_numpy(np.random.RandomState(2).standard_normal((B, 3, H, W)).astype(np.float32)).to(device)
    lab = torch.from_numpy(np.random.RandomState(3).randint(0, 4, (B, H, W)).astype(np.uint8)).to(device)
    case = synth.make_pose_case(5, n_obj=3, n_kps=8)
    args = (depth, lab, synth.LINEMOD_K, 1024, np.tile([1, 2, 3], (B, 1)), np.stack([case["RT"][1:]] * B), case["mesh_kps"],
            case["mesh_ctr"])
    plain = train_data.assemble_training_batch(rgb, *args, normals=nrm, seed=17, jitter_params=None)
    today = inputs.assemble_inputs(rgb, depth, nrm, synth.LINEMOD_K, 1024, seed=17)
    for k, v in today.items():
        assert torch.equal(plain[k], v), k
    g = torch.Generator().manual_seed(9)
    params = [train_data.draw_jitter_params(g), None]
    jittered = train_data.color_jitter(rgb, params)
    assert not torch.equal(jittered[0], rgb[0]) and torch.equal(jittered[1], rgb[1])
    got = train_data.assemble_training_batch(rgb, *args, normals=nrm, seed=17, jitter_params=params)
    want = train_data.assemble_training_batch(jittered, *args, normals=nrm, seed=17)
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(got[k], v) if torch.is_tensor(v) else got[k] == v, k
    assert not torch.equal(got["rgb"], plain["rgb"])
    # synthetic frames too: the jitter comes before the synthetic-frame branch
    syn = dict(synthetic=[True, False], noise_params=[dict(hsv=(1.3, 1.2)), None], aug_seed=4)
    got = train_data.assemble_training_batch(rgb, *args, normals=nrm, seed=17, jitter_params=params, **syn)
    want = train_data.assemble_training_batch(jittered, *args, normals=nrm, seed=17, **syn)
    assert torch.equal(got["rgb"], want["rgb"])
