"""Training samples on the MI355X (ffb6d_amd/train_data.py over csrc/train_data.hip): pose targets against the reference's
own get_pose_gt_info (tests/golden/train_small.npz) and through the pose solver end to end, robustness of the targets
kernel, the HSV round trip on all 2^24 colours, the filters, the noise statistics, compositing, and the whole builder."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from ffb6d_amd import _lib, evaluate, inputs, loss, model, pose, synth, train_data
from train_data_ref import filter_ref, hsv_jitter_ref
from test_train_data_cpu import golden_inputs, ulp_close

pytestmark = pytest.mark.gpu

spec = importlib.util.spec_from_file_location("make_golden_train", os.path.join(GOLDEN, "make_golden_train.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "train_small.npz"))


def _dev(a, device):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).to(device) if k in ("cld", "choose", "label_img") else v)
            for k, v in a.items()}


def _targets(a):
    return train_data.pose_targets(a["cld"], a["choose"], a["label_img"], a["cls_ids"], a["RTs"], a["kps"], a["ctr"])


# ---- pose targets -----------------------------------------------------------------------------------------------
def test_pose_targets_match_the_reference(device, golden):
    for flavour, tag, n, n_obj in (("ycb", "ycb", 3, 22), ("linemod", "lm", 2, 2)):
        for i in range(n):
            c, a = golden_inputs(flavour, i, n_obj)
            out = {k: v.cpu().numpy() for k, v in _targets(_dev(a, device)).items()}
            g = {k: golden[f"{tag}{i}/{k}"] for k in ("RTs", "kp_3ds", "ctr_3ds", "cls_ids", "kp_targ_ofst", "ctr_targ_ofst")}
            assert np.array_equal(out["labels"][0], c["labels"].astype(np.int32))
            assert np.array_equal(out["cls_ids"][0], g["cls_ids"].astype(np.int32))
            assert np.array_equal(out["RTs"][0], g["RTs"].astype(np.float32))
            for k in ("kp_3ds", "ctr_3ds", "kp_targ_ofst", "ctr_targ_ofst"):
                assert ulp_close(out[k][0], g[k]), (flavour, i, k)


def test_targets_round_trip_through_the_solver(device):
    B, n_obj, n_kps = 2, 2, 8
    cases = [synth.make_pose_case(40 + b, n_pts=2048, n_obj=n_obj, n_kps=n_kps, noise=0.0, outliers=0.0, label_noise=0.0,
                                  mesh_seed=77) for b in range(B)]
    cld = torch.from_numpy(np.stack([c["pcld"] for c in cases])).to(device)
    labels = np.stack([c["mask"] for c in cases]).astype(np.int32)                  # point i sits on pixel i
    lab_img = torch.from_numpy(labels.reshape(B, 32, 64)).to(device)
    choose = torch.arange(2048, device=device).repeat(B, 1)
    ids = np.tile(np.arange(1, n_obj + 1), (B, 1))
    RTs = np.stack([c["RT"][1:] for c in cases])
    tg = train_data.pose_targets(cld, choose, lab_img, ids, RTs, cases[0]["mesh_kps"], cases[0]["mesh_ctr"])
    res = pose.solve_poses(cld, tg["labels"].long(), tg["ctr_targ_ofst"][:, None], tg["kp_targ_ofst"].permute(0, 2, 1, 3).contiguous(),
                           cases[0]["mesh_kps"], cases[0]["mesh_ctr"], r_lst=cases[0]["r_lst"])
    models = evaluate.ModelPoints({c: synth.model_cloud(900 + c, 500) for c in range(1, n_obj + 1)}, device=device)
    for b, (cls, poses, _) in enumerate(res):
        assert sorted(int(c) for c in cls) == [1, 2]
        for c, P in zip(cls, poses):
            gt = cases[b]["RT"][int(c)]
            assert np.abs(P[:, 3] - gt[:, 3]).max() < 1e-5
            cosang = (np.trace(P[:, :3].T @ gt[:, :3]) - 1) / 2
            assert np.arccos(np.clip(cosang, -1, 1)) < 1e-4
            add, adds = evaluate.add_adds(P[None], gt[None], [int(c)], models)
            assert float(add) < 1e-5 and float(adds) < 1e-5


def test_pose_targets_robustness(device):
    rng = np.random.RandomState(3)
    B, N, O, H, W = 3, 700, 5, 20, 40
    for K in (1, 8, 16):
        kps = rng.rand(6, K, 3).astype(np.float32) - 0.5
        ctr = rng.rand(6, 3).astype(np.float32) - 0.5
        cld = torch.from_numpy(rng.rand(B, N, 3).astype(np.float32)).to(device)
        choose = torch.from_numpy(rng.randint(0, H * W, (B, N))).to(device)
        lab = torch.from_numpy(rng.randint(0, 7, (B, H, W)).astype(np.uint8)).to(device)
        ids = rng.randint(0, 6, (B, O))
        RTs = rng.rand(B, O, 3, 4)
        ref = train_data.pose_targets(cld, choose, lab, ids, RTs, kps, ctr)
        for b in range(B):                                                  # batch independence
            one = train_data.pose_targets(cld[b:b + 1], choose[b:b + 1], lab[b:b + 1], ids[b:b + 1], RTs[b:b + 1], kps, ctr)
            for k in one:
                assert torch.equal(one[k][0], ref[k][b]), (K, k)
        variants = [dict(choose=choose.int()), dict(lab=lab.int()), dict(RTs=RTs.astype(np.float32).astype(np.float64)),
                    dict(cld=cld.transpose(0, 1).contiguous().transpose(0, 1)), dict(ids=torch.from_numpy(ids).to(device))]
        for v in variants:
            a = dict(cld=cld, choose=choose, lab=lab, ids=ids, RTs=RTs)
            a.update(v)
            got = train_data.pose_targets(a["cld"], a["choose"], a["lab"], a["ids"], a["RTs"], kps, ctr)
            want = ref if "RTs" not in v else train_data.pose_targets(cld, choose, lab, ids, RTs.astype(np.float32), kps, ctr)
            for k in got:
                assert torch.equal(got[k], want[k]), (K, list(v), k)
    with pytest.raises(ValueError, match="outside"):
        train_data.pose_targets(cld, choose, lab, np.full((B, O), 6), RTs, kps, ctr)
    with pytest.raises(ValueError, match="outside"):
        train_data.pose_targets(cld, choose, lab, np.full((B, O), -1), RTs, kps, ctr)
    with pytest.raises(TypeError):
        train_data.pose_targets(cld.double(), choose, lab, ids, RTs, kps, ctr)
    with pytest.raises(TypeError):
        train_data.pose_targets(cld, choose.float(), lab, ids, RTs, kps, ctr)
    with pytest.raises(TypeError):
        train_data.pose_targets(cld, choose, lab.long(), ids, RTs, kps, ctr)
    with pytest.raises(_lib.FFB6DNativeError):
        train_data.pose_targets(cld.cpu(), choose, lab, ids, RTs, kps, ctr)


# ---- HSV ---------------------------------------------------------------------------------------------------------
def test_hsv_all_colours(device):
    v = np.arange(1 << 24, dtype=np.int64)
    planes = np.stack([v & 255, (v >> 8) & 255, v >> 16]).astype(np.uint8)          # plane 0 = "B"
    img = torch.from_numpy(planes.reshape(1, 3, 4096, 4096)).to(device)
    for fs, fv in ((1.3, 1.2), (0.8, 0.9), (1.45, 1.35)):
        out = train_data.rgb_add_noise(img, [dict(hsv=(fs, fv))], seed=0).cpu().numpy().reshape(3, -1)
        for s in range(0, 1 << 24, 1 << 22):
            want = hsv_jitter_ref(planes[0, s:s + (1 << 22)], planes[1, s:s + (1 << 22)], planes[2, s:s + (1 << 22)], fs, fv)
            for c in range(3):
                assert np.array_equal(out[c, s:s + (1 << 22)], want[c]), (fs, fv, c, s)
    grey = planes[0] == planes[1]
    grey &= planes[1] == planes[2]
    assert np.array_equal(out[0][grey], out[1][grey]) and np.array_equal(out[1][grey], out[2][grey])


# ---- filters -----------------------------------------------------------------------------------------------------
def _filter_cases():
    return [("sharpen", dict(sharpen=9.7), train_data.sharpen_taps(9.7)),
            ("motion", dict(motion=(33, 14)), train_data.motion_blur_taps(33, 14)),
            ("motion", dict(motion=(270, 15)), train_data.motion_blur_taps(270, 15)),
            ("gauss", dict(gauss=(3, 0.6)), train_data.gaussian_taps(3, 0.6)),
            ("gauss", dict(gauss=(5, 0.93)), train_data.gaussian_taps(5, 0.93))]


def test_filters_within_one_level(device):
    rng = np.random.RandomState(4)
    cases = _filter_cases()
    for H, W in ((96, 136), (37, 51)):
        img = rng.randint(0, 256, (len(cases) + 1, 3, H, W)).astype(np.uint8)
        out = train_data.rgb_add_noise(torch.from_numpy(img).to(device), [p for _, p, _ in cases] + [None], seed=1).cpu().numpy()
        for b, (_, _, taps) in enumerate(cases):
            want = np.clip(np.rint(filter_ref(img[b], taps)), 0, 255)
            assert np.abs(out[b].astype(np.int64) - want).max() <= 1, (H, W, b)
        assert np.array_equal(out[-1], img[-1])                             # a frame with no stages: unchanged
        const = np.full((len(cases), 3, H, W), 77, np.uint8)
        outc = train_data.rgb_add_noise(torch.from_numpy(const).to(device), [p for _, p, _ in cases], seed=1).cpu().numpy()
        assert np.all(outc == 77)


def test_filter_impulse_responses_equal_the_taps(device):
    H, W = 48, 64
    for _, p, (dy, dx, w) in _filter_cases():
        img = np.zeros((1, 3, H, W), np.uint8)
        img[0, :, 24, 32] = 200
        out = train_data.rgb_add_noise(torch.from_numpy(img).to(device), [p], seed=1).cpu().numpy()[0, 0].astype(np.float64)
        want = np.zeros((H, W))
        for a, b, v in zip(dy, dx, w):                                      # correlation: the tap at (dy, dx) lands at -(dy, dx)
            want[24 - a, 32 - b] += 200 * np.float32(v)
        assert np.abs(out - np.clip(np.rint(want), 0, 255)).max() <= 1


# ---- noise ---------------------------------------------------------------------------------------------------------
def test_noise_keys_identity_and_statistics(device):
    grey = torch.full((2, 3, 480, 640), 128, dtype=torch.uint8, device=device)
    p = [dict(noise_sigma=10), dict(noise_sigma=10)]
    a = train_data.rgb_add_noise(grey, p, seed=5)
    assert torch.equal(a, train_data.rgb_add_noise(grey, p, seed=5))
    assert not torch.equal(a, train_data.rgb_add_noise(grey, p, seed=6))
    assert not torch.equal(a[0], a[1])
    assert torch.equal(train_data.rgb_add_noise(grey, [dict(noise_sigma=0)] * 2, seed=5), grey)
    d = a.double().cpu().numpy() - 128.0
    # E and sd of trunc(clip(128 + 10 n)) - 128 by quadrature over n
    n = np.linspace(-9, 9, 2_000_001)
    pdf = np.exp(-0.5 * n * n) / np.sqrt(2 * np.pi)
    x = np.floor(np.clip(128 + 10 * n, 0, 255)) - 128
    dn = n[1] - n[0]
    mean = np.sum(x * pdf) * dn
    sd = np.sqrt(np.sum((x - mean) ** 2 * pdf) * dn)
    for b in range(2):
        assert abs(d[b].mean() - mean) < 0.05, (d[b].mean(), mean)
        assert abs(d[b].std() / sd - 1) < 0.02, (d[b].std(), sd)
    assert abs(np.corrcoef(d[0].ravel(), d[1].ravel())[0, 1]) < 0.01


# ---- compositing ---------------------------------------------------------------------------------------------------
def test_add_real_back_exact(device):
    rng = np.random.RandomState(9)
    B, H, W = 3, 48, 64
    rgb = rng.randint(0, 256, (B, 3, H, W)).astype(np.uint8)
    back = rng.randint(0, 256, (B, 3, H, W)).astype(np.uint8)
    lab = rng.randint(0, 3, (B, H, W)).astype(np.uint8)
    dep = np.where(rng.rand(B, H, W) < 0.3, 0, rng.rand(B, H, W)).astype(np.float32)
    bdep = rng.rand(B, H, W).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(device)                            # noqa: E731
    for flavour, bmask, flags in (("ycb", rng.randint(0, 3, (B, H, W)).astype(np.int32), None),
                                  ("linemod", rng.choice([0, 255], (B, H, W)).astype(np.uint8), [True, False, True]),
                                  ("linemod", rng.choice([0, 255], (B, H, W)).astype(np.uint8), [False] * 3)):
        o_rgb, o_dep = train_data.add_real_back(t(rgb), t(dep), t(lab), t(back), t(bdep), t(bmask), flavour, flags)
        keep = (bmask <= 0) if flavour == "ycb" else (bmask < 255)
        f = np.ones(B, bool) if flags is None else np.array(flags)
        want = np.where((lab <= 0)[:, None] & f[:, None, None, None], back * keep[:, None], rgb)
        assert np.array_equal(o_rgb.cpu().numpy(), want)
        assert np.array_equal(o_dep.cpu().numpy(), np.where(dep > 1e-6, dep, bdep * keep.astype(np.float32)))


# ---- the builder ---------------------------------------------------------------------------------------------------
def _frames(B, H=120, W=160, n_points=1024):
    fr = synth.make_batch(31, B, n_points=n_points, height=H, width=W)
    rgb = torch.from_numpy(fr["rgb"]).cuda()
    depth = torch.from_numpy(np.ascontiguousarray(fr["dpt_xyz"][:, 2])).cuda()
    nrm = torch.from_numpy(np.random.RandomState(2).standard_normal((B, 3, H, W)).astype(np.float32)).cuda()
    lab = torch.from_numpy(np.random.RandomState(3).randint(0, 4, (B, H, W)).astype(np.uint8)).cuda()
    return rgb, depth, nrm, lab


def test_builder_without_augmentation_equals_assemble_inputs(device):
    B = 2
    rgb, depth, nrm, lab = _frames(B)
    case = synth.make_pose_case(5, n_obj=3, n_kps=8)
    K = synth.LINEMOD_K
    got = train_data.assemble_training_batch(rgb, depth, lab, K, 1024, np.tile([1, 2, 3], (B, 1)), np.stack([case["RT"][1:]] * B),
                                             case["mesh_kps"], case["mesh_ctr"], normals=nrm, seed=17)
    want = inputs.assemble_inputs(rgb, depth, nrm, K, 1024, seed=17)
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    for k in ("labels", "rgb_labels", "RTs", "kp_3ds", "ctr_3ds", "cls_ids", "kp_targ_ofst", "ctr_targ_ofst"):
        assert got[k].is_cuda, k
    assert tuple(got["kp_targ_ofst"].shape) == (B, 1024, 8, 3) and tuple(got["ctr_targ_ofst"].shape) == (B, 1024, 3)


def test_builder_with_augmentation_feeds_a_training_step(device):
    B, n_cls = 2, 4
    rgb, depth, nrm, lab = _frames(B)
    brgb, bdepth, _, blab = _frames(B)
    rng = np.random.RandomState(11)
    params = [train_data.draw_noise_params(rng, "ycb") for _ in range(B)]
    params[0].update(sharpen=10.0, motion=(60, 7), gauss=(5, 0.8))
    case = synth.make_pose_case(6, n_obj=n_cls - 1, n_kps=8)
    out = train_data.assemble_training_batch(
        rgb, depth * 1000, lab, synth.LINEMOD_K, 1024, np.tile(np.arange(1, n_cls), (B, 1)), np.stack([case["RT"][1:]] * B),
        case["mesh_kps"], case["mesh_ctr"], cam_scale=1000.0, synthetic=[True, True], noise_params=params,
        back=dict(rgb=brgb, depth=bdepth * 1000, label=blab), second_noise_params=[params[1], None], seed=3, aug_seed=4)
    assert all(v.is_cuda for v in out.values() if torch.is_tensor(v))
    assert not torch.equal(out["rgb"], rgb.float())
    torch.manual_seed(0)
    net = model.FFB6D(n_classes=n_cls, n_pts=1024).to(device).train()
    end_points = net({k: v for k, v in out.items() if k not in ("n_valid",)})
    total, _ = loss.training_loss(end_points, out["labels"].long(), out["kp_targ_ofst"], out["ctr_targ_ofst"])
    total.backward()
    assert torch.isfinite(total)
