"""The hand-written stages of the point-major forward, one at a time, on inputs the unmodified reference held at its stage
boundaries, against the outputs it held there (tests/golden/stage_point_io.npz, stage_fusion_io.npz: forward hooks on the
reference's own modules, tests/golden/make_golden_taps.py): the dilated residual block with its local feature aggregation
(fused and as the chain it replaced), the sub-sampling, the decoder step and both fusion directions.  No MIOpen convolution,
no restatement and no earlier stage of ours sits between the reference's numbers and the kernel under test; the data are real
post-activation tensors (exact zeros, correlated channels, real neighbour lists) with the seed-0 weights the reference ran with.

Bar: HOT_TOL = 1e-5 of each reference tensor's range plus the elementwise clause of `assert_close_scaled` -- fp32 kernels
against the reference's fp32 CPU result.  The tests print what they measure.

Measured on the MI355X (max error / range; the SIMT emulator, with the host's exp, measures 2.7e-7 .. 8.2e-7 on the same tests):
    f_encoder_0..3   fused 2.7e-7  3.6e-7  5.3e-7  6.2e-7      chain 2.7e-7  3.6e-7  4.6e-7  6.2e-7
    f_decoder_0..2   2.8e-7  3.8e-7  3.8e-7
    encoder fusion 1 rgb_emb (p2r) 3.2e-7   p_emb (r2p) 6.2e-7
    decoder fusion 1 rgb_emb rows U (p2r) 4.7e-7   p_emb (r2p) 6.3e-7
    sub-sampling     equal bits at all four levels
-- the size of the oracle's own distance from the same tensors on the CPU (1e-7 .. 1.1e-6, tests/test_oracle_cpu.py), i.e. fp32
summation order; no stage needed the float64 evaluation the bar would otherwise call for.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from ffb6d_amd import forward_pm, ops_pm, synth
from oracle import knn as oknn
from oracle import pyramid as opyr
from test_forward_gpu import HOT_TOL, assert_close_scaled, build

pytestmark = pytest.mark.gpu


def rows(a, device):
    """reference layout [C,N] / [C,H,W] (one frame) -> point-major [1,N,C] / pixel-major [1,H,W,C], fp32"""
    t = torch.from_numpy(np.ascontiguousarray(np.moveaxis(a, 0, -1)))
    return t.unsqueeze(0).contiguous().to(device)


def cols(t):
    """back: [1,N,C] / [1,H,W,C] -> numpy [C,N] / [C,H,W]"""
    return np.moveaxis(t[0].float().cpu().numpy(), -1, 0)


@functools.lru_cache(maxsize=None)
def stage_context(device):
    """(net, point fixture, fusion fixture, index pyramid of frame 0 as [1,...] int64 / float32 tensors on `device`): the seed-0
    weights and the frame the fixtures were recorded with; the pyramid rebuilt with oracle.knn (the generator checks that it
    equals the reference kd-tree's, and stores under `idx/` whatever index tensor does not).  Built once, read only."""
    net = build(5, 1024, device)
    point = dict(np.load(os.path.join(GOLDEN, "stage_point_io.npz")))
    fusion = dict(np.load(os.path.join(GOLDEN, "stage_fusion_io.npz")))
    frame = synth.make_frame(synth.frame_seed(7, 0), n_points=1024, height=120, width=160)
    pyr = opyr.build_pyramid(frame["cld"], frame["dpt_xyz"], oknn.knn_search)
    pyr.update({k[4:]: v for k, v in point.items() if k.startswith("idx/")})
    idx = {k: torch.from_numpy(v.astype(np.int64) if v.dtype == np.int32 else v).unsqueeze(0).to(device) for k, v in pyr.items()}
    return net, point, fusion, idx


def in_range(idx, n):
    return int(idx.min()) >= 0 and int(idx.max()) < n


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("i", range(4))
def test_encoder_point_stage_matches_the_reference(device, i, fused):
    """rndla_ds_stages[i] (RandLANet.py:170-184: mlp1, local feature aggregation, mlp2 + shortcut) at d = 32 / 64 / 128 / 256 on
    N = 1024 / 256 / 64 / 16 points: the reference's input features -> its `f_encoder_i`.  fused: one launch per half of the
    aggregation (csrc/lfa_pm.hip); not fused: posenc_mlp -> att_pool -> mlp (the chain it replaced)."""
    net, point, _, idx = stage_context(device)
    p_in = rows(point["enc_in_%d" % i], device)
    if i == 0:                                               # the 8-channel stem output is stored 16 wide, as forward() does
        p_in = torch.nn.functional.pad(p_in, (0, 16 - p_in.shape[-1])).contiguous()
    xyz, nei = idx["cld_xyz%d" % i], idx["cld_nei_idx%d" % i]
    assert nei.shape == (1, p_in.shape[1], 16) and in_range(nei, p_in.shape[1])
    keep = forward_pm.LFA_FUSED
    forward_pm.LFA_FUSED = fused
    try:
        with torch.no_grad():
            got = forward_pm.dilated_res_block(net.rndla_ds_stages[i], p_in, ops_pm.xyz_table(xyz) if fused else xyz, nei)
    finally:
        forward_pm.LFA_FUSED = keep
    assert_close_scaled(cols(got), point["f_encoder_%d" % i], HOT_TOL, ("f_encoder_%d" % i, "fused" if fused else "chain"))


@pytest.mark.parametrize("i", range(4))
def test_sub_sampling_equals_the_reference_bit_for_bit(device, i):
    """FFB6D.random_sample (ffb6d.py:159-177, :240) on rows: the max over the 16 neighbours of the first N/4 points of the
    reference's `f_encoder_i` is the `p_emb0` it fed to ds_fuse_p2r_pre_layers[i]."""
    _, point, _, idx = stage_context(device)
    f_enc, sub = rows(point["f_encoder_%d" % i], device), idx["cld_sub_idx%d" % i]
    assert sub.shape == (1, f_enc.shape[1] // 4, 16) and in_range(sub, f_enc.shape[1])
    got = cols(ops_pm.random_sample(f_enc, sub))
    assert np.array_equal(got, point["p_emb0_ds%d" % i])


@pytest.mark.parametrize("i", range(3))
def test_decoder_point_stage_matches_the_reference(device, i):
    """rndla_up_stages[i] on cat(skip, nearest_interpolation(p_emb)) (ffb6d.py:273-279) as W_a skip + gather(W_b p)."""
    net, point, _, idx = stage_context(device)
    skip, p = rows(point["dec_skip_%d" % i], device), rows(point["dec_p_%d" % i], device)
    interp = idx["cld_interp_idx%d" % (3 - i)]
    assert interp.shape == (1, skip.shape[1], 1) and in_range(interp, p.shape[1])
    with torch.no_grad():
        got = forward_pm.decode(net.rndla_up_stages[i], skip, p, interp)
    assert_close_scaled(cols(got), point["f_decoder_%d" % i], HOT_TOL, "f_decoder_%d" % i)


def test_encoder_fusion_stage_matches_the_reference(device):
    """Both fusion directions of encoder stage 1 (ffb6d.py:245-263; 128 channels, 15 x 20 pixels, 64 points) through
    forward_pm.fusion_step, the function forward() calls: reference-held rgb_emb0 / p_emb0 -> its rgb_emb / p_emb."""
    net, _, fusion, idx = stage_context(device)
    rgb0, p0 = rows(fusion["enc1/rgb_emb0"], device), rows(fusion["enc1/p_emb0"], device)
    p2r, r2p = idx["p2r_ds_nei_idx1"], idx["r2p_ds_nei_idx1"]
    n_pix = rgb0.shape[1] * rgb0.shape[2]
    assert p2r.shape == (1, n_pix, 1) and in_range(p2r, p0.shape[1]) and r2p.shape == (1, p0.shape[1], 16) and in_range(r2p, n_pix)
    with torch.no_grad():
        rgb, p = forward_pm.fusion_step(net.ds_fuse_p2r_pre_layers[1], net.ds_fuse_p2r_fuse_layers[1], net.ds_fuse_r2p_pre_layers[1],
                                        net.ds_fuse_r2p_fuse_layers[1], rgb0, p0, p2r, r2p)
    assert_close_scaled(cols(rgb), fusion["enc1/rgb_emb"], HOT_TOL, "rgb_emb_ds1 (p2r)")
    assert_close_scaled(cols(p), fusion["enc1/p_emb"], HOT_TOL, "p_emb_ds1 (r2p)")


def test_decoder_fusion_stage_matches_the_reference(device):
    """Both fusion directions of decoder stage 1 (ffb6d.py:281-298; 64 colour / 128 point channels, 60 x 80 pixels, 64 points) on the
    pixel rows U the fixture holds: every pixel one of the 64 points pools over (so the r2p direction is complete) and every 16th
    pixel (the p2r direction, which is independent per pixel), laid out as a [1,1,|U|,64] map with both index tensors renumbered."""
    net, _, fusion, _ = stage_context(device)
    U = fusion["dec1/U"]
    rgb0 = rows(fusion["dec1/rgb_emb0_U"], device).unsqueeze(1)                                   # [1,1,|U|,64]
    p0 = rows(fusion["dec1/p_emb0"], device)
    p2r = torch.from_numpy(fusion["dec1/p2r_idx_U"].astype(np.int64)).unsqueeze(0).to(device)     # [1,|U|,1]
    r2p = torch.from_numpy(fusion["dec1/r2p_idx_U"].astype(np.int64)).unsqueeze(0).to(device)     # [1,64,16]
    assert rgb0.shape[2] == len(U) >= 300 and p2r.shape == (1, len(U), 1) and in_range(p2r, p0.shape[1])
    assert r2p.shape == (1, p0.shape[1], 16) and in_range(r2p, len(U))
    with torch.no_grad():
        rgb, p = forward_pm.fusion_step(net.up_fuse_p2r_pre_layers[1], net.up_fuse_p2r_fuse_layers[1], net.up_fuse_r2p_pre_layers[1],
                                        net.up_fuse_r2p_fuse_layers[1], rgb0, p0, p2r, r2p)
    assert_close_scaled(cols(rgb.squeeze(1)), fusion["dec1/rgb_emb_U"], HOT_TOL, "rgb_emb_up1 rows U (p2r)")
    assert_close_scaled(cols(p), fusion["dec1/p_emb"], HOT_TOL, "p_emb_up1 (r2p)")
