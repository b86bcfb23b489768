"""Winograd F(4x4,3x3) for the wide trunk convolutions, the parts that need no GPU: the plain-torch restatement of the three transforms
(tests/winograd4_ref.py, the specification of the F(4x4) kernels of csrc/winograd.h) against F.conv2d, the cached filter transform,
the two kernels on the SIMT-emulated library, the rule that picks the variant, and what the method costs in accuracy -- on one
convolution and through the whole network, measured on the oracle."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import winograd4_ref as w4
from conftest import GOLDEN
from ffb6d_amd import forward_pm, ops, ops_pm, synth

TRANSFORM_TOL = 1e-6    # of the tensor's range (tests/test_winograd_gpu.py); the fp32 restatement against the float64 one: 1.2e-7 .. 1.6e-7
CONV_TOL = 1e-5         # the project's per-operator bar (csrc/mlp_pm.hip header)
EMU_SHAPES = [(2, 13, 18, 8),       # H % 4 = 1, W % 4 = 2, T = 40
              (1, 16, 16, 12),      # exact tiles
              (2, 9, 43, 8),        # W % 4 = 3
              (3, 23, 30, 8)]       # H % 4 = 3, T = 144 -> Tp = 256: the live rows straddle a point tile


def rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


@pytest.mark.parametrize("shape", [(2, 8, 8), (2, 7, 9), (2, 6, 11), (2, 5, 10), (1, 1, 1), (1, 13, 18)])
def test_restatement_equals_conv2d_in_float64(shape):
    B, H, W = shape
    g = torch.Generator().manual_seed(H * 16 + W)
    x = torch.randn(B, H, W, 5, dtype=torch.float64, generator=g)
    w = torch.randn(3, 5, 3, 3, dtype=torch.float64, generator=g)
    want = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    got = w4.conv(x, w)
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    print(shape, "max abs err", err)
    assert err <= 1e-12


def test_filter_transform_of_the_package_is_the_restatement_and_follows_weight_edits():
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(8, 12, 3, 1, 1, bias=False)
    u0 = forward_pm.wino4_weights(conv)
    assert u0.dtype == torch.float32 and u0.shape == (36, 12, 8) and u0.is_contiguous()
    assert torch.equal(u0, w4.filter_transform(conv.weight.detach()))
    assert forward_pm.wino4_weights(conv) is u0                      # cached
    with torch.no_grad():
        conv.weight.mul_(1.5)                                        # in-place edit: the version counter moves
    u1 = forward_pm.wino4_weights(conv)
    assert u1 is not u0 and not torch.equal(u1, u0)
    assert torch.equal(u1, w4.filter_transform(conv.weight.detach()))
    assert forward_pm.wino_weights(conv).shape == (16, 12, 8)        # the F(2x2) filter keeps its own cache slot


@pytest.mark.parametrize("shape", EMU_SHAPES)
def test_input_kernel_on_the_emulator_matches_the_restatement_and_leaves_the_pad_rows_alone(emu, shape):
    B, H, W, C = shape
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(sum(shape)))
    T, Tp = ops_pm.wino4_tiles(B, H, W)
    assert T == w4.tiles(B, H, W) and Tp % 128 == 0 and 0 <= Tp - T < 128
    want = w4.input_transform(x.double())
    err32 = rel(w4.input_transform(x), want)
    buf = torch.full((36, Tp, C), -7.25)
    v = ops_pm.wino4_input(x, out=buf)
    err = rel(v[:, :T], want)
    print(shape, "input transform: kernel %.2e, fp32 restatement %.2e of range against float64" % (err, err32))
    assert err <= TRANSFORM_TOL
    assert bool((v[:, T:] == -7.25).all())            # rows T .. Tp - 1 of every plane: never written


@pytest.mark.parametrize("shape", EMU_SHAPES)
def test_output_kernel_on_the_emulator_matches_the_restatement(emu, shape):
    B, H, W, O = shape
    g = torch.Generator().manual_seed(sum(shape) + 1)
    T, Tp = ops_pm.wino4_tiles(B, H, W)
    m = torch.full((36, Tp, O), float("nan"))                        # pad rows: never read
    m[:, :T] = torch.randn(36, T, O, generator=g)
    scale, shift = torch.rand(O, generator=g) + .5, torch.randn(O, generator=g)
    rscale, rshift = torch.rand(O, generator=g) + .5, torch.randn(O, generator=g)
    res = torch.randn(B, H, W, O, generator=g)
    y64 = w4.output_transform(m[:, :T].double(), (B, H, W))
    err32 = rel(w4.output_transform(m[:, :T], (B, H, W)), y64)
    got = ops_pm.wino4_output(m, (B, H, W), torch.ones(O), torch.zeros(O))
    err = rel(got, y64)
    print(shape, "output transform: kernel %.2e, fp32 restatement %.2e of range against float64" % (err, err32))
    assert got.shape == (B, H, W, O) and not bool(torch.isnan(got).any())
    assert err <= TRANSFORM_TOL
    # fused BatchNorm / residual / ReLU: the restatement followed by the existing affine_act_
    for what, kw in (("no residual", {}), ("residual", {"residual": res}),
                     ("affine residual", {"residual": res, "res_affine": (rscale, rshift)})):
        got = ops_pm.wino4_output(m, (B, H, W), scale, shift, act=ops.ACT_RELU, **kw)
        want = ops_pm.affine_act_(y64.float(), scale, shift, act=ops.ACT_RELU, **kw)
        err = rel(got, want)
        print(shape, "output transform +", what, ": max err / range %.2e" % err)
        assert got.shape == (B, H, W, O) and not bool(torch.isnan(got).any()) and err <= TRANSFORM_TOL
        assert bool((got >= 0).all()) and bool((got == 0).any())


def test_the_variant_is_chosen_by_cost(monkeypatch):
    """(36 Tp4, 16 Tp2, variant) on the benchmark's trunk map, on the maps of the existing forward tests and on 30 x 40.  2 x 13 x 17 has
    126 F(2x2) tiles, so Tp2 = 128 and 16 Tp2 = 2048 (the proposal of the rule listed 4096 there; the variant is F(2x2) either way)."""
    def cost(B, H, W):
        return 36 * ops_pm.wino4_tiles(B, H, W)[1], 16 * ops_pm.wino_tiles(B, H, W)[1]

    assert forward_pm.TRUNK_WINOGRAD_F4 is True
    for (B, H, W), c4, c2, m in (((8, 60, 80), 87552, 153600, 4), ((2, 15, 20), 4608, 4096, 2), ((2, 13, 17), 4608, 2048, 2),
                                 ((1, 30, 40), 4608, 6144, 4)):
        assert cost(B, H, W) == (c4, c2) and forward_pm.wino_variant(B, H, W) == m
    for B, H, W in ((2, 15, 21), (1, 16, 16), (2, 9, 40)):          # SHAPES of tests/test_winograd_gpu.py
        assert forward_pm.wino_variant(B, H, W) == 2
    assert cost(1, 16, 16) == (36 * 128, 16 * 128) and forward_pm.wino_variant(1, 8, 8) == 2      # a tie stays with F(2x2)
    monkeypatch.setattr(forward_pm, "TRUNK_WINOGRAD_F4", False)
    assert forward_pm.wino_variant(8, 60, 80) == 2


@pytest.mark.parametrize("shape", [(2, 13, 18, 256, 256), (1, 30, 40, 512, 512)])
def test_one_fp32_convolution_stays_inside_the_operator_bar(shape):
    """One 3x3 convolution in fp32 by the restatement (filter transform in float64, rounded once) against F.conv2d in float64, randn data
    scaled like tests/test_winograd_gpu.py: <= CONV_TOL = 1e-5 of the output range.  Measured with these points (0, 1, -1, 2, -1/2):
    4.1e-6 at (2,13,18,256->256) and 4.3e-6 at (1,30,40,512->512) (4.0e-6 .. 5.8e-6 over these and the three shapes of
    tests/test_winograd_gpu.py; F(2x2) 5.8e-7 .. 7.4e-7).  The textbook points 0, +-1, +-2 of Lavin & Gray give 1.11e-5 and 1.20e-5 on the
    same data (1.08e-5 .. 1.27e-5 over the five shapes) and would fail this test."""
    B, H, W, C, O = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(O, C, 3, 3, generator=g) / (9 * C) ** .5
    want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)
    err = rel(w4.conv(x, w), want)
    print(shape, "F(4x4) restatement in fp32 against float64: max err / range %.2e" % err)
    assert err <= CONV_TOL


class _Functional:
    """torch.nn.functional with conv2d replaced (handed to oracle.forward_ref as its `F`)"""

    def __init__(self, conv2d):
        self.conv2d = conv2d

    def __getattr__(self, name):
        return getattr(F, name)


def test_winograd4_on_the_wide_layers_stays_at_the_reordering_floor(monkeypatch):
    """oracle/forward_ref.py in fp32 at the smallest test geometry with every 3x3 / stride 1 / padding 1 convolution of Cin >= 256 (all on
    the 15 x 20 trunk map) computed by the F(4x4) restatement (filter transform in fp64, rounded once) against the unmodified fp32
    oracle: the maximum over the three outputs and the 14 stage taps, relative to each tensor's range, must stay <= 5e-6, the bound
    and the reasoning of the F(2x2) test (tests/test_winograd_cpu.py: the floor of summing in another order is 2.0e-6, 2.5x is the
    margin for another BLAS, HOT_TOL is 1e-5).  Measured when this test was written: 2.1e-6 (F(2x2) in the same run: 2.2e-6)."""
    from oracle import forward_ref
    from oracle import knn as oknn
    from oracle import pyramid as opyr
    with open(os.path.join(GOLDEN, "state_dict_keys.json")) as fh:
        shapes = json.load(fh)
    sd = synth.synth_state_dict_from_shapes(shapes, seed=0, n_classes=5)
    frames = synth.make_batch(7, 2, n_points=1024, height=120, width=160)
    pyr = opyr.build_batch(frames, oknn.knn_search)
    inp = {"rgb": torch.from_numpy(frames["rgb"].astype(np.float32)), "cld_rgb_nrm": torch.from_numpy(frames["cld_rgb_nrm"]),
           "choose": torch.from_numpy(frames["choose"].astype(np.int64))}
    for k, v in pyr.items():
        inp[k] = torch.from_numpy(v.astype(np.int64) if v.dtype == np.int32 else v)
    converted = []

    def conv2d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        s = stride if isinstance(stride, int) else stride[0]
        p = padding if isinstance(padding, int) else padding[0]
        if w.dim() == 4 and tuple(w.shape[2:]) == (3, 3) and s == 1 and p == 1 and dilation == 1 and groups == 1 and w.shape[1] >= 256 \
                and tuple(x.shape[2:]) == (15, 20):
            converted.append(tuple(w.shape))
            y = w4.conv(x.permute(0, 2, 3, 1), w).permute(0, 3, 1, 2)
            return y if b is None else y + b[None, :, None, None]
        return F.conv2d(x, w, b, stride, padding, dilation, groups)

    def run():
        taps = {}
        with torch.no_grad():
            out = dict(forward_ref.ffb6d_forward(sd, inp, taps=taps))
        assert len(taps) == 14
        out.update(taps)
        return {k: v.double() for k, v in out.items() if torch.is_tensor(v) and v.is_floating_point()}

    direct = run()
    monkeypatch.setattr(forward_ref, "F", _Functional(conv2d))
    wino = run()
    assert len(converted) >= 17 and sorted(direct) == sorted(wino) and len(direct) == 17
    worst = 0.0
    for k in sorted(direct):
        err = float((wino[k] - direct[k]).abs().max() / direct[k].abs().max())
        print(k, "winograd F(4x4) vs direct, max err / range %.2e" % err)
        worst = max(worst, err)
    print("worst %.2e over %d converted convolutions" % (worst, len(converted)))
    assert worst <= 5e-6
