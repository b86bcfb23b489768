"""Winograd F(4x4,3x3) for the wide trunk convolutions on the device: each F(4x4) transform kernel (csrc/winograd.h) against its
plain-torch restatement (tests/winograd4_ref.py) evaluated in float64, the batched-weight GEMM with 36 matrices bit for bit against 36
separate launches, the whole convolution against F.conv2d in float64, the routing, and the forward with the form on against off.

Shapes: the smallest that reach every edge --
    (2, 13, 18, 256 -> 256)   H % 4 = 1, W % 4 = 2 (masked stores, zero-filled window rows / columns); T = 40 -> Tp = 128
    (1, 16, 16, 256 -> 512)   exact tiles; T = 16
    (2,  9, 43, 256 -> 256)   W % 4 = 3
    (3, 23, 30, 512 -> 512)   H % 4 = 3; T = 144 -> Tp = 256: a plane's live rows straddle a point tile"""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import winograd4_ref as w4
from conftest import GOLDEN
from ffb6d_amd import forward_pm, ops, ops_pm, pyramid, synth
from ffb6d_amd import model as M

pytestmark = pytest.mark.gpu

SHAPES = [(2, 13, 18, 256, 256), (1, 16, 16, 256, 512), (2, 9, 43, 256, 256), (3, 23, 30, 512, 512)]
HOT_TOL = 1e-5          # tests/test_forward_gpu.py
TRANSFORM_TOL = 1e-6    # of the tensor's range, against the restatement in float64 (the fp32 restatement itself: 1.2e-7 .. 1.6e-7)
CONV_TOL = 1e-5         # the project's per-operator bar (csrc/mlp_pm.hip header)


def rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


@pytest.fixture(scope="module")
def data(device):
    """per shape: x, filter, U, V (restatement in float64), BatchNorm-like parameters, a residual map"""
    out = {}
    for shape in SHAPES:
        B, H, W, C, O = shape
        g = torch.Generator().manual_seed(sum(shape))
        d = {"x": torch.randn(B, H, W, C, generator=g), "w": torch.randn(O, C, 3, 3, generator=g) / (9 * C) ** .5,
             "scale": torch.rand(O, generator=g) + .5, "shift": torch.randn(O, generator=g),
             "rscale": torch.rand(O, generator=g) + .5, "rshift": torch.randn(O, generator=g),
             "res": torch.randn(B, H, W, O, generator=g)}
        d = {k: v.to(device) for k, v in d.items()}
        d["u"] = w4.filter_transform(d["w"])
        d["v64"] = w4.input_transform(d["x"].double())
        out[shape] = d
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_input_transform_matches_the_restatement_and_leaves_the_pad_rows_alone(device, data, shape):
    B, H, W, C, O = shape
    d = data[shape]
    T, Tp = ops_pm.wino4_tiles(B, H, W)
    assert T == w4.tiles(B, H, W) and Tp % 128 == 0 and 0 <= Tp - T < 128
    buf = torch.full((36, Tp, C), -7.25, device=device)
    v = ops_pm.wino4_input(d["x"], out=buf)
    err = rel(v[:, :T], d["v64"])
    print(shape, "input transform: max err / range %.2e" % err)
    assert err <= TRANSFORM_TOL
    assert bool((v[:, T:] == -7.25).all())            # rows T .. Tp - 1 of every plane: never written


@pytest.mark.parametrize("shape", SHAPES)
def test_output_transform_matches_the_restatement(device, data, shape):
    B, H, W, C, O = shape
    d = data[shape]
    T, Tp = ops_pm.wino4_tiles(B, H, W)
    m = torch.full((36, Tp, O), float("nan"), device=device)         # pad rows: never read
    m[:, :T] = torch.randn(36, T, O, generator=torch.Generator().manual_seed(5)).to(device)
    y64 = w4.output_transform(m[:, :T].double(), (B, H, W))
    one, zero = torch.ones(O, device=device), torch.zeros(O, device=device)
    got = ops_pm.wino4_output(m, (B, H, W), one, zero)
    err = rel(got, y64)
    print(shape, "output transform: max err / range %.2e" % err)
    assert got.shape == (B, H, W, O) and not bool(torch.isnan(got).any())
    assert err <= TRANSFORM_TOL
    # fused BatchNorm / residual / ReLU: the restatement followed by the existing affine_act_
    for what, kw in (("no residual", {}), ("residual", {"residual": d["res"]}),
                     ("affine residual", {"residual": d["res"], "res_affine": (d["rscale"], d["rshift"])})):
        got = ops_pm.wino4_output(m, (B, H, W), d["scale"], d["shift"], act=ops.ACT_RELU, **kw)
        want = ops_pm.affine_act_(y64.float(), d["scale"], d["shift"], act=ops.ACT_RELU, **kw)
        err = rel(got, want)
        print(shape, "output transform +", what, ": max err / range %.2e" % err)
        assert got.shape == (B, H, W, O) and not bool(torch.isnan(got).any()) and err <= TRANSFORM_TOL
        assert bool((got >= 0).all()) and bool((got == 0).any())


def test_batched_gemm_equals_thirty_six_launches_bit_for_bit(device):
    shape = (3, 23, 30, 256, 256)
    B, H, W, C, O = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, w = torch.randn(B, H, W, C, generator=g).to(device), (torch.randn(O, C, 3, 3, generator=g) / (9 * C) ** .5).to(device)
    u = w4.filter_transform(w)
    T, Tp = ops_pm.wino4_tiles(B, H, W)
    v = torch.zeros(36, Tp, C, device=device)
    v[:, :T] = w4.input_transform(x)
    want = torch.stack([ops_pm.mlp(v[xi], u[xi], tile_hint=8) for xi in range(36)])
    got = ops_pm.mlp_batched(v, u)
    assert got.shape == (36, Tp, O) and torch.equal(got, want)
    assert torch.equal(ops_pm.mlp_batched(v, u, tile_hint=7), want)
    assert torch.equal(ops_pm.mlp_batched(v, u, tile_hint=8 + 256 * 2), want)
    assert rel(got, torch.einsum("xtc,xoc->xto", v.double(), u.double())) <= CONV_TOL


@pytest.mark.parametrize("shape", SHAPES)
def test_whole_convolution_against_float64(device, data, shape):
    B, H, W, C, O = shape
    d = data[shape]
    conv = torch.nn.Conv2d(C, O, 3, 1, 1, bias=False).to(device)
    with torch.no_grad():
        conv.weight.copy_(d["w"])
        assert forward_pm.wino_ok(conv, d["x"], m=4)
        got = forward_pm.conv_wino(d["x"], conv, d["scale"], d["shift"], residual=d["res"], m=4)
    y = F.conv2d(d["x"].double().permute(0, 3, 1, 2), d["w"].double(), padding=1).permute(0, 2, 3, 1)
    want = torch.relu(y * d["scale"].double() + d["shift"].double() + d["res"].double())
    err = rel(got, want)
    print(shape, "winograd F(4x4) convolution + BN + residual + ReLU against float64: max err / range %.2e" % err)
    assert err <= CONV_TOL


def test_routing_takes_only_the_layers_the_form_is_for_and_checks_the_variant_it_takes(device, monkeypatch):
    x = torch.zeros(1, 30, 40, 256, device=device)                  # the rule picks F(4x4) here
    ok = torch.nn.Conv2d(256, 256, 3, 1, 1, bias=False).to(device)
    assert forward_pm.wino_variant(1, 30, 40) == 4 and forward_pm.wino_variant(1, 8, 8) == 2
    assert forward_pm.wino_ok(ok, x) and forward_pm.wino_ok(ok, torch.zeros(1, 8, 8, 256, device=device))
    for bad in (torch.nn.Conv2d(256, 256, 3, 2, 1, bias=False), torch.nn.Conv2d(256, 256, 3, 1, 1, bias=True),
                torch.nn.Conv2d(256, 256, 1, 1, 0, bias=False), torch.nn.Conv2d(256, 256, 3, 1, 2, dilation=2, bias=False),
                torch.nn.Conv2d(256, 256, 3, 1, 1, groups=2, bias=False)):
        assert not forward_pm.wino_ok(bad.to(device), x)
    assert not forward_pm.wino_ok(torch.nn.Conv2d(128, 256, 3, 1, 1, bias=False).to(device), torch.zeros(1, 30, 40, 128, device=device))
    assert not forward_pm.wino_ok(ok, x.bfloat16())
    assert not forward_pm.wino_ok(ok, torch.zeros(8, 480, 640, 256, device="meta"))       # V would pass 2 GiB in either variant
    # the 2 GiB check uses the sizes of the variant taken: on 8 x 224 x 320 V of F(2x2) is 16 * 143360 rows of 1 KiB = 2.3 GB, V of
    # F(4x4) is 36 * 35840 rows = 1.3 GB
    big = torch.zeros(8, 224, 320, 256, device="meta")
    assert forward_pm.wino_variant(8, 224, 320) == 4
    assert forward_pm.wino_ok(ok, big) and forward_pm.wino_ok(ok, big, m=4) and not forward_pm.wino_ok(ok, big, m=2)
    monkeypatch.setattr(forward_pm, "TRUNK_WINOGRAD_F4", False)
    assert forward_pm.wino_variant(1, 30, 40) == 2 and forward_pm.wino_ok(ok, x) and not forward_pm.wino_ok(ok, big)
    monkeypatch.setattr(forward_pm, "TRUNK_WINOGRAD", False)
    assert not forward_pm.wino_ok(ok, x) and not forward_pm.wino_ok(ok, x, m=4)


def test_forward_with_the_form_on_agrees_with_off_and_repeats_its_bits(device, monkeypatch):
    config, bs, n_pts, h, w, n_cls = 7, 1, 1024, 240, 320, 5       # trunk map 1 x 30 x 40: the rule picks F(4x4)
    with open(os.path.join(GOLDEN, "state_dict_keys.json")) as fh:
        shapes = json.load(fh)
    net = M.FFB6D(n_classes=n_cls, n_pts=n_pts)
    net.load_state_dict(synth.synth_state_dict_from_shapes(shapes, seed=0, n_classes=n_cls))
    net = net.to(device).eval()
    inputs = pyramid.frames_to_device(synth.make_batch(config, bs, n_points=n_pts, height=h, width=w), device)
    calls = {"wino_input": [], "wino4_input": []}
    for name in calls:
        real = getattr(ops_pm, name)
        monkeypatch.setattr(ops_pm, name, lambda x, out=None, name=name, real=real: (calls[name].append(tuple(x.shape)), real(x, out))[1])

    def run(on):
        monkeypatch.setattr(forward_pm, "TRUNK_WINOGRAD_F4", on)
        for c in calls.values():
            c.clear()
        taps = {}
        with torch.no_grad():
            ep = dict(net(inputs, taps=taps))
        assert len(taps) == 14
        ep.update(taps)
        return {k: v.clone() for k, v in ep.items() if torch.is_tensor(v) and v.is_floating_point()}

    off = run(False)
    assert len(calls["wino_input"]) == 17 and not calls["wino4_input"]
    on = run(True)
    assert len(calls["wino4_input"]) == 17 and not calls["wino_input"]
    assert {c[1:3] for c in calls["wino4_input"]} == {(30, 40)} and {c[-1] for c in calls["wino4_input"]} == {256, 512}
    assert len(off) == 17
    for k in sorted(off):
        err = rel(on[k], off[k])
        print(k, "F(4x4) on against off: max err / range %.2e" % err)
        assert err <= HOT_TOL, k
    # the converted layers repeat their bits: the blocks whose two convolutions both take the form, run twice on the same input
    blocks = [m for m in net.modules() if isinstance(m, M.ResBlock) and m.downsample is None and m.conv1.in_channels >= 256]
    assert len(blocks) == 7
    for rb in blocks:
        x = torch.randn(1, 30, 40, rb.conv1.in_channels, device=device)
        calls["wino4_input"].clear()
        with torch.no_grad():
            a, b = forward_pm.res_block(rb, x), forward_pm.res_block(rb, x)
        assert torch.equal(a, b) and len(calls["wino4_input"]) == 4
