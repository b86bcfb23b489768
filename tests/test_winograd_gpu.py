"""Winograd F(2x2,3x3) for the wide trunk convolutions on the device: each transform kernel (csrc/winograd.h) against its plain-torch
restatement (tests/winograd_ref.py), the batched-weight GEMM (csrc/mlp_pm.hip) bit for bit against 16 separate launches, the whole
convolution against F.conv2d in float64, and the forward with the form on against the form off.

Shapes: the smallest that reach every edge --
    (2, 15, 21, 256 -> 256)   odd H and W (masked stores, zero-filled last row / column); T = 176, Tp = 256: unwritten pad rows
    (1, 16, 16, 256 -> 512)   exact tiles; T = 64 -> Tp = 128: one weight matrix per single point tile
    (2,  9, 40, 512 -> 512)   T = 200: a plane's live rows straddle a point tile"""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import winograd_ref as wr
from conftest import GOLDEN
from ffb6d_amd import _lib, forward_pm, ops, ops_pm, pyramid, synth
from ffb6d_amd import model as M

pytestmark = pytest.mark.gpu

SHAPES = [(2, 15, 21, 256, 256), (1, 16, 16, 256, 512), (2, 9, 40, 512, 512)]
HOT_TOL = 1e-5          # tests/test_forward_gpu.py
TRANSFORM_TOL = 1e-6    # of the tensor's range: adds and subtracts only, the orders of the sums may differ
CONV_TOL = 1e-5         # the project's per-operator bar (csrc/mlp_pm.hip header)


def rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


@pytest.fixture(scope="module")
def data(device):
    """per shape: x, filter, U, V (restatement), M = V U^T (batched GEMM), BatchNorm-like parameters, a residual map"""
    out = {}
    for shape in SHAPES:
        B, H, W, C, O = shape
        g = torch.Generator().manual_seed(sum(shape))
        d = {"x": torch.randn(B, H, W, C, generator=g), "w": torch.randn(O, C, 3, 3, generator=g) / (9 * C) ** .5,
             "scale": torch.rand(O, generator=g) + .5, "shift": torch.randn(O, generator=g),
             "rscale": torch.rand(O, generator=g) + .5, "rshift": torch.randn(O, generator=g),
             "res": torch.randn(B, H, W, O, generator=g)}
        d = {k: v.to(device) for k, v in d.items()}
        d["u"] = wr.filter_transform(d["w"])
        d["v"] = wr.input_transform(d["x"])
        out[shape] = d
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_input_transform_matches_the_restatement_and_leaves_the_pad_rows_alone(device, data, shape):
    B, H, W, C, O = shape
    d = data[shape]
    T, Tp = ops_pm.wino_tiles(B, H, W)
    assert T == wr.tiles(B, H, W) and Tp % 128 == 0 and 0 <= Tp - T < 128
    buf = torch.full((16, Tp, C), -7.25, device=device)
    v = ops_pm.wino_input(d["x"], out=buf)
    err = rel(v[:, :T], d["v"])
    print(shape, "input transform: max err / range %.2e" % err)
    assert err <= TRANSFORM_TOL
    assert bool((v[:, T:] == -7.25).all())            # rows T .. Tp - 1 of every plane: never written


@pytest.mark.parametrize("shape", SHAPES)
def test_output_transform_matches_the_restatement(device, data, shape):
    B, H, W, C, O = shape
    d = data[shape]
    T, Tp = ops_pm.wino_tiles(B, H, W)
    m = torch.full((16, Tp, O), float("nan"), device=device)         # pad rows: never read
    m[:, :T] = torch.randn(16, T, O, generator=torch.Generator().manual_seed(5)).to(device)
    y = wr.output_transform(m[:, :T], (B, H, W))
    one, zero = torch.ones(O, device=device), torch.zeros(O, device=device)
    got = ops_pm.wino_output(m, (B, H, W), one, zero)
    err = rel(got, y)
    print(shape, "output transform: max err / range %.2e" % err)
    assert err <= TRANSFORM_TOL
    # fused BatchNorm / residual / ReLU: the restatement followed by the existing affine_act_
    for what, kw in (("no residual", {}), ("residual", {"residual": d["res"]}),
                     ("affine residual", {"residual": d["res"], "res_affine": (d["rscale"], d["rshift"])})):
        got = ops_pm.wino_output(m, (B, H, W), d["scale"], d["shift"], act=ops.ACT_RELU, **kw)
        want = ops_pm.affine_act_(y.clone(), d["scale"], d["shift"], act=ops.ACT_RELU, **kw)
        err = rel(got, want)
        print(shape, "output transform +", what, ": max err / range %.2e" % err)
        assert got.shape == (B, H, W, O) and err <= TRANSFORM_TOL
        assert bool((got >= 0).all()) and bool((got == 0).any())


@pytest.mark.parametrize("shape", SHAPES)
def test_batched_gemm_equals_sixteen_launches_bit_for_bit(device, data, shape):
    B, H, W, C, O = shape
    d = data[shape]
    T, Tp = ops_pm.wino_tiles(B, H, W)
    v = torch.zeros(16, Tp, C, device=device)
    v[:, :T] = d["v"]
    # 16 separate launches in the two forms the batched entry has (at these row counts the automatic choice of ops_pm.mlp is the form
    # that splits K over the waves, whose sums run in another order -- the one form that does not share its bits with the others)
    want = torch.stack([ops_pm.mlp(v[xi], d["u"][xi], tile_hint=8) for xi in range(16)])
    assert torch.equal(want, torch.stack([ops_pm.mlp(v[xi], d["u"][xi], tile_hint=7) for xi in range(16)]))
    seq = ops_pm.mlp_batched(v, d["u"])
    lds = ops_pm.mlp_batched(v, d["u"], tile_hint=7)
    pairs = ops_pm.mlp_batched(v, d["u"], tile_hint=8 + 256 * 2)      # sequences of two channel tiles: the riding epilogue
    assert torch.equal(seq, want) and torch.equal(lds, want) and torch.equal(pairs, want)
    assert rel(seq, torch.einsum("xtc,xoc->xto", v.double(), d["u"].double())) <= CONV_TOL


def test_batched_gemm_refuses_what_it_cannot_run(device):
    x, w = torch.zeros(2, 128, 128, device=device), torch.zeros(2, 128, 128, device=device)
    ops_pm.mlp_batched(x, w)
    with pytest.raises(_lib.FFB6DNativeError, match="LIN"):
        ops_pm.mlp_batched(x, w, tile_hint=8 + 256 * 0xF2)             # balanced sequences cross point tiles
    with pytest.raises(_lib.FFB6DNativeError, match="tile_hint"):
        ops_pm.mlp_batched(x, w, tile_hint=1)
    with pytest.raises(_lib.FFB6DNativeError, match="multiple of 128"):
        ops_pm.mlp_batched(torch.zeros(2, 64, 128, device=device), w)
    with pytest.raises(_lib.FFB6DNativeError, match="K >= 128"):
        ops_pm.mlp_batched(torch.zeros(2, 128, 64, device=device), torch.zeros(2, 128, 64, device=device))


@pytest.mark.parametrize("shape", SHAPES)
def test_whole_convolution_against_float64(device, data, shape):
    B, H, W, C, O = shape
    d = data[shape]
    conv = torch.nn.Conv2d(C, O, 3, 1, 1, bias=False).to(device)
    with torch.no_grad():
        conv.weight.copy_(d["w"])
        assert forward_pm.wino_ok(conv, d["x"])
        got = forward_pm.conv_wino(d["x"], conv, d["scale"], d["shift"], residual=d["res"])
    y = F.conv2d(d["x"].double().permute(0, 3, 1, 2), d["w"].double(), padding=1).permute(0, 2, 3, 1)
    want = torch.relu(y * d["scale"].double() + d["shift"].double() + d["res"].double())
    err = rel(got, want)
    print(shape, "winograd convolution + BN + residual + ReLU against float64: max err / range %.2e" % err)
    assert err <= CONV_TOL


def test_routing_takes_only_the_layers_the_form_is_for(device):
    x = torch.zeros(1, 8, 8, 256, device=device)
    ok = torch.nn.Conv2d(256, 256, 3, 1, 1, bias=False).to(device)
    assert forward_pm.wino_ok(ok, x)
    for bad in (torch.nn.Conv2d(256, 256, 3, 2, 1, bias=False), torch.nn.Conv2d(256, 256, 3, 1, 1, bias=True),
                torch.nn.Conv2d(256, 256, 1, 1, 0, bias=False), torch.nn.Conv2d(256, 256, 3, 1, 2, dilation=2, bias=False),
                torch.nn.Conv2d(256, 256, 3, 1, 1, groups=2, bias=False)):
        assert not forward_pm.wino_ok(bad.to(device), x)
    assert not forward_pm.wino_ok(torch.nn.Conv2d(128, 256, 3, 1, 1, bias=False).to(device), torch.zeros(1, 8, 8, 128, device=device))
    assert not forward_pm.wino_ok(ok, x.bfloat16())
    assert not forward_pm.wino_ok(ok, torch.zeros(8, 480, 640, 256, device="meta"))       # V would pass 2 GiB


def test_forward_with_the_form_on_agrees_with_off_and_repeats_its_bits(device, monkeypatch):
    config, bs, n_pts, h, w, n_cls = 7, 2, 1024, 120, 160, 5
    with open(os.path.join(GOLDEN, "state_dict_keys.json")) as fh:
        shapes = json.load(fh)
    net = M.FFB6D(n_classes=n_cls, n_pts=n_pts)
    net.load_state_dict(synth.synth_state_dict_from_shapes(shapes, seed=0, n_classes=n_cls))
    net = net.to(device).eval()
    inputs = pyramid.frames_to_device(synth.make_batch(config, bs, n_points=n_pts, height=h, width=w), device)
    calls = []
    real = ops_pm.wino_input
    monkeypatch.setattr(ops_pm, "wino_input", lambda x, out=None: (calls.append(tuple(x.shape)), real(x, out))[1])

    def run(on):
        monkeypatch.setattr(forward_pm, "TRUNK_WINOGRAD", on)
        taps = {}
        with torch.no_grad():
            ep = dict(net(inputs, taps=taps))
        assert len(taps) == 14
        ep.update(taps)
        return {k: v.clone() for k, v in ep.items() if torch.is_tensor(v) and v.is_floating_point()}

    off = run(False)
    assert not calls
    on = run(True)
    assert len(calls) == 17 and {c[-1] for c in calls} == {256, 512}      # 6 + 3 blocks, less the 128 -> 256 convolution
    assert len(off) == 17
    for k in sorted(off):
        err = rel(on[k], off[k])
        print(k, "form on against off: max err / range %.2e" % err)
        assert err <= HOT_TOL, k
    # the converted layers repeat their bits: the blocks whose two convolutions both take the form, run twice on the same input
    blocks = [m for m in net.modules() if isinstance(m, M.ResBlock) and m.downsample is None and m.conv1.in_channels >= 256]
    assert len(blocks) == 7
    for rb in blocks:
        x = torch.randn(2, 15, 20, rb.conv1.in_channels, device=device)
        with torch.no_grad():
            a, b = forward_pm.res_block(rb, x), forward_pm.res_block(rb, x)
        assert torch.equal(a, b)
