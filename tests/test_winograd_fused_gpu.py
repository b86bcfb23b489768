"""The fused Winograd F(4x4,3x3) convolution of the narrow trunk layers on the device (csrc/winograd_fused.h): the whole operator against
float64, what it may and may not touch, repeatable bits, the host checks, and the forward with the form on against off.

Shapes: the smallest that reach every edge --
    (1,  4,  4,  64 ->  64)   one tile, 15 idle tile slots
    (1,  5,  3, 128 -> 128)   map narrower than a window; two K chunks, two channel blocks
    (2, 13, 18,  64 ->  64)   40 tiles: partial last block, H % 4 = 1, W % 4 = 2, a tile block crossing the frame boundary
    (2,  9, 43,  64 ->  64)   W % 4 = 3
    (1, 16, 16, 128 -> 128)   exact blocks
    (3, 23, 30, 128 -> 128)   H % 4 = 3, 144 tiles
    (2, 13, 18, 128 -> 256)   the widening layer: four channel blocks"""
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

SHAPES = [(1, 4, 4, 64, 64), (1, 5, 3, 128, 128), (2, 13, 18, 64, 64), (2, 9, 43, 64, 64), (1, 16, 16, 128, 128), (3, 23, 30, 128, 128),
          (2, 13, 18, 128, 256)]
HOT_TOL = 1e-5          # tests/test_forward_gpu.py
CONV_TOL = 1e-5         # the project's per-operator bar (csrc/mlp_pm.hip header)


def rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


@pytest.fixture(scope="module")
def data(device):
    """per shape: x, filter, U, BatchNorm-like parameters, a residual map, the convolution in float64"""
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
        d["y64"] = F.conv2d(d["x"].double().permute(0, 3, 1, 2), d["w"].double(), padding=1).permute(0, 2, 3, 1)
        out[shape] = d
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_whole_operator_against_float64(device, data, shape):
    """Convolution + BatchNorm + residual + ReLU, then with the projected residual, in both workgroup shapes of the kernel, <= 1e-5 of the
    output range against float64.  Measured worst over the seven shapes, both residual forms and both workgroup shapes: 2.0e-6 of range
    (the fp32 restatement alone: up to 3.4e-6)."""
    d = data[shape]
    for what, kw, add in (("residual", {"residual": d["res"]}, d["res"].double()),
                          ("projected residual", {"residual": d["res"], "res_affine": (d["rscale"], d["rshift"])},
                           d["res"].double() * d["rscale"].double() + d["rshift"].double())):
        want = torch.relu(d["y64"] * d["scale"].double() + d["shift"].double() + add)
        for form in (1, 2):
            got = ops_pm.wino4_conv(d["x"], d["u"], d["scale"], d["shift"], act=ops.ACT_RELU, form=form, **kw)
            err = rel(got, want)
            print(shape, "form", form, "fused F(4x4) convolution + BN +", what, "+ ReLU against float64: max err / range %.2e" % err)
            assert got.shape == want.shape and err <= CONV_TOL
    assert torch.equal(ops_pm.wino4_conv(d["x"], d["u"], d["scale"], d["shift"], act=ops.ACT_RELU, residual=d["res"]),
                       ops_pm.wino4_conv(d["x"], d["u"], d["scale"], d["shift"], act=ops.ACT_RELU, residual=d["res"], form=1))


@pytest.mark.parametrize("shape", SHAPES)
def test_writes_only_its_output_reads_only_its_map_and_repeats_its_bits(device, data, shape):
    B, H, W, C, O = shape
    d = data[shape]
    nx, no, pad = B * H * W * C, B * H * W * O, 4096
    xbuf = torch.full((nx + 2 * pad,), float("nan"), device=device)
    xbuf[pad:pad + nx] = d["x"].reshape(-1)
    x = xbuf[pad:pad + nx].view(B, H, W, C)
    for form in (1, 2):
        obuf = torch.full((no + 2 * pad,), float("nan"), device=device)
        out = obuf[pad:pad + no].view(B, H, W, O)
        got = ops_pm.wino4_conv(x, d["u"], d["scale"], d["shift"], act=ops.ACT_RELU, residual=d["res"], out=out, form=form)
        assert got.data_ptr() == out.data_ptr()
        assert bool(torch.isnan(obuf[:pad]).all()) and bool(torch.isnan(obuf[pad + no:]).all())       # the neighbours stay NaN
        assert not bool(torch.isnan(out).any())                                                        # the NaNs around x do not leak in
        again = ops_pm.wino4_conv(d["x"], d["u"], d["scale"], d["shift"], act=ops.ACT_RELU, residual=d["res"], form=form)
        assert torch.equal(out, again)                                                                 # two runs, equal bits


def test_host_checks(device, data):
    d = data[(1, 4, 4, 64, 64)]
    lib = __import__("ffb6d_amd._lib", fromlist=["load"]).load()
    out = torch.empty(1, 4, 4, 64, device=device)
    with pytest.raises(Exception, match="alias"):
        ops_pm.wino4_conv(d["x"], d["u"], d["scale"], d["shift"], residual=out, out=out)
    with pytest.raises(Exception, match="input channels"):                                    # C not in the domain
        ops_pm.wino4_conv(torch.zeros(1, 4, 4, 32, device=device), torch.zeros(36, 64, 32, device=device), d["scale"], d["shift"])
    with pytest.raises(Exception, match="aligned"):
        ops_pm.wino4_conv(d["x"], d["u"], torch.ones(68, device=device)[1:65], d["shift"])
    # a 2 GiB operand by shape arithmetic only: 8 x 1024 x 1024 x 64 floats; refused before any pointer is read
    p = d["x"].data_ptr()
    rc = lib.ffb6d_wino4_conv_f32(p, p, p, p, None, None, None, out.data_ptr(), 8, 1024, 1024, 64, 64, 1, 0.0, 0, None)
    assert rc != 0


def test_forward_with_the_form_on_agrees_with_off_and_repeats_its_bits(device, monkeypatch):
    """B = 1, 240 x 320 as in tests/test_winograd4_gpu.py: 14 layers take the fused kernel (6 on 60 x 80, 8 on 30 x 40); on against off
    <= HOT_TOL on all 17 tensors; measured worst 1.9e-6 (pred_rgbd_segs)."""
    config, bs, n_pts, h, w, n_cls = 7, 1, 1024, 240, 320, 5
    with open(os.path.join(GOLDEN, "state_dict_keys.json")) as fh:
        shapes = json.load(fh)
    net = M.FFB6D(n_classes=n_cls, n_pts=n_pts)
    net.load_state_dict(synth.synth_state_dict_from_shapes(shapes, seed=0, n_classes=n_cls))
    net = net.to(device).eval()
    inputs = pyramid.frames_to_device(synth.make_batch(config, bs, n_points=n_pts, height=h, width=w), device)
    calls = []
    real = ops_pm.wino4_conv
    monkeypatch.setattr(ops_pm, "wino4_conv", lambda x, u, *a, **k: (calls.append(tuple(x.shape) + (u.shape[1],)), real(x, u, *a, **k))[1])

    def run(on):
        monkeypatch.setattr(forward_pm, "TRUNK_WINOGRAD_FUSED", on)
        calls.clear()
        taps = {}
        with torch.no_grad():
            ep = dict(net(inputs, taps=taps))
        assert len(taps) == 14
        ep.update(taps)
        return {k: v.clone() for k, v in ep.items() if torch.is_tensor(v) and v.is_floating_point()}

    off = run(False)
    assert not calls
    on = run(True)
    assert sorted(calls) == sorted([(1, 60, 80, 64, 64)] * 6 + [(1, 30, 40, 128, 128)] * 7 + [(1, 30, 40, 128, 256)])
    assert len(off) == 17 and sorted(on) == sorted(off)
    worst = 0.0
    for k in sorted(off):
        err = rel(on[k], off[k])
        print(k, "fused form on against off: max err / range %.2e" % err)
        worst = max(worst, err)
        assert err <= HOT_TOL, k
    print("worst %.2e" % worst)
    # the converted layers repeat their bits: blocks whose two convolutions both take the kernel, run twice on the same input
    blocks = [m for m in net.modules() if isinstance(m, M.ResBlock) and m.downsample is None and m.conv1.in_channels <= 128]
    assert len(blocks) == 6
    for rb in blocks:
        x = torch.randn(1, 30, 40, rb.conv1.in_channels, device=device)
        calls.clear()
        with torch.no_grad():
            a, b = forward_pm.res_block(rb, x), forward_pm.res_block(rb, x)
        assert torch.equal(a, b) and len(calls) == 4
