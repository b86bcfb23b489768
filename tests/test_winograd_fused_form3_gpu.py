"""Form 3 of the fused Winograd F(4x4,3x3) convolution on the device (csrc/winograd_fused.h: 4 waves x 16 tiles x 64 output channels
within 256 registers, two workgroups per CU): the same bits as form 1 for every residual form and activation, the whole operator
against float64, what it may and may not touch, the host check of the form number, and which form the automatic choice takes.

Shapes: the seven of tests/test_winograd_fused_gpu.py (one tile with 15 idle slots, a map narrower than a window, a partial last block
crossing a frame boundary, W % 4 = 3, exact blocks, 144 tiles, four channel blocks) and
    (1,  8,  8,  64 -> 128)   two 32-channel chunks, two channel blocks"""
import pytest
import torch
import torch.nn.functional as F

import winograd4_ref as w4
from ffb6d_amd import ops, ops_pm

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 4, 64, 64), (1, 5, 3, 128, 128), (2, 13, 18, 64, 64), (2, 9, 43, 64, 64), (1, 16, 16, 128, 128), (3, 23, 30, 128, 128),
          (2, 13, 18, 128, 256), (1, 8, 8, 64, 128)]
CONV_TOL = 1e-5         # the project's per-operator bar (tests/test_winograd_fused_gpu.py)


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


def residual_forms(d):
    return (("no residual", {}, None),
            ("residual", {"residual": d["res"]}, d["res"].double()),
            ("projected residual", {"residual": d["res"], "res_affine": (d["rscale"], d["rshift"])},
             d["res"].double() * d["rscale"].double() + d["rshift"].double()))


@pytest.mark.parametrize("shape", SHAPES)
def test_form3_gives_the_bits_of_form1(device, data, shape):
    """Every residual form with ReLU, and every activation with the plain residual: torch.equal."""
    d = data[shape]
    cases = [(ops.ACT_RELU, kw) for _, kw, _ in residual_forms(d)]
    cases += [(act, {"residual": d["res"]}) for act in (ops.ACT_NONE, ops.ACT_LEAKY)]
    cases += [(act, {}) for act in (ops.ACT_NONE, ops.ACT_LEAKY)]
    for act, kw in cases:
        one = ops_pm.wino4_conv(d["x"], d["u"], d["scale"], d["shift"], act=act, slope=0.2, form=1, **kw)
        three = ops_pm.wino4_conv(d["x"], d["u"], d["scale"], d["shift"], act=act, slope=0.2, form=3, **kw)
        assert not bool(torch.isnan(three).any())
        assert torch.equal(three, one), (act, sorted(kw))


@pytest.mark.parametrize("shape", SHAPES)
def test_form3_against_float64(device, data, shape):
    d = data[shape]
    for what, kw, add in residual_forms(d):
        want = d["y64"] * d["scale"].double() + d["shift"].double()
        want = torch.relu(want if add is None else want + add)
        got = ops_pm.wino4_conv(d["x"], d["u"], d["scale"], d["shift"], act=ops.ACT_RELU, form=3, **kw)
        err = rel(got, want)
        print(shape, "form 3, fused F(4x4) convolution + BN +", what, "+ ReLU against float64: max err / range %.2e" % err)
        assert got.shape == want.shape and err <= CONV_TOL


@pytest.mark.parametrize("shape", SHAPES)
def test_form3_writes_only_its_output_reads_only_its_map_and_repeats_its_bits(device, data, shape):
    B, H, W, C, O = shape
    d = data[shape]
    nx, no, pad = B * H * W * C, B * H * W * O, 4096
    xbuf = torch.full((nx + 2 * pad,), float("nan"), device=device)
    xbuf[pad:pad + nx] = d["x"].reshape(-1)
    x = xbuf[pad:pad + nx].view(B, H, W, C)
    obuf = torch.full((no + 2 * pad,), float("nan"), device=device)
    out = obuf[pad:pad + no].view(B, H, W, O)
    got = ops_pm.wino4_conv(x, d["u"], d["scale"], d["shift"], act=ops.ACT_RELU, residual=d["res"], out=out, form=3)
    assert got.data_ptr() == out.data_ptr()
    assert bool(torch.isnan(obuf[:pad]).all()) and bool(torch.isnan(obuf[pad + no:]).all())       # the neighbours stay NaN
    assert not bool(torch.isnan(out).any())                                                        # the NaNs around x do not leak in
    again = ops_pm.wino4_conv(d["x"], d["u"], d["scale"], d["shift"], act=ops.ACT_RELU, residual=d["res"], form=3)
    assert torch.equal(out, again)                                                                 # two runs, equal bits


def test_form_number_is_checked(device, data):
    d = data[(1, 4, 4, 64, 64)]
    with pytest.raises(Exception, match="form must be"):
        ops_pm.wino4_conv(d["x"], d["u"], d["scale"], d["shift"], form=4)
    with pytest.raises(Exception, match="form must be"):
        ops_pm.wino4_conv(d["x"], d["u"], d["scale"], d["shift"], form=-1)


@pytest.mark.parametrize("shape", SHAPES)
def test_automatic_form_is_the_one_the_width_table_names(device, data, shape):
    d = data[shape]
    form = ops_pm.wino4_conv_form(shape[3], shape[4])
    assert form in (1, 3)
    auto = ops_pm.wino4_conv(d["x"], d["u"], d["scale"], d["shift"], act=ops.ACT_RELU, residual=d["res"])
    named = ops_pm.wino4_conv(d["x"], d["u"], d["scale"], d["shift"], act=ops.ACT_RELU, residual=d["res"], form=form)
    assert torch.equal(auto, named)
