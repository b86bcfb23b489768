"""The fused Winograd F(4x4,3x3) convolution of the narrow trunk layers (csrc/winograd_fused.h), the parts that need no GPU: the kernel
on the SIMT-emulated library against the float64 restatement (tests/winograd4_ref.py), what converting the 64- and 128-wide layers
costs in accuracy through the whole network (measured on the oracle), and which form every trunk convolution takes."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import winograd4_ref as w4
from conftest import GOLDEN
from ffb6d_amd import forward_pm, model, ops, ops_pm, synth

CONV_TOL = 1e-5         # the project's per-operator bar; the fp32 restatement alone measures <= 3.4e-6 on these shapes
EMU_SHAPES = [(1, 4, 4, 64, 64),        # one tile, 15 idle tile slots
              (1, 5, 3, 128, 128),      # map narrower than a window, two K chunks, two channel blocks
              (2, 13, 18, 64, 64),      # 40 tiles: partial last block, H % 4 = 1, W % 4 = 2, a block crossing the frame boundary
              (1, 16, 16, 128, 128)]    # exact blocks


def rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


def problem(shape):
    B, H, W, C, O = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(O, C, 3, 3, generator=g) / (9 * C) ** .5
    scale, shift = torch.rand(O, generator=g) + .5, .1 * torch.randn(O, generator=g)
    rscale, rshift = torch.rand(O, generator=g) + .5, .1 * torch.randn(O, generator=g)
    res = torch.randn(B, H, W, O, generator=g)
    y64 = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)
    return x, w, scale, shift, rscale, rshift, res, y64


def glue64(y, scale, shift, act, slope, res=None, raff=None):
    v = y * scale.double() + shift.double()
    if res is not None:
        v = v + (res.double() * raff[0].double() + raff[1].double() if raff is not None else res.double())
    return v if act == ops.ACT_NONE else torch.where(v > 0, v, (0.0 if act == ops.ACT_RELU else slope) * v)


@pytest.mark.parametrize("shape", EMU_SHAPES)
def test_kernel_on_the_emulator_matches_float64(emu, shape):
    """Both workgroup shapes of the kernel; plain convolution, then every activation with no residual, a residual and a projected residual.
    The restatement of tests/winograd4_ref.py in float64 equals F.conv2d to 1e-12 (tests/test_winograd4_cpu.py), so F.conv2d in float64 is
    the reference here."""
    x, w, scale, shift, rscale, rshift, res, y64 = problem(shape)
    O = shape[4]
    assert float((w4.conv(x.double(), w.double()) - y64).abs().max()) <= 1e-12
    u = forward_pm.wino4_filter(w)
    assert torch.equal(u, w4.filter_transform(w))
    worst = 0.0
    for form in (1, 2):
        got = ops_pm.wino4_conv(x, u, torch.ones(O), torch.zeros(O), form=form)
        assert got.shape == y64.shape and not bool(torch.isnan(got).any())
        err = rel(got, y64)
        print(shape, "form", form, "convolution: max err / range %.2e" % err)
        worst = max(worst, err)
        assert err <= CONV_TOL
    cases = [(act, kw) for act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY)
             for kw in ({}, {"residual": res}, {"residual": res, "res_affine": (rscale, rshift)})]
    for n, (act, kw) in enumerate(cases):
        got = ops_pm.wino4_conv(x, u, scale, shift, act=act, slope=0.2, form=1 + n % 2, **kw)
        want = glue64(y64, scale, shift, act, 0.2, kw.get("residual"), kw.get("res_affine"))
        err = rel(got, want)
        print(shape, "act", act, sorted(kw), ": max err / range %.2e" % err)
        worst = max(worst, err)
        assert err <= CONV_TOL
        if act == ops.ACT_RELU:
            assert bool((got >= 0).all()) and bool((got == 0).any())
    print(shape, "worst %.2e" % worst)


def test_host_checks_reject_what_the_kernel_is_not_built_for(emu):
    x, w, scale, shift, _, _, res, _ = problem((1, 4, 4, 64, 64))
    u = forward_pm.wino4_filter(w)
    out = torch.empty(1, 4, 4, 64)
    with pytest.raises(Exception, match="alias"):
        ops_pm.wino4_conv(x, u, scale, shift, residual=out, out=out)
    with pytest.raises(Exception, match="alias"):
        ops_pm.wino4_conv(x, u, scale, shift, out=x)
    with pytest.raises(Exception, match="input channels"):
        ops_pm.wino4_conv(torch.zeros(1, 4, 4, 32), torch.zeros(36, 64, 32), scale, shift)
    with pytest.raises(Exception, match="input channels"):
        ops_pm.wino4_conv(x, torch.zeros(36, 96, 64), torch.ones(96), torch.zeros(96))
    with pytest.raises(Exception, match="aligned"):
        ops_pm.wino4_conv(x, u, torch.ones(68)[1:65], shift)


class _Functional:
    """torch.nn.functional with conv2d replaced (handed to oracle.forward_ref as its `F`)"""

    def __init__(self, conv2d):
        self.conv2d = conv2d

    def __getattr__(self, name):
        return getattr(F, name)


def test_winograd4_on_every_trunk_layer_from_64_channels_stays_at_the_reordering_floor(monkeypatch):
    """tests/test_winograd4_cpu.py's network test with the condition widened to Cin >= 64 on every map (the trunk maps are 30 x 40 and
    15 x 20 at this geometry): oracle/forward_ref.py in fp32 with those 3x3 / stride 1 / padding 1 convolutions computed by the F(4x4) restatement against
    the unmodified fp32 oracle, worst error over the three outputs and the 14 stage taps relative to each tensor's range <= 5e-6 (the
    bound and its reasoning: tests/test_winograd_cpu.py).  Measured when this test was written: see the worst figure the test prints (the proposal measured 2.28e-6); 34 convolutions
    are converted, 14 of them the narrow trunk layers the fused kernel takes."""
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
        if w.dim() == 4 and tuple(w.shape[2:]) == (3, 3) and s == 1 and p == 1 and dilation == 1 and groups == 1 and w.shape[1] >= 64:
            converted.append(tuple(w.shape) + tuple(x.shape[2:]))
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
    trunk = [s for s in converted if s[4:] in ((30, 40), (15, 20))]
    narrow = [s[:2] for s in trunk if s[1] < 256]
    print("converted", len(converted), "on the trunk maps", len(trunk), "of which narrow", len(narrow), "elsewhere", sorted(set(converted) - set(trunk)))
    assert len(converted) >= 33 and len(narrow) == 14 and len([s for s in trunk if s[1] >= 256]) >= 17
    assert sorted(narrow) == sorted([(64, 64)] * 6 + [(128, 128)] * 7 + [(256, 128)])
    assert sorted(direct) == sorted(wino) and len(direct) == 17
    worst = 0.0
    for k in sorted(direct):
        err = float((wino[k] - direct[k]).abs().max() / direct[k].abs().max())
        print(k, "winograd F(4x4) from 64 channels vs direct, max err / range %.2e" % err)
        worst = max(worst, err)
    print("worst %.2e over %d converted convolutions" % (worst, len(converted)))
    assert worst <= 5e-6


def trunk_forms(net, B, H, W, dtype=torch.float32):
    """[(Cin, Cout, h, w, form)] of the two convolutions of every residual block of the trunk on a B x H x W frame (meta tensors: only
    shapes and dtypes decide)"""
    out = []
    h, w = H // 4, W // 4                                  # after the stride-2 stem and the max-pool
    for rb in [m for m in net.modules() if isinstance(m, model.ResBlock)]:
        for c in (rb.conv1, rb.conv2):
            x = torch.empty(B, h, w, c.in_channels, dtype=dtype, device="meta")
            out.append((c.in_channels, c.out_channels, h, w, forward_pm.trunk_conv_form(c, x)))
            h, w = (h - 1) // c.stride[0] + 1, (w - 1) // c.stride[0] + 1
    return out


def count(forms, form, cin=None, cout=None):
    return sum(1 for f in forms if f[4] == form and (cin is None or f[:2] == (cin, cout)))


def test_routing_of_every_trunk_convolution(monkeypatch):
    """Benchmark geometry (8 x 480 x 640) and the two small test geometries: the six 64 -> 64 layers, the seven 128 -> 128 layers and the
    128 -> 256 layer take the fused kernel, the seventeen wide layers the three-kernel path, the two stride-2 heads MIOpen; bf16 takes
    neither Winograd form; the switch off restores the parent's choice."""
    net = model.FFB6D(n_classes=5, n_pts=1024)
    assert forward_pm.TRUNK_WINOGRAD_FUSED is True
    for B, H, W in ((8, 480, 640), (1, 240, 320), (2, 120, 160)):
        forms = trunk_forms(net, B, H, W)
        assert len(forms) == 32
        assert count(forms, "fused") == 14 and count(forms, "wino") == 17 and count(forms, "miopen") == 1
        assert count(forms, "fused", 64, 64) == 6 and count(forms, "fused", 128, 128) == 7 and count(forms, "fused", 128, 256) == 1
        assert [f[:2] for f in forms if f[4] == "miopen"] == [(64, 128)]                     # stride 2
        assert {f[2:4] for f in forms if f[:2] == (64, 64)} == {(H // 4, W // 4)}
        assert {f[2:4] for f in forms if f[0] >= 128} == {(H // 8, W // 8)}
        assert all(f[4] == "miopen" for f in trunk_forms(net, B, H, W, torch.bfloat16))
    on = trunk_forms(net, 8, 480, 640)
    monkeypatch.setattr(forward_pm, "TRUNK_WINOGRAD_FUSED", False)
    off = trunk_forms(net, 8, 480, 640)
    assert count(off, "fused") == 0 and count(off, "wino") == 17 and count(off, "miopen") == 15
    assert [f for f in off if f[4] == "wino"] == [f for f in on if f[4] == "wino"]
    monkeypatch.setattr(forward_pm, "TRUNK_WINOGRAD_FUSED", True)
    monkeypatch.setattr(forward_pm, "TRUNK_WINOGRAD_FUSED_WIDTHS", frozenset({(64, 64)}))      # the per-width rule
    assert count(trunk_forms(net, 8, 480, 640), "fused") == 6
    monkeypatch.setattr(forward_pm, "TRUNK_WINOGRAD", False)
    assert all(f[4] == "miopen" for f in trunk_forms(net, 8, 480, 640))
    for bad in (torch.nn.Conv2d(64, 64, 3, 2, 1, bias=False), torch.nn.Conv2d(64, 64, 3, 1, 1, bias=True),
                torch.nn.Conv2d(64, 64, 1, 1, 0, bias=False), torch.nn.Conv2d(64, 64, 3, 1, 2, dilation=2, bias=False),
                torch.nn.Conv2d(64, 64, 3, 1, 1, groups=2, bias=False), torch.nn.Conv2d(64, 32, 3, 1, 1, bias=False)):
        monkeypatch.setattr(forward_pm, "TRUNK_WINOGRAD", True)
        assert not forward_pm.wino_fused_ok(bad, torch.empty(1, 8, 8, 64, device="meta"))
    assert not forward_pm.wino_fused_ok(torch.nn.Conv2d(64, 64, 3, 1, 1, bias=False), torch.empty(8, 1200, 1600, 64, device="meta"))   # 2 GiB
