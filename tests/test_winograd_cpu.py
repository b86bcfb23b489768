"""Winograd F(2x2,3x3) for the wide trunk convolutions, the parts that need no GPU: the plain-torch restatement of the three transforms
(tests/winograd_ref.py, the specification of csrc/winograd.h) against F.conv2d, the cached filter transform, and what the method
costs in accuracy through the whole network, measured on the oracle."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import winograd_ref as wr
from conftest import GOLDEN
from ffb6d_amd import forward_pm, synth


@pytest.mark.parametrize("shape", [(2, 6, 8), (2, 7, 8), (2, 6, 9), (2, 5, 7), (1, 1, 1)])
def test_restatement_equals_conv2d_in_float64(shape):
    B, H, W = shape
    g = torch.Generator().manual_seed(H * 16 + W)
    x = torch.randn(B, H, W, 5, dtype=torch.float64, generator=g)
    w = torch.randn(3, 5, 3, 3, dtype=torch.float64, generator=g)
    want = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    got = wr.conv(x, w)
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    print(shape, "max abs err", err)
    assert err <= 1e-12


def test_filter_transform_of_the_package_is_the_restatement_and_follows_weight_edits():
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(8, 12, 3, 1, 1, bias=False)
    u0 = forward_pm.wino_weights(conv)
    assert u0.dtype == torch.float32 and u0.shape == (16, 12, 8) and u0.is_contiguous()
    assert torch.equal(u0, wr.filter_transform(conv.weight.detach()))
    assert forward_pm.wino_weights(conv) is u0                       # cached
    with torch.no_grad():
        conv.weight.mul_(1.5)                                        # in-place edit: the version counter moves
    u1 = forward_pm.wino_weights(conv)
    assert u1 is not u0 and not torch.equal(u1, u0)
    assert torch.equal(u1, wr.filter_transform(conv.weight.detach()))


class _Functional:
    """torch.nn.functional with conv2d replaced (handed to oracle.forward_ref as its `F`)"""

    def __init__(self, conv2d):
        self.conv2d = conv2d

    def __getattr__(self, name):
        return getattr(F, name)


def test_winograd_on_the_wide_layers_stays_at_the_reordering_floor(monkeypatch):
    """oracle/forward_ref.py in fp32 at the smallest test geometry with every 3x3 / stride 1 / padding 1 convolution of Cin >= 256
    computed by the restatement (filter transform in fp64, rounded once) against the unmodified fp32 oracle: the maximum over the
    three outputs and the 14 stage taps, relative to each tensor's range, must stay <= 5e-6 -- 2.0e-6 was measured when the bound was
    set (the same figure as summing the nine taps of the direct convolution in another order; 2.6e-6 with this file's einsum); 2.5x is
    the margin for another BLAS; HOT_TOL is 1e-5."""
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
        if w.dim() == 4 and tuple(w.shape[2:]) == (3, 3) and s == 1 and p == 1 and dilation == 1 and groups == 1 and w.shape[1] >= 256:
            converted.append(tuple(w.shape))
            y = wr.conv(x.permute(0, 2, 3, 1), w).permute(0, 3, 1, 2)
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
        print(k, "winograd vs direct, max err / range %.2e" % err)
        worst = max(worst, err)
    print("worst %.2e over %d converted convolutions" % (worst, len(converted)))
    assert worst <= 5e-6
