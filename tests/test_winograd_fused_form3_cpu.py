"""Form 3 of the fused Winograd F(4x4,3x3) convolution (csrc/winograd_fused.h) on the SIMT-emulated library, as
tests/test_winograd_fused_cpu.py runs forms 1 and 2: the same bits as form 1, and the operator against float64."""
import pytest
import torch

from ffb6d_amd import forward_pm, ops, ops_pm
from test_winograd_fused_cpu import CONV_TOL, glue64, problem, rel

EMU_SHAPES = [(1, 4, 4, 64, 64),        # one tile, 15 idle tile slots; two 32-channel chunks
              (1, 5, 3, 128, 128),      # map narrower than a window, four chunks, two channel blocks
              (2, 13, 18, 64, 64),      # 40 tiles: partial last block, H % 4 = 1, W % 4 = 2, a block crossing the frame boundary
              (1, 8, 8, 64, 128)]       # two chunks, two channel blocks


@pytest.mark.parametrize("shape", EMU_SHAPES)
def test_form3_on_the_emulator_matches_form1_and_float64(emu, shape):
    x, w, scale, shift, rscale, rshift, res, y64 = problem(shape)
    u = forward_pm.wino4_filter(w)
    cases = [(act, kw) for act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY)
             for kw in ({}, {"residual": res}, {"residual": res, "res_affine": (rscale, rshift)})]
    worst = 0.0
    for act, kw in cases:
        one = ops_pm.wino4_conv(x, u, scale, shift, act=act, slope=0.2, form=1, **kw)
        three = ops_pm.wino4_conv(x, u, scale, shift, act=act, slope=0.2, form=3, **kw)
        assert not bool(torch.isnan(three).any())
        assert torch.equal(three, one), (act, sorted(kw))
        err = rel(three, glue64(y64, scale, shift, act, 0.2, kw.get("residual"), kw.get("res_affine")))
        worst = max(worst, err)
        assert err <= CONV_TOL
    print(shape, "form 3 worst max err / range %.2e" % worst)
    form = ops_pm.wino4_conv_form(shape[3], shape[4])
    assert form in (1, 3)
    assert torch.equal(ops_pm.wino4_conv(x, u, scale, shift, form=0), ops_pm.wino4_conv(x, u, scale, shift, form=form))
    with pytest.raises(Exception, match="form must be"):
        ops_pm.wino4_conv(x, u, scale, shift, form=4)
