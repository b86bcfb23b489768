"""The operand ring of the split-bf16 GEMM form (ffb6d_amd/csrc/mlp_pm_split.hip): two 32-k slots, W requested one step ahead by
LDS-DMA, X two steps ahead in registers, counted waits and one bare barrier per step.

Shapes: rows 257, cout 260 (three point tiles, two channel tiles, both ragged); K = 64, 96, ... 32 x (2 x ring depth + 3) = 224, so that
start-up, steady state, wrap-around and drain (an even and an odd number of steps: the loop's half turn) each occur with both slots.
Bars: float64 at 1e-5 of range (test_split_gemm_gpu._check), equal bits between runs around a launch on other operands, and values
equal to the unpadded launch when W and X are zero-padded along K -- a slot read before it landed or after it was overwritten gives
another number.  Conventions (NaN guard columns on every operand and beside `out`) as tests/test_split_gemm_gpu.py."""
import pytest
import torch

from ffb6d_amd import ops_pm
import test_split_gemm_gpu as base

pytestmark = pytest.mark.gpu

RING = 2                                              # slots of 32 k (SP_NS in the kernel)
KS = list(range(64, 32 * (2 * RING + 3) + 1, 32))
ROWS, COUT = 257, 260


def _case(K):
    return base._operands(ROWS, COUT, K, True, None, seed=1000 + K)


def _dirty(device):
    """a launch on other operands: other K, large values in every slot of the ring"""
    gen = torch.Generator().manual_seed(77)
    x = (1e3 * torch.randn(300, 160, generator=gen)).to(device)
    w = (1e3 * torch.randn(264, 160, generator=gen)).to(device)
    ops_pm.mlp(x, w, None, 0, tile_hint=ops_pm.SPLIT_FORM)


@pytest.mark.parametrize("K", KS)
def test_every_ring_phase_against_float64_and_across_dirty_lds(device, K):
    o = _case(K)
    got, wide = base._run(o, 1, device)
    got = got.clone()
    base._check(got, base._want64(o, 1), f"ring K={K}")
    assert bool(torch.isnan(wide[..., :base.LEFT]).all() and torch.isnan(wide[..., base.LEFT + COUT:]).all())
    _dirty(device)
    again, _ = base._run(o, 1, device)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), (K, "bits differ after a launch on other operands")


@pytest.mark.parametrize("K", KS)
def test_zero_padding_along_k_leaves_every_value(device, K):
    o = _case(K)
    want, _ = base._run(o, 1, device)
    want = want + 0.0                                 # (-0 may become +0: values, not bits)
    for pad in (32, 64, 96):
        p = dict(o)
        p["x"] = torch.cat([o["x"], torch.zeros(o["B"], o["P"], pad)], dim=-1)
        p["w"] = torch.cat([o["w"], torch.zeros(COUT, pad)], dim=-1)
        got, _ = base._run(p, 1, device)
        assert torch.equal(got + 0.0, want), (K, pad, float((got - want).abs().max()))


@pytest.mark.parametrize("R", [128, 384])
@pytest.mark.parametrize("K", [64, 96])
def test_batched_entry_carries_the_bits_of_separate_launches(device, R, K):
    G = 36
    gen = torch.Generator().manual_seed(G * R + K)
    x = torch.randn(G, R, K, generator=gen).to(device)
    w = (torch.randn(G, 256, K, generator=gen) / K ** 0.5).to(device)
    got = ops_pm.mlp_batched(x, w, tile_hint=ops_pm.SPLIT_FORM, w_split=ops_pm.split_weight(w))
    base._check(got, torch.einsum("grk,gck->grc", x.double().cpu(), w.double().cpu()), f"batched {G}x{R}x{K}")
    for g in range(G):
        sep = ops_pm.mlp(x[g], w[g], tile_hint=ops_pm.SPLIT_FORM)
        assert torch.equal(got[g].view(torch.int32), sep.view(torch.int32)), g
