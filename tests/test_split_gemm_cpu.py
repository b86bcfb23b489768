"""The arithmetic of the split-bf16 GEMM form (ffb6d_amd/csrc/mlp_pm_split.hip) on the CPU restatement tests/split_gemm_ref.py:
the representation a = a0 + a1 + a2, the truncation bound of the six kept terms, and the restatement's fp32 error against the
project's GEMM bar.  The kernel itself runs on the device only (tests/test_split_gemm_gpu.py)."""
import pytest
import torch

import split_gemm_ref as ref


def _f32_from_bits(bits):
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


def _every_exponent(gen):
    """finite fp32 of every biased exponent 0..254 and both signs: random mantissas plus the mantissas around the bf16 rounding
    boundaries of each part (low 16 bits 0x7fff / 0x8000 / 0x8001: just under, on and over a tie of a0; low 8 bits the same for a1)"""
    edge = [0x000000, 0x000001, 0x007FFF, 0x008000, 0x008001, 0x00FFFF, 0x017FFF, 0x018000, 0x018001, 0x7FFFFF, 0x7F7FFF, 0x7F8000,
            0x00007F, 0x000080, 0x000081, 0x00017F, 0x000180, 0x000181, 0x7FFF7F, 0x7FFF80, 0x7FFF81, 0x3FFFFF, 0x400000, 0x555555]
    bits = []
    for e in range(0, 255):
        man = edge + [int(v) for v in torch.randint(0, 1 << 23, (40,), generator=gen)]
        for m in man:
            for s in (0, 1):
                bits.append((s << 31) | (e << 23) | m)
    a = _f32_from_bits(bits)
    return a[a.abs() <= ref.BF16_MAX]                 # above the largest finite bf16 the first rounding overflows: outside the domain


def test_three_bf16_parts_represent_every_finite_fp32_exactly():
    """a0 + a1 + a2 == a for every finite fp32 with |a| >= 2^-110 (and for 0), whatever its mantissa: ties, values just under a
    rounding boundary, residuals that are subnormal bf16 numbers.  Below 2^-110 the lowest bits of a fall under the smallest bf16
    subnormal (2^-133) and the sum misses a by less than that.  The truncation bound of the form rests on this."""
    a = _every_exponent(torch.Generator().manual_seed(1))
    a0, a1, a2 = ref.split3(a)
    for part in (a0, a1, a2):
        assert bool(torch.isfinite(part).all())
        assert torch.equal(part.bfloat16().float(), part)          # each part IS a bf16 number
    total = a0.double() + a1.double() + a2.double()                # exact in float64
    big = (a.abs() >= ref.EXACT_FROM) | (a == 0)
    assert int(big.sum()) > 30000 and int((~big).sum()) > 1000
    assert torch.equal(total[big], a.double()[big])
    assert float((total[~big] - a.double()[~big]).abs().max()) < 2.0 ** -133
    # the parts shrink as the bound assumes: |a - a0| <= 2^-8 |a|, |a - a0 - a1| <= 2^-16 |a|  (half an ulp of 8 significant bits = 2^-9)
    ad = a.double()[big]
    assert bool(((ad - a0.double()[big]).abs() <= 2.0 ** -8 * ad.abs()).all())
    assert bool(((ad - a0.double()[big] - a1.double()[big]).abs() <= 2.0 ** -16 * ad.abs()).all())


def test_infinite_and_oversized_inputs_are_outside_the_domain():
    """what the header states: +-inf gives NaN parts (inf - inf), a finite value above the largest bf16 overflows on rounding"""
    a0, a1, _ = ref.split3(torch.tensor([float("inf"), 3.4e38], dtype=torch.float32))
    assert bool(torch.isinf(a0).all()) and bool(torch.isnan(a1[0]))


SHAPES = [(256, "randn"), (256, "relu"), (1024, "lognormal"), (1024, "relu"), (4608, "randn"), (4608, "lognormal")]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for K, kind in SHAPES:
        gen = torch.Generator().manual_seed(K + len(kind))
        x = ref.data(kind, (48, K), gen)
        w = ref.data("randn", (40, K), gen) * (1.0 / K ** 0.5)
        out[(K, kind)] = (x, w, x.double() @ w.double().T, x.double().abs() @ w.double().abs().T)
    return out


@pytest.mark.parametrize("K,kind", SHAPES)
def test_six_terms_truncate_below_two_to_minus_23(cases, K, kind):
    """the six kept products summed exactly miss W x by at most 2^-23 sum |w||x|: the dropped terms are a1 b2 + a2 b1 + a2 b2 with
    |a1| <= 2^-8 |a|, |a2| <= 2^-16 |a| (the representation test), so <= (2^-24 + 2^-24 + 2^-32) |a||b| per product"""
    x, w, want, mag = cases[(K, kind)]
    err = (ref.six_terms_f64(x, w) - want).abs()
    worst = float((err / mag.clamp_min(1e-300)).max())
    print(f"K={K} {kind}: truncation / sum|w||x| = {worst:.3e}, / range = {float(err.max()) / float(want.abs().max()):.3e}")
    assert bool((err <= 2.0 ** -23 * mag).all()), worst


@pytest.mark.parametrize("K,kind", SHAPES)
def test_restatement_in_fp32_keeps_the_gemm_bar(cases, K, kind):
    """the form as the kernel accumulates it (fp32, documented order) against float64: within 1e-5 max|want|, the per-operator bar of
    tests/test_pm_forms_gpu.py; its ratio to the error of a plain fp32 matmul on the same data is printed (-s)"""
    x, w, want, _ = cases[(K, kind)]
    rng = float(want.abs().max())
    err = float((ref.gemm(x, w).double() - want).abs().max())
    plain = float(((x @ w.T).double() - want).abs().max())
    print(f"K={K} {kind}: split {err / rng:.3e} of range, plain fp32 matmul {plain / rng:.3e}, ratio {err / max(plain, 1e-300):.2f}")
    assert err <= 1e-5 * rng, (err, rng)


def test_epilogue_restatement_matches_torch():
    acc = torch.randn(5, 8)
    b, y = torch.randn(8), torch.randn(5, 8)
    assert torch.equal(ref.epilogue(acc, b, y, 1), torch.relu((acc + b) + y))
    assert torch.equal(ref.epilogue(acc, None, None, 0), acc)
    assert torch.allclose(ref.epilogue(acc, b, None, 2), torch.nn.functional.leaky_relu(acc + b, 0.2), rtol=0, atol=1e-7)
    assert ref.ulps(torch.tensor([1.0, -1.0]), torch.tensor([1.0 + 2.0 ** -23, -1.0])) == 1
