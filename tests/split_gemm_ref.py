"""CPU restatement of the split-bf16 GEMM form (ffb6d_amd/csrc/mlp_pm_split.hip) in torch: the three-way bf16 split of an fp32 operand,
the six products in the documented order, fp32 accumulation.

One v_mfma_f32_32x32x16_bf16 is restated as `acc = fp32(acc + exact sum of its 16 products)`: the products of bf16 numbers are exact in
fp32, their sum of 16 and the accumulator are added in float64 and rounded once.  How the instruction rounds inside is not documented;
the device test measures how far its bits are from this idealisation."""
import torch

# (w part, x part) per 16 k, in the order the kernel issues them: small terms first
TERMS = ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0))
BF16_MAX = float(torch.finfo(torch.bfloat16).max)
# a0 + a1 + a2 == a exactly while the lowest set bit of a is representable in a bf16 (>= 2^-133): every fp32 with |a| >= 2^-110
EXACT_FROM = 2.0 ** -110


def split3(a):
    """fp32 tensor -> (a0, a1, a2) as fp32 tensors holding bf16 values: a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1),
    round to nearest even, the subtractions in fp32 (they are exact)"""
    assert a.dtype == torch.float32
    a0 = a.bfloat16().float()
    r1 = a - a0
    a1 = r1.bfloat16().float()
    a2 = (r1 - a1).bfloat16().float()
    return a0, a1, a2


def six_terms_f64(x, w):
    """[R,K] x [C,K] -> [R,C] float64: the six kept products summed without rounding (the truncation error alone)"""
    xs = [t.double() for t in split3(x)]
    ws = [t.double() for t in split3(w)]
    out = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float64)
    for i, j in TERMS:
        out += xs[j] @ ws[i].T
    return out


def gemm(x, w):
    """[R,K] x [C,K] -> [R,C] float32 as the kernel accumulates it: per 16 k the six terms in TERMS order, one rounding per MFMA"""
    R, K = x.shape
    assert K % 16 == 0
    xs = [t.double() for t in split3(x)]
    ws = [t.double() for t in split3(w)]
    acc = torch.zeros(R, w.shape[0], dtype=torch.float32)
    for k0 in range(0, K, 16):
        for i, j in TERMS:
            acc = (acc.double() + xs[j][:, k0:k0 + 16] @ ws[i][:, k0:k0 + 16].T).float()
    return acc


def epilogue(acc, bias=None, extra=None, act=0):
    """(acc + bias) + extra in fp32, then identity / ReLU / LeakyReLU(0.2) as max(v, slope * v) (csrc/mlp_pm_common.h: pm_epilogue)"""
    v = acc
    if bias is not None:
        v = v + bias
    if extra is not None:
        v = v + extra
    slope = (1.0, 0.0, 0.2)[act]
    return torch.maximum(v, torch.tensor(slope, dtype=torch.float32) * v)


def ulps(a, b):
    """largest distance of two fp32 tensors in units in the last place (of the ordered integer representation)"""
    def key(t):
        i = t.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((key(a) - key(b)).abs().max()) if a.numel() else 0


def data(kind, shape, gen):
    """the operand distributions of the accuracy record: randn, ReLU-like (half zeros), log-normal scale per row"""
    t = torch.randn(shape, generator=gen)
    if kind == "relu":
        return t.clamp_min(0)
    if kind == "lognormal":
        return t * torch.exp(2.0 * torch.randn(shape[0], 1, generator=gen))
    return t
