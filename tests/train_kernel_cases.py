"""Cases, float64 references and bounds for the training-step kernels (csrc/train_rows.hip, csrc/train_ops.hip and the scatter they hand
to csrc/neighbour_ops.hip), shared by tests/test_train_kernels_gpu.py (device, or --emulate) and tests/test_train_kernels_emu_cpu.py.

Two kinds of case:

EXACT    operands are small integers or dyadic fractions: every float32 partial sum is exact in any order and the result is representable
         in the output type, so the kernel's output must equal the float64 reference bit for bit (`assert_exact`; no tolerance, no element
         excluded).  `exact_conditions` asserts the premises on the reference side: sum |terms| < 2^24 grid steps per output element, the
         result a whole number of grid steps, representable in the output type and, for bfloat16, at most 256 steps.

ROUNDED  operands are random reals already rounded to the operand type; the reference is float64 arithmetic on the same operands,
         written out (no autograd).  Per element, nothing excluded (`assert_rounded`):

             |got - want| <= half_ulp_out(want) + c * 2^-24 * A  (+ floor)

         half_ulp_out = half the spacing of the output type at |want| (2^(floor(log2|want|) - 8) for bfloat16, - 24 for float32): the one
         rounding of the store -- a truncating store misses it on about half of the elements.  A = the float64 sum of the absolute values
         of the element's terms (its conditioning: cancellation needs no exclusion).  c counts the float32 roundings on the way:
           * sums and products: derived from the operation count, stated at each `run_*` below;
           * paths with expf / logf / a division (att_pool_rows*, log_softmax_rows*): c = 4 x the largest ratio |torch_fp32 - float64| /
             (2^-24 A) that plain torch float32 on the CPU shows for the same formula on the same inputs (`torch_fp32_ratios`, recorded in
             MEASURED) -- the kernel may order its sums differently and use another expf, but an order of magnitude above ATen is a
             defect.  These bounds also carry the floor |g| (1 + |f|) 2^-126: float32 underflow of a softmax weight that float64 keeps.
         Nothing in a bound comes from the kernels' own output.

Every `run_*` drives the operator through its public Python entry, as the model does, and asserts through a log of the native entry points
(`call_log`) that the native code ran -- or, where the case is meant to take a fallback, that it did not."""
import contextlib
import zlib

import numpy as np
import torch

from ffb6d_amd import _lib, ops, ops_cl

F32, BF16 = torch.float32, torch.bfloat16
DTS = [F32, BF16]
U24 = 2.0 ** -24
TINY = 2.0 ** -126

# operator, output -> (largest ratio of torch float32 on the CPU over all cases of the tables below, rounded up to two decimals; c = 4 x that).
# Regenerate with `python tests/train_kernel_cases.py`; tests/test_train_kernels_emu_cpu.py checks that torch float32 itself meets c.
MEASURED = {
    ("att_pool", "out"): (4.75, 19.00),
    ("att_pool", "grad_feat"): (4.36, 17.44),
    ("att_pool", "grad_scores"): (2.31, 9.24),
    ("log_softmax", "out"): (5.34, 21.36),
    ("log_softmax", "grad"): (14.04, 56.16),
}


def gen(*key):
    """a generator seeded by the case itself: every builder below gives the same operands on every machine"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def ids(table):
    """readable pytest ids for the rows of a case table"""
    def word(v):
        if isinstance(v, (torch.dtype,)):
            return {F32: "f32", BF16: "bf16", torch.int32: "i32", torch.int64: "i64"}[v]
        if isinstance(v, tuple):
            return "x".join(word(e) for e in v)
        return {True: "y", False: "n"}.get(v, str(v)) if isinstance(v, bool) else str(v)
    return ["-".join(word(v) for v in row) for row in table]


def rows_of(x):
    """[B,C,*S] -> [B,prod(S),C] on the CPU in float64 (values only)"""
    B, C = x.shape[:2]
    return x.detach().cpu().double().reshape(B, C, -1).transpose(1, 2)


def as_cl_grad(rows, spatial):
    """[B,U,W] rows -> a [B,W,*spatial] view of them with channels_last strides (what a channels_last consumer hands back)"""
    B, U, W = rows.shape
    return rows.transpose(1, 2).reshape(B, W, *spatial)


@contextlib.contextmanager
def call_log(*names):
    """log[name] = the argument tuples of every call of that native entry point inside the block"""
    lib = _lib.load()
    saved = {n: getattr(lib, n) for n in names}
    log = {n: [] for n in names}
    try:
        for n, fn in saved.items():
            def logged(*a, _fn=fn, _n=n):
                log[_n].append(a)
                return _fn(*a)
            setattr(lib, n, logged)
        yield log
    finally:
        for n, fn in saved.items():
            setattr(lib, n, fn)


@contextlib.contextmanager
def aten_bilinear_backward_log():
    """calls of ATen's own bilinear backward, the fallback of ops.upsample_align"""
    ns, name = torch.ops.aten, "upsample_bilinear2d_backward"
    real = getattr(ns, name)
    calls = []

    def logged(*a, **kw):
        calls.append(a)
        return real(*a, **kw)
    setattr(ns, name, logged)
    try:
        yield calls
    finally:
        setattr(ns, name, real)


# ---------------------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------------------
def half_ulp(want, dt):
    """half the spacing of dtype dt at |want| (float64 tensor); below the smallest normal the spacing of the subnormals"""
    _, e = torch.frexp(want.abs())                                   # |want| = m 2^e with m in [0.5, 1): floor(log2 |want|) = e - 1
    e = torch.where(torch.isfinite(want) & (want != 0), e - 1, torch.full_like(e, -126)).clamp(min=-126)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double() - (8 if dt == BF16 else 24))


def as_f64(t):
    return t.detach().cpu().double()


def assert_exact(got, want, dt, what, signed_zero=False):
    assert got.dtype == dt, (what, got.dtype)
    got = as_f64(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (what, "NaN pattern")
    a, b = torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0)
    bad = a != b
    if signed_zero:
        bad |= torch.signbit(a) != torch.signbit(b)
    assert not bad.any(), (what, int(bad.sum()), "of", bad.numel(), "first", bad.nonzero()[0].tolist(),
                           float(a[bad][0]), float(b[bad][0]))


def exact_conditions(want, A, dt, grid=1.0):
    """the premises of an exact case, asserted on the reference"""
    fin = torch.nan_to_num(want, nan=0.0)
    steps = fin / grid
    assert float(torch.nan_to_num(A, nan=0.0).max()) / grid < 2 ** 24
    assert torch.equal(steps, steps.round())
    assert torch.equal(fin.to(dt).double(), fin)
    if dt == BF16:
        assert float(steps.abs().max()) <= 256


def ratio(err, A, floor=0.0):
    """largest (err - floor) / (2^-24 A); an element whose error is within the floor counts 0"""
    over = (err - floor).clamp(min=0)
    r = torch.where(over > 0, over / (U24 * A).clamp(min=1e-300), torch.zeros_like(over))
    return float(r.max()) if r.numel() else 0.0


def assert_rounded(got, want, A, c, dt, what, floor=0.0):
    assert got.dtype == dt, (what, got.dtype)
    got = as_f64(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(want).all() and torch.isfinite(A).all(), what
    assert torch.isfinite(got).all(), (what, "not finite")
    hu = half_ulp(want, dt)
    err = (got - want).abs()
    bound = hu + c * U24 * A + floor
    print("%-28s %-8s max (err - half ulp - floor) / (2^-24 A) = %8.3f   c = %s" % (
        what, str(dt).split(".")[1], ratio(err, A, hu + floor), ("%.1f" % float(torch.as_tensor(c).max()))))
    bad = err > bound
    if bad.any():
        i = tuple(bad.nonzero()[(err / bound.clamp(min=1e-300))[bad].argmax()].tolist())
        raise AssertionError((what, "%d of %d beyond the bound" % (int(bad.sum()), bad.numel()), "worst at", i, "got", float(got[i]), "want",
                              float(want[i]), "err", float(err[i]), "bound", float(bound[i]), "half ulp", float(hu[i])))


# ---------------------------------------------------------------------------------------------------------------------------------------
# gather_sum_rows: the backward of every row gather
# ---------------------------------------------------------------------------------------------------------------------------------------
# (dtype, C, entry, pad): lanes per (row, unit) follow from q = C / VL -- float32 q = 1, 4, 16, 32 (8, 8, 4, 2 lanes), 64 (one lane on the
# power-of-two path), 6 and 130 (the one-lane kernel); pad > 0: the gradient is a channel slice of a wider channels_last tensor (ldg = C + pad)
GATHER_CASES = [(F32, C, "interp", 0) for C in (4, 16, 64, 128, 256, 24, 520)] + [(BF16, C, "interp", 0) for C in (8, 64, 256, 512, 48)] + \
               [(F32, 16, "neigh", 8), (F32, 24, "neigh", 40), (BF16, 64, "neigh", 8), (BF16, 48, "neigh", 40)]
GATHER_B, GATHER_M, GATHER_U = 2, 25, 300


def gather_indices():
    """[2, 300] into 25 source rows: row m is read by exactly m outputs (0 .. 24 readers: 0, 1, L, L + 1, 2L, 2L + 1 and beyond for every
    lane count L <= 8, 0 .. 9 for the 4-way unrolled kernel), readers shuffled, another permutation per frame"""
    base = torch.repeat_interleave(torch.arange(GATHER_M), torch.arange(GATHER_M))
    assert base.numel() == GATHER_U
    return torch.stack([base[torch.randperm(GATHER_U, generator=gen("gather", b))] for b in range(GATHER_B)])


def run_gather_sum(device, dt, C, entry, pad, exact):
    """c = readers - 1: a sum of n values in any order makes n - 1 additions, each off by at most 2^-24 of a partial sum <= A"""
    B, M, U = GATHER_B, GATHER_M, GATHER_U
    g = gen("gather_sum", dt, C, pad, exact)
    idx = gather_indices()
    W = C + pad
    grad = (torch.randint(-1, 3, (B, U, W), generator=g).float() if exact else torch.randn(B, U, W, generator=g)).to(dt)
    feat = cl(torch.randn(B, C, M, 1, generator=g)).to(dt).to(device).requires_grad_(True)
    spatial = (U, 1) if entry == "interp" else (25, 12)
    with call_log("ffb6d_gather_rows_pm", "ffb6d_gather_sum_rows") as log:
        if entry == "interp":
            out = ops_cl.nearest_interpolation(feat, idx.to(device).unsqueeze(2))
        else:
            out = ops_cl.gather_neighbour(feat, idx.to(device).reshape(B, 25, 12))
        y = out if pad == 0 else torch.cat([out, cl(torch.zeros(B, pad, *spatial, dtype=dt, device=device))], dim=1)
        (gf,) = torch.autograd.grad(y, feat, as_cl_grad(grad.to(device), spatial))
    assert len(log["ffb6d_gather_rows_pm"]) == 1 and len(log["ffb6d_gather_sum_rows"]) == 1, log
    a = log["ffb6d_gather_sum_rows"][0]
    assert a[0] == int(dt == BF16) and a[2] == W and a[7] == C, a                 # the slice arrived as a slice: ldg = C + pad
    src = rows_of(feat)
    assert_exact(out.detach().reshape(B, C, U).transpose(1, 2), torch.stack([src[b][idx[b]] for b in range(B)]), dt, "gather forward")
    g64 = grad.double()[:, :, :C]
    want = torch.stack([torch.zeros(M, C, dtype=torch.float64).index_add_(0, idx[b], g64[b]) for b in range(B)])
    A = torch.stack([torch.zeros(M, C, dtype=torch.float64).index_add_(0, idx[b], g64[b].abs()) for b in range(B)])
    got = gf.reshape(B, C, M).transpose(1, 2)
    if exact:
        exact_conditions(want, A, dt)
        assert_exact(got, want, dt, "gather_sum_rows")
    else:
        readers = torch.stack([torch.bincount(idx[b], minlength=M) for b in range(B)])
        assert_rounded(got, want, A, (readers - 1).clamp(min=0).double().unsqueeze(2), dt, "gather_sum_rows")


# ---------------------------------------------------------------------------------------------------------------------------------------
# random_sample_rows_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------
# (M, Np, K, C); the last shape runs more than one workgroup in both dtypes (2 * 70 * q threads)
SAMPLE_SHAPES = [(20, 13, 16, 8), (20, 13, 1, 8), (20, 13, 5, 24), (40, 70, 16, 32)]
SAMPLE_CASES = [(dt, s, idt, False) for dt in DTS for s in SAMPLE_SHAPES for idt in (torch.int32, torch.int64)] + \
               [(dt, SAMPLE_SHAPES[0], torch.int64, True) for dt in DTS]


def first_max(gath):
    """the rule, stated: along K the FIRST maximum wins, and a NaN beats every number (its first occurrence), as in torch.max.
    gath [B,Np,K,C] -> (values, k of the winner) [B,Np,C]"""
    best, arg = gath[:, :, 0], torch.zeros(gath[:, :, 0].shape, dtype=torch.int64)
    for k in range(1, gath.shape[2]):
        v = gath[:, :, k]
        win = (v > best) | (torch.isnan(v) & ~torch.isnan(best))
        best, arg = torch.where(win, v, best), torch.where(win, torch.full_like(arg, k), arg)
    return best, arg


def run_random_sample(device, dt, shape, idt, nan):
    """exact only: features in {-1, 0, 1} (ties between different rows in every neighbourhood, and index rows that repeat entries),
    gradients in {-2 .. 2}; contributions to one source row add up"""
    M, Np, K, C = shape
    B = 2
    g = gen("random_sample", dt, shape, nan)
    feat = torch.randint(-1, 2, (B, C, M, 1), generator=g).float()
    idx = torch.randint(0, M, (B, Np, K), generator=g)
    if K > 1:
        idx[:, ::2, K - 1] = idx[:, ::2, 0]                          # the same row twice in one neighbourhood
    if nan:
        feat[0, 1, 3, 0] = float("nan")
        idx[0, 2, 5] = idx[0, 2, 9] = 3                              # twice in one neighbourhood: the first occurrence takes the gradient
    grad = torch.randint(-2, 3, (B, Np, C), generator=g).float().to(dt)
    x = cl(feat).to(dt).to(device).requires_grad_(True)
    with call_log("ffb6d_random_sample_pm", "ffb6d_random_sample_rows_bwd") as log:
        out = ops_cl.random_sample(x, idx.to(idt).to(device))
        (gf,) = torch.autograd.grad(out, x, as_cl_grad(grad.to(device), (Np, 1)))
    assert len(log["ffb6d_random_sample_pm"]) == 1 and len(log["ffb6d_random_sample_rows_bwd"]) == 1, log
    a = log["ffb6d_random_sample_rows_bwd"][0]
    assert a[0] == int(dt == BF16) and a[3] == (32 if idt == torch.int32 else 64), a
    src = rows_of(x)                                                 # [B,M,C]
    gath = src[torch.arange(B)[:, None, None], idx]                  # [B,Np,K,C]
    best, arg = first_max(gath)
    if K > 1:
        rows_at_max = torch.where(gath == best.unsqueeze(2), idx.unsqueeze(3).expand_as(gath), torch.full_like(idx.unsqueeze(3).expand_as(gath), -1))
        tied = (rows_at_max.max(dim=2)[0] != torch.where(rows_at_max < 0, torch.full_like(rows_at_max, M), rows_at_max).min(dim=2)[0])
        assert tied.float().mean() > 0.25                            # maxima shared by different source rows are the rule, not the exception
    assert torch.equal(torch.isnan(best), torch.isnan(gath).any(dim=2)) and bool(torch.isnan(best).any()) == nan
    assert_exact(out.detach().reshape(B, C, Np).transpose(1, 2), best, dt, "random_sample forward")
    winner = idx.unsqueeze(3).expand(B, Np, K, C).gather(2, arg.unsqueeze(2)).squeeze(2)          # [B,Np,C] source row
    want = torch.zeros(B, M, C, dtype=torch.float64).scatter_add_(1, winner, grad.double())
    A = torch.zeros(B, M, C, dtype=torch.float64).scatter_add_(1, winner, grad.double().abs())
    exact_conditions(want, A, dt)
    assert_exact(gf.reshape(B, C, M).transpose(1, 2), want, dt, "random_sample_rows_bwd")


# ---------------------------------------------------------------------------------------------------------------------------------------
# att_pool_rows / att_pool_rows_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------
# (dtype, K, C, sliced): K = 16 is the form that holds its rows in registers, the others the three-pass form; sliced: features and scores
# are channel slices of two channels_last tensors of different widths (ldf = C + 16, lds = C + 24)
POOL_CASES = [(dt, K, C, sliced) for dt in DTS for K in (16, 1, 5, 17) for C in (8, 40) for sliced in (False, True)]
POOL_B, POOL_N = 2, 9


def pool_operands(dt, K, C):
    """the nine points of a frame carry the score kinds: 0-3 3 * randn; 4, 5 40 * randn (one neighbour takes all the weight); 6 K equal
    scores; 7 one -inf among finite scores; 8 all but one -inf (K = 1: a lone -inf has no softmax, these two stay finite)"""
    B, N = POOL_B, POOL_N
    g = gen("att_pool", dt, K, C)
    f = torch.randn(B, C, N, K, generator=g)
    s = 3 * torch.randn(B, C, N, K, generator=g)
    s[:, :, 4:6] = 40 * torch.randn(B, C, 2, K, generator=g)
    s[:, :, 6] = torch.randn(B, C, 1, generator=g)
    if K > 1:
        s[:, :, 7, K // 2] = float("-inf")
        s[:, :, 8, :K - 1] = float("-inf")
    grad = torch.randn(B, C, N, 1, generator=g)
    return f.to(dt), s.to(dt), grad.to(dt), g


def pool_reference(f, s, grad):
    """float64, written out: z = s - max_K s, p = exp(z) / sum_K exp(z), out = sum_K p f, d/df = g p, d/ds = g p (f - out).
    The sums of absolute terms weigh every softmax weight with 1 + |z|: exp has the condition number |z|, and z is a rounded float32
    difference, so p_k arrives with a relative error of (1 + |z_k|) roundings whatever the expf -- a weight is a term of that size."""
    f, s, grad = f.double(), s.double(), grad.double()
    z = s - s.max(dim=3, keepdim=True)[0]
    w = torch.exp(z)
    p = w / w.sum(dim=3, keepdim=True)
    k = 1 + torch.nan_to_num(z.abs(), posinf=0.0)                   # a weight of exactly 0 (score -inf) is exact
    out = (p * f).sum(dim=3, keepdim=True)
    A_out = (p * k * f.abs()).sum(dim=3, keepdim=True)
    B_out = (p * f.abs()).sum(dim=3, keepdim=True)
    fmax = f.abs().max(dim=3, keepdim=True)[0]
    ref = {"out": (out, A_out, (1 + fmax) * TINY),
           "grad_feat": (grad * p, grad.abs() * p * k, grad.abs() * (1 + fmax) * TINY),
           "grad_scores": (grad * p * (f - out), grad.abs() * p * (k * (f.abs() + B_out) + A_out), grad.abs() * (1 + fmax) * TINY)}
    for want, A, _ in ref.values():                                  # -inf scores included: finite and free of NaN
        assert torch.isfinite(want).all() and torch.isfinite(A).all()
    return ref


def pool_torch_fp32(f, s, grad):
    """plain torch float32 on the CPU, the same formula (RandLANet.py:245-248) on the same operands"""
    f, s = f.float().clone().requires_grad_(True), s.float().clone().requires_grad_(True)
    out = (f * torch.softmax(s, dim=3)).sum(dim=3, keepdim=True)
    gf, gs = torch.autograd.grad(out, (f, s), grad.float())
    got = {"out": out.detach(), "grad_feat": gf.detach(), "grad_scores": gs.detach()}
    assert all(torch.isfinite(t).all() for t in got.values())
    return got


def run_att_pool(device, dt, K, C, sliced):
    B, N = POOL_B, POOL_N
    f, s, grad, g = pool_operands(dt, K, C)
    if sliced:
        fw = cl(torch.randn(B, C + 16, N, K, generator=g).to(dt))
        sw = cl(torch.randn(B, C + 24, N, K, generator=g).to(dt))
        fw[:, 8:8 + C], sw[:, :C] = f, s
        feat, sc = fw.to(device)[:, 8:8 + C].detach().requires_grad_(True), sw.to(device)[:, :C].detach().requires_grad_(True)
    else:
        feat, sc = cl(f).to(device).clone().requires_grad_(True), cl(s).to(device).clone().requires_grad_(True)
    ldf, lds = (C + 16, C + 24) if sliced else (C, C)
    with call_log("ffb6d_att_pool_rows", "ffb6d_att_pool_rows_bwd") as log:
        out = ops_cl.att_pool(feat, sc)
        gf, gs = torch.autograd.grad(out, (feat, sc), as_cl_grad(rows_like(grad, device), (N, 1)))
    assert len(log["ffb6d_att_pool_rows"]) == 1 and len(log["ffb6d_att_pool_rows_bwd"]) == 1, log
    a, b = log["ffb6d_att_pool_rows"][0], log["ffb6d_att_pool_rows_bwd"][0]
    assert (a[0], a[2], a[4], a[7], a[8]) == (int(dt == BF16), ldf, lds, K, C), a          # strided rows reached the kernel uncopied
    assert (b[0], b[4], b[6], b[10], b[11]) == (int(dt == BF16), ldf, lds, K, C), b
    ref = pool_reference(f, s, grad)
    for name, got in (("out", out.detach()), ("grad_feat", gf), ("grad_scores", gs)):
        want, A, floor = ref[name]
        assert_rounded(got, want, A, MEASURED["att_pool", name][1], dt, "att_pool " + name, floor)


def rows_like(x, device):
    """[B,C,*S] values -> [B,prod(S),C] contiguous rows on the device"""
    B, C = x.shape[:2]
    return x.reshape(B, C, -1).transpose(1, 2).contiguous().to(device)


# ---------------------------------------------------------------------------------------------------------------------------------------
# log_softmax_rows / log_softmax_rows_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------
# (dtype, C, scale of the values, upstream gradient): q = C / VL from 1 to 64; maps of 2 x 3 x 5 = 30 rows, so the last wave and workgroup
# are ragged at every q.  "lin": the gradient of tests/test_zz_ops_cl_gpu.py; "zero_sum": channel sum near zero (cancellation in g - p sum g)
LSM_SHAPES = [(F32, C) for C in (4, 8, 64, 256)] + [(BF16, C) for C in (8, 16, 512)]
LSM_CASES = [(dt, C, scale, gk) for dt, C in LSM_SHAPES for scale in (3.0, 80.0 if dt == F32 else 30.0) for gk in ("lin", "zero_sum")]
LSM_ISOLATION = [(dt, C, poison) for dt, C in LSM_SHAPES for poison in ("nan", "big")]
LSM_ROW = 7                                                           # the replaced row: shares its wave with other rows whenever q < 64


def lsm_operands(dt, C, scale, gk):
    shape = (2, C, 3, 5)
    g = gen("log_softmax", dt, C, scale, gk)
    x = scale * torch.randn(*shape, generator=g)
    if gk == "lin":
        grad = torch.linspace(-1.0, 1.0, x.numel()).reshape(shape)
    else:
        grad = torch.randn(*shape, generator=g)
        grad = grad - grad.mean(dim=1, keepdim=True)
    return x.to(dt), grad.to(dt)


def lsm_reference(x, grad):
    """float64, written out: z = x - m, y = z - log(sum exp z), gx = g - exp(y) sum(g).  As in pool_reference a softmax weight p = exp(y)
    is a term of size p (1 + |z|).  Terms of y: z, the logarithm, and the relative error of the sum inside it (d log s = ds / s):
    sum p (1 + |z|)."""
    x, grad = x.double(), grad.double()
    z = x - x.max(dim=1, keepdim=True)[0]
    ls = torch.log(torch.exp(z).sum(dim=1, keepdim=True))
    y = z - ls
    p = torch.exp(y)
    k = 1 + z.abs()
    sabs = grad.abs().sum(dim=1, keepdim=True)
    ref = {"out": (y, z.abs() + ls.abs() + (p * k).sum(dim=1, keepdim=True), 0.0),
           "grad": (grad - p * grad.sum(dim=1, keepdim=True), grad.abs() + p * k * sabs, (sabs * TINY).expand_as(x))}
    return ref


def lsm_torch_fp32(x, grad):
    x = x.float().clone().requires_grad_(True)
    y = torch.log_softmax(x, dim=1)
    (gx,) = torch.autograd.grad(y, x, grad.float())
    return {"out": y.detach(), "grad": gx.detach()}


def lsm_call(device, x, grad):
    xd = cl(x).to(device).clone().requires_grad_(True)
    with call_log("ffb6d_log_softmax_rows", "ffb6d_log_softmax_rows_bwd") as log:
        y = ops_cl.channel_log_softmax(xd)
        (gx,) = torch.autograd.grad(y, xd, cl(grad).to(device))
    assert len(log["ffb6d_log_softmax_rows"]) == 1 and len(log["ffb6d_log_softmax_rows_bwd"]) == 1, log
    assert log["ffb6d_log_softmax_rows"][0][0] == int(x.dtype == BF16) and log["ffb6d_log_softmax_rows"][0][4] == x.shape[1]
    return y.detach(), gx


def run_log_softmax(device, dt, C, scale, gk):
    x, grad = lsm_operands(dt, C, scale, gk)
    y, gx = lsm_call(device, x, grad)
    ref = lsm_reference(x, grad)
    for name, got in (("out", y), ("grad", gx)):
        want, A, floor = ref[name]
        assert_rounded(got, want, A, MEASURED["log_softmax", name][1], dt, "log_softmax " + name, floor)


def run_log_softmax_isolation(device, dt, C, poison):
    """rows share a wave when q < 64: one row replaced by NaN, or by +-1e4 alternating, must leave every other row of y and gx
    bit-identical to a run in which that row holds zeros, and show torch's own NaN pattern itself"""
    x, grad = lsm_operands(dt, C, 3.0, "lin")
    rows = x.permute(0, 2, 3, 1).reshape(-1, C)                                        # a copy: x is not channels_last
    bad = torch.full((C,), float("nan")) if poison == "nan" else 1e4 * (1 - 2 * (torch.arange(C) % 2)).float()

    def with_row(v):
        r = rows.clone()
        r[LSM_ROW] = v.to(dt)
        return r.reshape(2, 3, 5, C).permute(0, 3, 1, 2)
    keep = torch.ones(rows.shape[0], dtype=torch.bool)
    keep[LSM_ROW] = False
    y0, g0 = lsm_call(device, with_row(torch.zeros(C)), grad)
    y1, g1 = lsm_call(device, with_row(bad), grad)
    want = lsm_torch_fp32(with_row(bad), grad)
    for name, a, b in (("out", y0, y1), ("grad", g0, g1)):
        a, b = as_f64(a).permute(0, 2, 3, 1).reshape(-1, C), as_f64(b).permute(0, 2, 3, 1).reshape(-1, C)
        assert torch.isfinite(a).all(), name
        assert torch.equal(a[keep], b[keep]), (name, "a neighbouring row changed")
        t = want[name].permute(0, 2, 3, 1).reshape(-1, C)
        assert torch.equal(torch.isnan(b), torch.isnan(t)), (name, "NaN pattern")
        assert bool(torch.isnan(b[LSM_ROW]).all()) == (poison == "nan") and not torch.isinf(b).any(), name


# ---------------------------------------------------------------------------------------------------------------------------------------
# bilinear_bwd_pm: the backward of ops.upsample_align
# ---------------------------------------------------------------------------------------------------------------------------------------
# (IH, IW, OH, OW, C, dtypes, exact, native)
BILINEAR_CASES = [
    (2, 2, 4, 4, 8, DTS, False, True),             # smallest
    (3, 5, 5, 9, 8, DTS, True, True),              # ratio exactly 1/2: every weight is 0, 1/2 or 1 -- the exact case
    (5, 7, 13, 20, 8, DTS, False, True),           # non-integer ratios that differ per axis
    (3, 3, 9, 9, 8, DTS, False, True),             # OH = 4 IH - 3: the widest window the gate admits
    (3, 3, 10, 10, 8, DTS, False, False),          # one past the gate: ATen's backward, same bound
    (4, 6, 4, 6, 8, DTS, False, True),             # identity
    (6, 70, 12, 140, 16, [F32], False, True),      # 280 threads per row: two workgroups in x
]
BILINEAR_PARAMS = [(dt,) + c[:5] + c[6:] for c in BILINEAR_CASES for dt in c[5]]


def axis_matrix(I, O):
    """[O, I] weights with which output coordinate o reads input coordinate i, align_corners = True, from ATen's own float32
    source-index arithmetic restated in numpy float32 (UpSample.h: area_pixel_compute_scale / compute_source_index_and_lambda):
    scale = float32(I - 1) / float32(O - 1), s = scale * float32(o), i0 = int(s), l1 = s - i0, l0 = 1 - l1.  The weights are float32
    values; the matrix holds them in float64.  (Weights from float64 indices differ by ~1e-5 at 140 columns.)"""
    scale = np.float32(I - 1) / np.float32(O - 1) if O > 1 else np.float32(0)
    s = scale * np.arange(O, dtype=np.float32)
    assert s.dtype == np.float32
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < I - 1)
    l1 = s - i0.astype(np.float32)
    l0 = np.float32(1) - l1
    assert l0.dtype == np.float32 and l1.dtype == np.float32
    W = np.zeros((O, I), dtype=np.float64)
    np.add.at(W, (np.arange(O), i0), l0.astype(np.float64))
    np.add.at(W, (np.arange(O), i1), l1.astype(np.float64))
    return torch.from_numpy(W)


def bilinear_reference(grad, IH, IW):
    """gin[b,c,iy,ix] = sum over (oy, ox) of wy[oy,iy] wx[ox,ix] g[b,c,oy,ox] in float64; A the same with |g|; T the number of non-zero terms"""
    OH, OW = grad.shape[2:]
    wy, wx = axis_matrix(IH, OH), axis_matrix(IW, OW)
    want = torch.einsum("oi,pj,bcop->bcij", wy, wx, grad.double())
    A = torch.einsum("oi,pj,bcop->bcij", wy, wx, grad.double().abs())
    T = (wy != 0).sum(dim=0).double()[:, None] * (wx != 0).sum(dim=0).double()[None, :]
    return want, A, T


def run_bilinear(device, dt, IH, IW, OH, OW, C, exact, native):
    """c = T + 2 for T non-zero terms: one rounding of the weight product wy wx and one of the (fused) accumulation per term -- T - 1
    additions and T products -- plus one per axis where l0 + l1 of a clamped border pixel is added in float32.  The exact case has
    gradients in {-4, 0, 4, 8}: products with weights {0, 1/4, 1/2, 1} are integers.
    native = False: one past the gate of ops.upsample_align, ATen's backward runs (two roundings per product, T - 1 additions: within the
    same c).  On the device ATen adds each term onto a gradient of the map's own type with an atomic; a bfloat16 map missed this bound by
    three orders of magnitude until the fallback summed in float32 and rounded once (ops._UpsampleAlign.backward)."""
    B = 2
    g = gen("bilinear", dt, IH, IW, OH, OW)
    x = cl(torch.randn(B, C, IH, IW, generator=g)).to(dt).to(device).requires_grad_(True)
    grad = (4.0 * torch.randint(-1, 3, (B, C, OH, OW), generator=g) if exact else torch.randn(B, C, OH, OW, generator=g)).to(dt)
    with call_log("ffb6d_bilinear_resize_pm", "ffb6d_bilinear_bwd_pm") as log, aten_bilinear_backward_log() as aten:
        y = ops.upsample_align(x, (OH, OW))
        (gx,) = torch.autograd.grad(y, x, cl(grad).to(device))
    assert len(log["ffb6d_bilinear_resize_pm"]) == 1, log
    assert (len(log["ffb6d_bilinear_bwd_pm"]), len(aten)) == ((1, 0) if native else (0, 1)), (log, aten)
    if native:
        assert log["ffb6d_bilinear_bwd_pm"][0][0] == int(dt == BF16)
    want, A, T = bilinear_reference(grad, IH, IW)
    if exact:
        exact_conditions(want, A, dt)
        assert_exact(gx, want, dt, "bilinear_bwd_pm")
    else:
        assert_rounded(gx, want, A, T + 2, dt, "bilinear_bwd_pm" if native else "ATen bilinear backward")


def check_bilinear_restatement():
    """the restated index arithmetic against float64 F.interpolate autograd, 1e-4 of range, every resize of the table"""
    for IH, IW, OH, OW, C in sorted({c[:5] for c in BILINEAR_CASES}):
        g = gen("restatement", IH, IW, OH, OW)
        x = torch.randn(2, C, IH, IW, generator=g, dtype=torch.float64, requires_grad=True)
        grad = torch.randn(2, C, OH, OW, generator=g, dtype=torch.float64)
        y = torch.nn.functional.interpolate(x, size=(OH, OW), mode="bilinear", align_corners=True)
        (gx,) = torch.autograd.grad(y, x, grad)
        want, _, _ = bilinear_reference(grad, IH, IW)
        assert float((want - gx).abs().max()) <= 1e-4 * float(gx.abs().max()), (IH, IW, OH, OW)


# ---------------------------------------------------------------------------------------------------------------------------------------
# prelu_fwd / prelu_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------
SLOPES = [0.5, -0.25, 0.0, 1.5]
# (dtype, shape, memory format): one unit; one workgroup; (2,16,33,35) = 37 workgroups in float32
PRELU_SHAPES = [(F32, (1, 4, 1, 1), "nchw"), (BF16, (1, 8, 1, 1), "nchw")] + \
               [(dt, shape, fmt) for dt in DTS for shape in ((2, 8, 5, 6), (2, 16, 33, 35)) for fmt in ("nchw", "cl")]
PRELU_CASES = [(dt, shape, fmt, slope, kind) for dt, shape, fmt in PRELU_SHAPES for slope in SLOPES for kind in ("exact", "rounded")] + \
              [(dt, (2, 8, 5, 6), "cl", slope, "nan") for dt in DTS for slope in SLOPES]
# more units than 4096 workgroups x 256 threads: the grid-stride loop makes a second trip (17 MB, milliseconds on the device)
PRELU_BIG = [(F32, (1, 8, 724, 725), "cl"), (BF16, (1, 16, 724, 725), "nchw")]


def prelu_operands(dt, shape, slope, kind):
    g = gen("prelu", dt, shape, slope, kind)
    n = int(np.prod(shape))
    if kind == "rounded":
        return torch.randn(*shape, generator=g).to(dt), torch.randn(*shape, generator=g).to(dt)
    vals = torch.tensor([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0])
    grad = torch.randint(-1, 3, shape, generator=g).float()
    if kind == "big":                            # only every 97th element is non-positive: the slope gradient's terms stay below 2^24 in
        x = vals[torch.randint(4, 6, (n,), generator=g)]              # total, every workgroup and every loop trip still contributes
        x[::97] = vals[torch.randint(0, 4, (len(range(0, n, 97)),), generator=g)]
        x = x.reshape(shape)
    else:
        x = vals[torch.randint(0, 6, (n,), generator=g)].reshape(shape)
    if kind == "nan":
        x.view(-1)[[3, n // 2]] = float("nan")
    return x.to(dt), grad.to(dt)


def run_prelu(device, dt, shape, fmt, slope, kind):
    """torch's rule at zero and at NaN: y = x > 0 ? x : a x, gx = x > 0 ? g : a g, slope gradient = sum over x <= 0 (or NaN) of g x.
    Rounded: y and gx are one product, c = 1; the slope gradient sums its n non-zero terms in any order, c = n - 1 (bf16 products are
    exact in float32; a float32 product's rounding takes the place of the last addition's, which the half ulp of the result covers)."""
    x, grad = prelu_operands(dt, shape, slope, kind)
    put = cl if fmt == "cl" else (lambda t: t.contiguous())
    xd, w = put(x).to(device).clone().requires_grad_(True), torch.tensor([slope], device=device, requires_grad=True)
    with call_log("ffb6d_prelu_fwd", "ffb6d_prelu_bwd") as log:
        y = ops.prelu(xd, w)
        gx, gw = torch.autograd.grad(y, (xd, w), put(grad).to(device))
    assert len(log["ffb6d_prelu_fwd"]) == 1 and len(log["ffb6d_prelu_bwd"]) == 1, log
    assert log["ffb6d_prelu_bwd"][0][0] == int(dt == BF16) and log["ffb6d_prelu_bwd"][0][6] == x.numel()
    assert y.stride() == xd.stride() and gx.stride() == xd.stride() and gw.shape == (1,)
    x64, g64 = x.double(), grad.double()
    pos = x64 > 0
    want_y, want_gx = torch.where(pos, x64, slope * x64), torch.where(pos, g64, slope * g64)
    terms = torch.where(pos, torch.zeros_like(x64), g64 * x64)
    want_gw, A_gw = terms.sum().reshape(1), terms.abs().sum().reshape(1)
    if kind == "rounded":
        assert_rounded(y.detach(), want_y, (slope * x64).abs() * ~pos, 1.0, dt, "prelu y")
        assert_rounded(gx, want_gx, (slope * g64).abs() * ~pos, 1.0, dt, "prelu gx")
        assert_rounded(gw, want_gw, A_gw, float(max(int((terms != 0).sum()) - 1, 0)), F32, "prelu slope gradient")
        return
    exact_conditions(want_y, want_y.abs(), dt, grid=0.25)
    exact_conditions(want_gx, want_gx.abs(), dt, grid=0.25)
    exact_conditions(want_gw, A_gw, F32)
    assert_exact(y.detach(), want_y, dt, "prelu y", signed_zero=True)
    assert_exact(gx, want_gx, dt, "prelu gx", signed_zero=True)
    assert_exact(gw, want_gw, F32, "prelu slope gradient")
    if kind == "nan":                            # the NaN pattern of all three is torch's own
        xt, wt = x.float().clone().requires_grad_(True), torch.tensor([slope], requires_grad=True)
        yt = torch.nn.functional.prelu(xt, wt)
        gxt, gwt = torch.autograd.grad(yt, (xt, wt), grad.float())
        assert int(torch.isnan(yt).sum()) == 2 and not torch.isnan(gxt).any() and torch.isnan(gwt).all()
        for got, t in ((y, yt), (gx, gxt), (gw, gwt)):
            assert torch.equal(torch.isnan(got.detach().cpu()), torch.isnan(t.detach()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# nearest_interpolation backward, channel-major float32 (csrc/neighbour_ops.hip entry, csrc/train_ops.hip privatised form)
# ---------------------------------------------------------------------------------------------------------------------------------------
# (B, C, M, U): privatised in LDS with the channel group halved and ragged; the largest M whose rows fit the 96 KB LDS budget; one more:
# the global-atomic fallback
NEAREST_SHAPES = [(2, 7, 50, 300), (1, 3, 24576, 300), (1, 3, 24577, 300)]
NEAREST_CASES = [s + (idt,) for s in NEAREST_SHAPES for idt in (torch.int32, torch.int64)]


def run_nearest_cm(device, B, C, M, U, idt):
    """exact: integer gradients; indices include 0 and M - 1, every fifth output reads M - 1"""
    g = gen("nearest_cm", B, C, M, U)
    idx = torch.randint(0, M, (B, U), generator=g)
    idx[:, 1] = 0
    idx[:, ::5] = M - 1
    grad = torch.randint(-2, 3, (B, C, U, 1), generator=g).float()
    feat = torch.randn(B, C, M, 1, generator=g).to(device).requires_grad_(True)
    with call_log("ffb6d_nearest_interpolation_f32", "ffb6d_nearest_interpolation_bwd_f32") as log:
        out = ops.nearest_interpolation(feat, idx.to(idt).to(device).unsqueeze(2))
        (gf,) = torch.autograd.grad(out, feat, grad.to(device))
    assert len(log["ffb6d_nearest_interpolation_f32"]) == 1 and len(log["ffb6d_nearest_interpolation_bwd_f32"]) == 1, log
    a = log["ffb6d_nearest_interpolation_bwd_f32"][0]
    assert a[2] == (32 if idt == torch.int32 else 64) and tuple(a[4:8]) == (B, C, M, U), a
    src = as_f64(feat).squeeze(3)
    sel = idx.unsqueeze(1).expand(B, C, U)
    assert_exact(out.detach().squeeze(3), src.gather(2, sel), F32, "nearest_interpolation forward")
    want = torch.zeros(B, C, M, dtype=torch.float64).scatter_add_(2, sel, grad.double().squeeze(3))
    A = torch.zeros(B, C, M, dtype=torch.float64).scatter_add_(2, sel, grad.double().squeeze(3).abs())
    exact_conditions(want, A, F32)
    assert_exact(gf.squeeze(3), want, F32, "nearest_interpolation_bwd")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the MEASURED table
# ---------------------------------------------------------------------------------------------------------------------------------------
def torch_fp32_ratios():
    """largest |torch_fp32 - float64| / (2^-24 A) (beyond the underflow floor) of plain torch float32 on the CPU over all cases of
    POOL_CASES and LSM_CASES, per operator and output"""
    worst = {k: 0.0 for k in MEASURED}
    for dt, K, C, _ in POOL_CASES:
        f, s, grad, _ = pool_operands(dt, K, C)
        ref, got = pool_reference(f, s, grad), pool_torch_fp32(f, s, grad)
        for name, (want, A, floor) in ref.items():
            worst["att_pool", name] = max(worst["att_pool", name], ratio((got[name].double() - want).abs(), A, floor))
    for dt, C, scale, gk in LSM_CASES:
        x, grad = lsm_operands(dt, C, scale, gk)
        ref, got = lsm_reference(x, grad), lsm_torch_fp32(x, grad)
        for name, (want, A, floor) in ref.items():
            worst["log_softmax", name] = max(worst["log_softmax", name], ratio((got[name].double() - want).abs(), A, floor))
    return worst


if __name__ == "__main__":
    import math
    for key, r in torch_fp32_ratios().items():
        r = math.ceil(100 * r) / 100                       # recorded rounded up to two decimals; c = 4 x the recorded figure
        print("    %r: (%.2f, %.2f)," % (key, r, 4 * r))
