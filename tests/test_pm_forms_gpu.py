"""Every form of the point-major GEMM family against every operand feature, on the device (tests/pm_cases.py holds the table and says
what a form and a feature are).  The form a layer takes is chosen from its shape (ffb6d_mlp_pm_choice / ffb6d_mlp_pm_tile), so another
point count or class count sends a layer through a (form, feature) pair: here every such pair has run once.  LDS-DMA loads, barrier
placement and prefetch order exist on the chip only; `--emulate` runs the same cases as a functional pre-flight (the boundaries test
excepted: -k "not boundaries").

Bars: fp32 max|got - want| <= 1e-5 max|want| against float64 (the GEMM bar of this suite); bf16 tests/test_pm_gpu.py::_close_bf16
against float64 of the bf16-rounded operands.  Every slice lives in a buffer whose other columns are NaN -- inputs and `out` alike."""
import time

import pytest
import torch

from ffb6d_amd import _lib, ops_pm
import pm_cases as pc
from test_pm_gpu import BF, SEQ, _close_bf16, _lfa_case

pytestmark = pytest.mark.gpu

WORST = {}          # (what, dtype) -> worst error seen, in units of the bar


@pytest.fixture(scope="module", autouse=True)
def report():
    """Not a check: after the module's tests, print (-s shows it) the cases per form, the worst error per form and dtype in units of
    its bar, and the wall time"""
    import collections
    t0 = time.time()
    yield
    n = collections.Counter((c.form, c.dt) for c in pc.CASES)
    print("\npm forms: cases per form " + ", ".join(f"{f}/{d} {k}" for (f, d), k in sorted(n.items())))
    print("pm forms: worst error / bar " + ", ".join(f"{f}/{d} {e:.3f}" for (f, d), e in sorted(WORST.items())))
    print(f"pm forms: {time.time() - t0:.1f} s")


def _dev(o, device):
    """operands on the device; slices stay slices (the wide buffer moves, the view is taken again)"""
    def mv(t):
        if t is None:
            return None
        if t._base is None:
            return t.to(device)
        base = t._base.to(device)
        return base.as_strided(t.shape, t.stride(), t.storage_offset())
    out = {k: mv(v) for k, v in o.items() if k not in ("gather", "out", "out_wide")}
    out["gather"] = None if o["gather"] is None else (mv(o["gather"][0]), o["gather"][1].to(device))
    if o["out_wide"] is None:
        out["out"], out["out_wide"] = o["out"].to(device), None
    else:
        out["out_wide"] = o["out_wide"].to(device)
        out["out"] = out["out_wide"].as_strided(o["out"].shape, o["out"].stride(), o["out"].storage_offset())
    return out


def _call(d, act, hint):
    return ops_pm.mlp(d["x1"], d["w"], d["bias"], act, x2=d["x2"], add=d["add"], gather=d["gather"], x1_gather=d["x1_gather"],
                      out=d["out"], tile_hint=hint)


def _neighbours_are_nan(d, cout, left=8):
    w = d["out_wide"]
    return w is None or bool(torch.isnan(w[..., :left]).all() and torch.isnan(w[..., left + cout:]).all())


def _note(what, dt, err):
    WORST[(what, dt)] = max(WORST.get((what, dt), 0.0), err)


def _check(got, want, dt, what, label):
    """the bar of the dtype; the error is recorded in units of the bar before anything is asserted"""
    got, want = got.double().cpu(), want.double()
    assert got.shape == want.shape and not bool(torch.isnan(got).any()), (label, "NaN in the result")
    if dt == "f32":
        bar = 1e-5 * float(want.abs().max())
        err = float((got - want).abs().max())
        _note(what, dt, err / bar if bar > 0 else (0.0 if err == 0 else float("inf")))
        assert err <= bar, (label, err, bar)
    else:
        tol = 2.0 ** -8 * want.abs() + 2.0 ** -8 * float(want.abs().mean())
        _note(what, dt, float(((got - want).abs() / tol.clamp_min(1e-300)).max()))
        _close_bf16(got, want, label)


@pytest.mark.parametrize("c", pc.CASES, ids=pc.case_id)
def test_form_honours_the_operand_features(device, c):
    """One table case through its form: float64 bar, no NaN from the padding of any slice, `out`'s neighbours still NaN"""
    o = pc.operands(c)
    d = _dev(o, device)
    got = _call(d, c.act, c.hint)
    assert got.data_ptr() == d["out"].data_ptr()
    _check(got, pc.reference(o, c.act), c.dt, c.form, pc.case_id(c))
    assert _neighbours_are_nan(d, c.cout), "columns beside the out slice were written"


SIBLING = {"f32": ("seq", pc.HINTS["seq"]), "bf16": ("big", pc.HINTS["big"])}
BOTH = [c for c in pc.CASES if c.form in ("lds", "seq", "big") and pc.in_domain(c._replace(form="lds", hint=7)) and
        pc.in_domain(c._replace(form=SIBLING[c.dt][0], hint=SIBLING[c.dt][1][0]))]


@pytest.mark.parametrize("c", BOTH, ids=pc.case_id)
def test_long_row_forms_carry_equal_bits(device, c):
    """mlp_pm_seq_kernel (fp32) and mlp_pm_big_kernel (bf16) feed every accumulator the same products in the same k order as
    mlp_pm_lds_kernel and run the same epilogue arithmetic (test_tile_sequence_and_big_tile_forms_equal_the_lds_tiled_form_bit_for_bit):
    here with gathered operand rows, slices, int32 indices and a missing bias, which change addresses and not arithmetic.  Every table
    case in the domain of both forms; a case of the LDS-tiled form runs through every plan of its sibling.  (Equal on the emulator for
    every feature: none is held to float64 only.)"""
    o = pc.operands(c)
    want = _call(_dev(o, device), c.act, 7).clone()
    for h in ((c.hint,) if c.form != "lds" else SIBLING[c.dt][1]):
        d = _dev(o, device)
        got = _call(d, c.act, h)
        assert torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), (pc.case_id(c), h)
        assert _neighbours_are_nan(d, c.cout)


@pytest.mark.parametrize("what,c", pc.REJECTED, ids=[w for w, _ in pc.REJECTED])
def test_form_rejects_what_lies_outside_its_domain(device, what, c):
    """One case per documented constraint, just outside it: refused by the host code, `out` untouched"""
    d = _dev(pc.operands(c), device)
    with pytest.raises(_lib.FFB6DNativeError):
        _call(d, c.act, c.hint)
    assert bool(torch.isnan(d["out_wide"]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# the batched-weight entry
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,R,K,cout,hint", pc.BATCHED)
def test_mlp_batched_at_its_edges(device, G, R, K, cout, hint):
    """x [G,R,K] w [G,cout,K]: float64, and the documented contract -- every out[g] carries the bits of mlp(x[g], w[g]) in the same form"""
    g = torch.Generator().manual_seed(G + R + K + cout)
    x, w = torch.randn(G, R, K, generator=g), torch.randn(G, cout, K, generator=g) / K ** 0.5
    xd, wd = x.to(device), w.to(device)
    out = torch.full((G, R, cout), pc.NAN, device=device)
    got = ops_pm.mlp_batched(xd, wd, out=out, tile_hint=hint)
    _check(got, x.double() @ w.double().transpose(1, 2), "f32", "batched", (G, R, K, cout, hint))
    one = hint if hint else SEQ(1)        # tile_hint 0 of the batched entry: the tile-sequence form in whole-point-tile groups
    for i in sorted({0, G // 2, G - 1}):
        assert torch.equal(got[i], ops_pm.mlp(xd[i], wd[i], tile_hint=7 if hint == 7 else one)), (i, "differs from mlp(x[g], w[g])")


@pytest.mark.parametrize("what,G,R,K,cout,hint", pc.BATCHED_REJECTED, ids=[b[0] for b in pc.BATCHED_REJECTED])
def test_mlp_batched_rejects_what_lies_outside_its_domain(device, what, G, R, K, cout, hint):
    x, w = torch.randn(G, R, K).to(device), torch.randn(G, cout, K).to(device)
    out = torch.full((G, R, cout), pc.NAN, device=device)
    with pytest.raises(_lib.FFB6DNativeError):
        ops_pm.mlp_batched(x, w, out=out, tile_hint=hint)
    assert bool(torch.isnan(out).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# the automatic choice at its thresholds (device only: up to 131072 rows)
# ---------------------------------------------------------------------------------------------------------------------------------
def _big_case(device, rows, cout, k1, k2, act, bf16, xg, extra=0):
    """operands made on the device, float64 matmul by torch on the device"""
    tdt = BF if bf16 else torch.float32
    g = torch.Generator(device=device).manual_seed(rows + cout + k1)
    r = lambda *s: torch.randn(*s, generator=g, device=device).to(tdt)               # noqa: E731
    B = 2 if rows % 2 == 0 else 1
    P = rows // B
    M = 777 if xg else P
    x1, x2 = r(B, M, k1), (r(B, P, k2) if k2 else None)
    w = (torch.randn(cout, k1 + k2, generator=g, device=device) / (k1 + k2) ** 0.5).to(tdt)
    bias = torch.randn(cout, generator=g, device=device)
    idx = torch.randint(0, M, (B, P), generator=g, device=device) if xg else None
    wide = torch.full((B, P, cout + extra), pc.NAN, dtype=tdt, device=device)
    got = ops_pm.mlp(x1, w, bias, act, x2=x2, x1_gather=idx, out=wide[..., :cout], tile_hint=0)
    o = dict(x1=x1, x2=x2, w=w, bias=bias, add=None, gather=None, x1_gather=idx)
    return got, pc.reference(o, act), wide


@pytest.mark.parametrize("what,rows,cout,k1,k2,act,bf16,xg,form", pc.BOUNDARIES,
                         ids=[f"{b[0]}-{b[1]}x{b[3] + b[4]}x{b[2]}".replace(" ", "_") for b in pc.BOUNDARIES])
def test_automatic_choice_boundaries(device, native_lib, what, rows, cout, k1, k2, act, bf16, xg, form):
    """One shape on each side of every threshold of ffb6d_mlp_pm_choice / ffb6d_mlp_pm_tile, tile_hint 0: the form first (a pure host
    function), then the result against float64"""
    assert native_lib.ffb6d_mlp_pm_choice(rows, cout, k1, k2, act, bf16, xg) & 255 == form
    got, want, _ = _big_case(device, rows, cout, k1, k2, act, bf16, xg)
    _check(got, want.cpu(), "bf16" if bf16 else "f32", "auto", what)


@pytest.mark.parametrize("what,rows,cout,k1,bf16,form,extra", pc.FALLBACKS, ids=[f[0].split(":")[0].replace(" ", "_") for f in pc.FALLBACKS])
def test_automatic_choice_boundaries_fall_back_on_misaligned_rows(device, native_lib, what, rows, cout, k1, bf16, form, extra):
    """The shape asks for the stream / tile-sequence / 256 x 256 form, the row stride of `out` rules it out: mlp_pm_impl takes the next
    form instead of refusing"""
    assert native_lib.ffb6d_mlp_pm_choice(rows, cout, k1, 0, 1, bf16, 0) & 255 == form
    got, want, wide = _big_case(device, rows, cout, k1, 0, 1, bf16, 0, extra=extra)
    _check(got, want.cpu(), "bf16" if bf16 else "f32", "auto", what)
    assert bool(torch.isnan(wide[..., cout:]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# sibling entry points that share the loaders
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("d,p_hint,N,mode,bits,B", pc.LFA)
def test_lfa_half_strided_table_and_sliced_rows(device, d, p_hint, N, mode, bits, B, dt):
    """What forward_pm.py feeds lfa_half and no operator test did: the coordinate table as the first N rows of every frame of a finer
    level's table ([B, 3N + 5, 4][:, :N], NaN beyond N), `f` and `out` as channel slices of NaN-padded row buffers.  fp32: the float64
    restatement oracle/ops_ref.lfa_half, 1e-5 of the range; bf16: the bar of test_fused_lfa_half_bf16 (2e-2 of the range, two store
    roundings restated)"""
    from oracle import ops_ref
    tdt = torch.float32 if dt == "f32" else BF
    a = _lfa_case(B, N, d, mode, tdt, torch.int32 if bits == 32 else torch.int64, seed=N + d + mode + p_hint)
    table = torch.full((B, 3 * N + 5, 4), pc.NAN)
    table[:, :N, :3] = a["xyz"]
    table[:, :N, 3] = 0
    cout = d // 2 if mode == 1 else d
    f, _ = pc.nan_slice(a["f"], True)
    out, out_wide = pc.nan_slice(torch.full((B, N, cout), pc.NAN, dtype=tdt), True)
    dd = _dev(dict(f=f, out=out, out_wide=out_wide, gather=None), device)
    dv = {k: v.to(device) for k, v in a.items() if k not in ("f", "xyz")}
    kw = dict(w2=dv["w2"], b2=dv["b2"], act2=2) if mode == 2 else {}
    got = ops_pm.lfa_half(mode, table.to(device)[:, :N], dv["nei"], dd["f"], dv["w1"], dv["b1"], 2, dv["wfc"], dv["wm"], dv["bm"], 2,
                          out=dd["out"], p_hint=p_hint, **kw).cpu()
    kr = dict(w2=a["w2"], b2=a["b2"], act2=2) if mode == 2 else {}
    store = None if dt == "f32" else (lambda t: t.to(BF).to(torch.float64))
    want = ops_ref.lfa_half(mode, a["xyz"], a["nei"], a["f"], a["w1"], a["b1"], 2, a["wfc"], a["wm"], a["bm"], 2, store=store, **kr)
    assert got.shape == want.shape and got.dtype == tdt and not bool(torch.isnan(got).any())
    bar = (1e-5 if dt == "f32" else 2e-2) * float(want.abs().max())
    err = float((got.double() - want).abs().max())
    _note("lfa_half", dt, err / bar)
    assert err <= bar, (err, bar)
    assert _neighbours_are_nan(dd, cout)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B,N,C1,C2,bits", [(2, 129, 16, 16, 32), (1, 63, 32, 32, 64), (3, 17, 64, 64, 32), (2, 1, 128, 128, 64),
                                            (1, 300, 16, 48, 64), (2, 65, 96, 32, 32)])
def test_att_pool_sliced_rows(device, B, N, C1, C2, bits, dt):
    """`f`, `g` and `out` as channel slices of NaN-padded row buffers, both index types"""
    tdt = torch.float32 if dt == "f32" else BF
    g = torch.Generator().manual_seed(N + C1 + C2)
    f = torch.randn(B, N, C1, generator=g).to(tdt)
    nei = torch.randint(0, N, (B, N, 16), generator=g).to(torch.int32 if bits == 32 else torch.int64)
    pair = torch.randn(B, N, 16, C2, generator=g).to(tdt)
    d_ = C1 + C2
    w = (torch.randn(d_, d_, generator=g) / d_ ** 0.5 * 3).to(tdt)
    S = torch.cat([torch.gather(f.double(), 1, nei.long().reshape(B, -1, 1).expand(-1, -1, C1)).view(B, N, 16, C1), pair.double()], dim=3)
    want = (S * torch.softmax(S @ w.double().t(), dim=2)).sum(dim=2)
    out, out_wide = pc.nan_slice(torch.full((B, N, d_), pc.NAN, dtype=tdt), True)
    dd = _dev(dict(f=pc.nan_slice(f, True)[0], pair=pc.nan_slice(pair, True, left=16)[0], out=out, out_wide=out_wide, gather=None), device)
    got = ops_pm.att_pool(dd["f"], nei.to(device), dd["pair"], w.to(device), out=dd["out"])
    _check(got, want, dt, "att_pool", (B, N, C1, C2))
    assert _neighbours_are_nan(dd, d_)


@pytest.mark.parametrize("cols,cout,N,bits", [(10, 16, 65, 64), (12, 32, 17, 32), (16, 64, 130, 64), (13, 128, 1, 32)])
def test_posenc_mlp_weight_as_the_first_columns_of_a_wider_matrix(device, cols, cout, N, bits):
    """`w` [cout, 10 .. 16] as the first columns of a [cout, 40] matrix (stride(0) > row; NaN beyond), columns past 10 ignored"""
    from oracle import ops_ref
    g = torch.Generator().manual_seed(cols + cout)
    B = 2
    xyz = torch.rand(B, N, 3, generator=g)
    nei = torch.randint(0, N, (B, N, 16), generator=g).to(torch.int32 if bits == 32 else torch.int64)
    wide = torch.full((cout, 40), pc.NAN)
    wide[:, :cols] = torch.randn(cout, cols, generator=g) / 2
    bias = torch.randn(cout, generator=g) / 2
    enc = ops_ref.relative_pos_encoding(xyz.double(), nei.long())
    want = torch.nn.functional.leaky_relu(enc @ wide[:, :10].double().t() + bias.double(), 0.2)
    got = ops_pm.posenc_mlp(xyz.to(device), nei.to(device), wide.to(device)[:, :cols], bias.to(device), 2)
    _check(got, want, "f32", "posenc_mlp", (cols, cout, N))
