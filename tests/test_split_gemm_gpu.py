"""The split-bf16 form of the long-row fp32 GEMMs (ffb6d_amd/csrc/mlp_pm_split.hip; ops_pm.mlp / mlp_batched with tile_hint 10) on the
device, at small shapes that cross its seams: ragged first and last point tiles (128 rows) and channel tiles (256), a third channel
tile, two and an odd number of 32-k steps, the stage ring's wrap, every epilogue feature, NaN-padded channel slices on every operand,
and the batched entry.

Bars: max|got - want| <= 1e-5 max|want| against float64 (the fp32 GEMM bar of tests/test_pm_forms_gpu.py::_check); equal bits between
two runs and between the batched entry and separate launches.  The distance to the CPU restatement (tests/split_gemm_ref.py, which
idealises the MFMA's inner sum as exact) is printed in ulps (-s) and not asserted: the instruction's inner rounding is not documented."""
import pytest
import torch

from ffb6d_amd import _lib, ops_pm
import split_gemm_ref as ref

pytestmark = pytest.mark.gpu

LEFT = 8            # NaN columns on both sides of every slice (32 bytes: the slices stay 16-byte aligned)


def _padded(t):
    """t [..., C] -> a slice of a wider buffer whose other columns are NaN"""
    wide = torch.full(t.shape[:-1] + (t.shape[-1] + 2 * LEFT,), float("nan"), dtype=t.dtype)
    wide[..., LEFT:LEFT + t.shape[-1]] = t
    return wide


def _slice(wide_dev, c):
    return wide_dev[..., LEFT:LEFT + c]


def _operands(rows, cout, K, bias, extra, seed):
    """CPU operands of one case; rows are laid out as [B = 1 or 3][P] when an index array needs frames"""
    gen = torch.Generator().manual_seed(seed)
    B = 3 if rows % 3 == 0 else 1
    P = rows // B
    o = dict(B=B, P=P, x=torch.randn(B, P, K, generator=gen).clamp_min(-0.5), w=torch.randn(cout, K, generator=gen) / K ** 0.5,
             bias=torch.randn(cout, generator=gen) if bias else None, add=None, y=None, idx=None)
    if extra == "add":
        o["add"] = torch.randn(B, P, cout, generator=gen)
    elif extra in ("gather32", "gather64"):
        py = 37
        o["y"] = torch.randn(B, py, cout, generator=gen)
        o["idx"] = torch.randint(0, py, (B, P), generator=gen, dtype=torch.int32 if extra == "gather32" else torch.int64)
    return o


def _want64(o, act):
    v = o["x"].double() @ o["w"].double().T
    if o["bias"] is not None:
        v = v + o["bias"].double()
    if o["add"] is not None:
        v = v + o["add"].double()
    if o["y"] is not None:
        v = v + torch.stack([o["y"][b].double()[o["idx"][b].long()] for b in range(o["B"])])
    slope = (1.0, 0.0, 0.2)[act]
    return torch.maximum(v, slope * v)


def _restated(o, act):
    acc = ref.gemm(o["x"].reshape(-1, o["x"].shape[-1]), o["w"]).reshape(o["B"], o["P"], -1)
    extra = o["add"]
    if o["y"] is not None:
        extra = torch.stack([o["y"][b][o["idx"][b].long()] for b in range(o["B"])])
    return ref.epilogue(acc, o["bias"], extra, act)


def _run(o, act, device, w3=None):
    """through ops_pm.mlp with every operand and `out` a slice of a NaN-padded buffer -> (out slice, out's wide buffer)"""
    cout, K = o["w"].shape
    x = _slice(_padded(o["x"]).to(device), K)
    w = o["w"].to(device)
    out_wide = torch.full((o["B"], o["P"], cout + 2 * LEFT), float("nan"), device=device)
    kw = {}
    if o["add"] is not None:
        kw["add"] = _slice(_padded(o["add"]).to(device), cout)
    if o["y"] is not None:
        kw["gather"] = (_slice(_padded(o["y"]).to(device), cout), o["idx"].to(device))
    got = ops_pm.mlp(x, w, None if o["bias"] is None else o["bias"].to(device), act, out=_slice(out_wide, cout),
                     tile_hint=ops_pm.SPLIT_FORM, w_split=w3, **kw)
    return got, out_wide


def _check(got, want, label):
    got = got.double().cpu()
    assert got.shape == want.shape and not bool(torch.isnan(got).any()), (label, "NaN in the result")
    bar = 1e-5 * float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"{label}: err / bar = {err / bar:.3f}")
    assert err <= bar, (label, err, bar)


# rows: 1, 255, 257, 513 (ragged first / last tiles, tiles on different XCD slots); cout: 4, 132, 260, 516 (ragged channel tiles, a third
# one); K: 64 (two steps), 96 (odd), 160, 1024 (the two-stage ring wraps 16 times)
SHAPES = [(1, 4, 64), (255, 132, 96), (257, 260, 160), (513, 516, 1024), (513, 4, 96), (1, 516, 160), (257, 132, 1024), (255, 260, 64)]
EPILOGUES = [(act, bias, extra) for act in (0, 1, 2) for bias in (False, True) for extra in (None, "add", "gather32", "gather64")]


def _one_case(device, rows, cout, K, act, bias, extra):
    label = f"{rows}x{cout}x{K} act{act} bias{int(bias)} {extra}"
    o = _operands(rows, cout, K, bias, extra, seed=rows * 7 + cout * 3 + K + act)
    got, wide = _run(o, act, device)
    again, _ = _run(o, act, device)
    _check(got, _want64(o, act), label)
    assert torch.equal(got, again), (label, "two runs differ")
    assert bool(torch.isnan(wide[..., :LEFT]).all() and torch.isnan(wide[..., LEFT + cout:]).all()), (label, "columns beside out were written")
    print(f"{label}: ulps from the CPU restatement = {ref.ulps(got.cpu().contiguous(), _restated(o, act).contiguous())}")


@pytest.mark.parametrize("rows,cout,K", SHAPES)
def test_split_form_at_the_tile_seams(device, rows, cout, K):
    """bias + ReLU and the bare product at every seam shape; float64 bar, equal bits across two runs, NaN neighbours of `out` intact"""
    _one_case(device, rows, cout, K, 1, True, None)
    _one_case(device, rows, cout, K, 0, False, None)


@pytest.mark.parametrize("act,bias,extra", EPILOGUES)
def test_split_form_epilogue_features(device, act, bias, extra):
    """every activation with and without bias, `add`, `gather` with int32 and int64 indices, on 3 frames of 86 / 129 rows"""
    _one_case(device, 258 if extra else 387, 132, 96, act, bias, extra)


def test_presplit_weight_images_are_exact_and_reusable(device):
    """split_weight on the device equals the CPU split part for part (so w == the sum of its images exactly), and a launch with the
    cached images carries the bits of a launch that splits on the fly"""
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(132, 96, generator=gen) * torch.exp(3.0 * torch.randn(132, 1, generator=gen))
    w3 = ops_pm.split_weight(w.to(device))
    assert w3.dtype == torch.bfloat16 and tuple(w3.shape) == (3, 132, 96)
    for got, want in zip(w3.float().cpu(), ref.split3(w)):
        assert torch.equal(got, want)
    o = _operands(257, 132, 96, True, None, seed=9)
    o["w"] = w
    assert torch.equal(_run(o, 1, device, w3=w3)[0], _run(o, 1, device)[0])


@pytest.mark.parametrize("G,R,K", [(3, 128, 128), (36, 128, 256), (3, 384, 256), (36, 384, 128)])
def test_batched_entry_equals_separate_launches(device, G, R, K):
    """rows_per_w = 128 / 384 with 3 / 36 matrices, cout 256: every matrix's rows carry the bits of a launch of their own; float64 bar;
    and with the rows ending inside the last matrix the rest of `out` stays untouched"""
    gen = torch.Generator().manual_seed(G * R + K)
    x = torch.randn(G, R, K, generator=gen)
    w = torch.randn(G, 256, K, generator=gen) / K ** 0.5
    xd, wd = x.to(device), w.to(device)
    w3 = ops_pm.split_weight(wd)
    got = ops_pm.mlp_batched(xd, wd, tile_hint=ops_pm.SPLIT_FORM, w_split=w3)
    _check(got, torch.einsum("grk,gck->grc", x.double(), w.double()), f"batched {G}x{R}x{K}")
    for g in range(G):
        assert torch.equal(got[g], ops_pm.mlp(xd[g], wd[g], tile_hint=ops_pm.SPLIT_FORM)), g
    rows = G * R - 100
    part = torch.full((G, R, 256), float("nan"), device=device)
    ops_pm.mlp_batched(xd, wd, out=part, tile_hint=ops_pm.SPLIT_FORM, w_split=w3, rows=rows)
    flat = part.view(G * R, 256)
    assert torch.equal(flat[:rows], got.view(G * R, 256)[:rows]) and bool(torch.isnan(flat[rows:]).all())


def test_launches_outside_the_domain_are_refused_with_out_untouched(device):
    """one case just outside each documented constraint of ffb6d_mlp_pm_split_f32: a second source, a gathered operand, a single
    32-k step, K not a multiple of 32, cout not a multiple of 4, the log-softmax epilogue, rows that are not 16-byte aligned"""
    gen = torch.Generator().manual_seed(3)

    def refused(K=64, cout=8, act=0, **kw):
        x = torch.randn(2, 40, K, generator=gen).to(device)
        w = torch.randn(cout, K + (kw["x2"].shape[-1] if "x2" in kw else 0), generator=gen).to(device)
        lead = kw["x1_gather"].shape if "x1_gather" in kw else (2, 40)
        out = torch.full(tuple(lead) + (cout,), 7.0, device=device)
        with pytest.raises(_lib.FFB6DNativeError):
            ops_pm.mlp(x, w, None, act, out=out, tile_hint=ops_pm.SPLIT_FORM, **{k: v.to(device) for k, v in kw.items()})
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())

    refused(x2=torch.randn(2, 40, 32, generator=gen))
    refused(x1_gather=torch.randint(0, 40, (2, 24), generator=gen))
    refused(K=32)
    refused(K=80)
    refused(cout=6)
    refused(act=ops_pm.ACT_LOG_SOFTMAX)
    # a row stride of 66 floats: rows_view would copy such a tensor, so the C entry is called directly
    lib = _lib.load()
    x = torch.randn(40, 66, generator=gen).to(device)
    w3 = ops_pm.split_weight(torch.randn(8, 64, generator=gen).to(device))
    out = torch.full((40, 8), 7.0, device=device)
    rc = lib.ffb6d_mlp_pm_split_f32(w3.data_ptr(), None, x.data_ptr(), 64, 66, None, 0, None, 0, 0, None, 0, None, 0, 0, 40,
                                    out.data_ptr(), 8, 40, 8, 0, 0, None)
    torch.cuda.synchronize()
    assert rc != 0 and bool((out == 7.0).all())


@pytest.mark.parametrize("shape", [(2, 13, 18, 256, 256), (3, 23, 30, 512, 512)])
def test_whole_winograd_convolution_through_the_split_form_against_float64(device, shape):
    """input transform -> batched GEMM in the split-bf16 form -> output transform + BN + residual + ReLU, as forward_pm.conv_wino chains
    them for a routed layer, against F.conv2d in float64: the per-operator bar, 1e-5 of range"""
    import torch.nn.functional as F
    from ffb6d_amd import forward_pm, ops
    B, H, W, C, O = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, w = torch.randn(B, H, W, C, generator=g).to(device), (torch.randn(O, C, 3, 3, generator=g) / (9 * C) ** .5).to(device)
    scale, shift, res = (torch.rand(O, generator=g) + .5).to(device), torch.randn(O, generator=g).to(device), torch.randn(B, H, W, O, generator=g).to(device)
    conv = torch.nn.Conv2d(C, O, 3, 1, 1, bias=False).to(device)
    with torch.no_grad():
        conv.weight.copy_(w)
        u3 = forward_pm.wino4_split_weights(conv)
        assert forward_pm.wino4_split_weights(conv) is u3                       # cached under the weight's version ...
        mm = ops_pm.mlp_batched(ops_pm.wino4_input(x), forward_pm.wino4_weights(conv), tile_hint=ops_pm.SPLIT_FORM, w_split=u3)
        got = ops_pm.wino4_output(mm, (B, H, W), scale, shift, act=ops.ACT_RELU, residual=res)
        conv.weight.mul_(2.0)                                                   # ... and split again after an in-place edit
        u3b = forward_pm.wino4_split_weights(conv)
        assert u3b is not u3 and torch.equal(u3b, ops_pm.split_weight(forward_pm.wino4_weights(conv)))
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)
    want = torch.relu(y * scale.double() + shift.double() + res.double())
    err = float((got.double() - want).abs().max() / want.abs().max())
    print(shape, "F(4x4) convolution with the split-bf16 GEMM against float64: max err / range %.2e" % err)
    assert err <= 1e-5


def test_forward_with_the_split_form_agrees_with_off(device, monkeypatch):
    """the whole forward with every launch in the form's domain routed to it (the rule's size thresholds lifted: at 1 x 240 x 320 no
    layer is large enough for it) against the forward with the form off: every output and stage tap within HOT_TOL = 1e-5 of range;
    the form is asked for where the rule says and nowhere else, and off means no launch takes it"""
    import json
    import os
    from ffb6d_amd import forward_pm, model as M, pyramid, synth
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(golden, "state_dict_keys.json")) as fh:
        shapes = json.load(fh)
    net = M.FFB6D(n_classes=5, n_pts=1024)
    net.load_state_dict(synth.synth_state_dict_from_shapes(shapes, seed=0, n_classes=5))
    net = net.to(device).eval()
    inputs = pyramid.frames_to_device(synth.make_batch(7, 1, n_points=1024, height=240, width=320), device)
    taken = []
    real = {n: getattr(_lib.load(), n) for n in ("ffb6d_mlp_pm_split_f32", "ffb6d_mlp_pm_split_batched_f32")}
    lib = _lib.load()
    for n, fn in real.items():
        monkeypatch.setattr(lib, n, lambda *a, n=n, fn=fn: (taken.append(n), fn(*a))[1])

    def run(on):
        monkeypatch.setattr(forward_pm, "GEMM_SPLIT_FORM", on)
        monkeypatch.setattr(forward_pm, "gemm_split_takes",
                            lambda rows, cout, K, act=0: forward_pm.GEMM_SPLIT_FORM and K % 32 == 0 and K >= 64 and cout % 4 == 0 and 0 <= int(act) <= 2)
        taken.clear()
        taps = {}
        with torch.no_grad():
            ep = dict(net(inputs, taps=taps))
        ep.update(taps)
        return {k: v.clone() for k, v in ep.items() if torch.is_tensor(v) and v.is_floating_point()}, list(taken)

    off, n_off = run(False)
    on, n_on = run(True)
    assert not n_off
    assert n_on.count("ffb6d_mlp_pm_split_batched_f32") == 17 and n_on.count("ffb6d_mlp_pm_split_f32") >= 3, n_on
    for k in sorted(off):
        err = float((on[k].double() - off[k].double()).abs().max() / off[k].double().abs().max())
        print(k, "split-bf16 form on against off: max err / range %.2e" % err)
        assert err <= 1e-5, k
