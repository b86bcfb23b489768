"""Deterministic case tables for the point-major GEMM family (ffb6d_amd/ops_pm.py: mlp, mlp_batched; csrc/mlp_pm.hip,
mlp_pm_big.hip) -- every kernel FORM against every OPERAND FEATURE (tests/test_pm_forms_gpu.py, test_pm_forms_cpu.py).  No tests
live here, and nothing is random at run time: the tables are drawn from fixed seeds when the module is imported.

Forms (tile_hint): t1 .. t5 the tile kernels (1 .. 5), stream (6), lds (7), seq (8 + 256 * plan: group plans SEQ(..) and balanced
plans LIN(..)), big (9 + 256 * channel tiles per workgroup), and the batched-weight entry (BATCHED below).  Each has its own loader,
prefetch and epilogue code and must honour the same operand features, the AXES of a case:

    dt          f32 / bf16
    src2        a second source (K2 > 0)
    x1_gather   x1 rows picked by index in the load (`choose`)
    epi         none / gather (Y[b, idx[b, p]] added) / add (Y[b, p] added)
    bias        present / missing
    act         0 none, 1 relu, 2 leaky 0.2, 3 log-softmax (the forms that have that epilogue)
    in_slice    every row operand (x1, x2, Y) is a channel slice of a wider buffer: row stride > row
    out_slice   `out` is a channel slice of a wider buffer: ldo > cout
    bits        int32 / int64 indices (cases with an index array)
    hint        the plans of seq and big
    sched       seq, big: what the plan makes of the shape (seq_schedule), * = some workgroup multiplies several tiles in a row
    rag_rows / rag_cout / n_pt / n_ct    ragged last point / channel tile, one or several tiles each way

DOMAIN.  in_domain(case) restates what the host code accepts (csrc/mlp_pm.hip: the FFB6D_REQUIREs of mlp_pm_impl, stream_form_ok,
seq_form_ok; csrc/mlp_pm_big.hip: big_form_ok) for the aligned buffers operands() builds.  KSTEP = 8 (f32) / 16 (bf16) elements,
a 128-byte segment SEG = 32 / 64 elements:
    every form  k1, k2 multiples of KSTEP; log-softmax needs cout <= 64, cout % 4 == 0
    t1 .. t5    nothing more; log-softmax only where a wave's tile spans all channels: t2 (cout <= 64), t3 (cout <= 32)
    stream      cout <= 128, cout * SZ % 16 == 0, 3 KSTEP <= K <= 16 KSTEP, no x1_gather, log-softmax from one source only
    lds         k1 and K whole segments, no log-softmax
    seq         f32 only, lds's conditions, K >= 128 (four segments), cout % 4 == 0
    big         bf16 only, lds's conditions, K >= 128 (two segments), cout % 16 == 0
CASES is drawn inside the domain only; REJECTED holds one case just outside it per documented constraint.

COVERAGE.  Per (form, dtype) 400 candidates are drawn and a greedy cover keeps the few that between them hold every value of every
axis AND every pair of values of two feature axes (src2 x x1_gather, epi x in_slice, hint x bits, ...: a loader that forgets the row
stride only when it also gathers shows in a pair, not in either value alone), plus the "everything at once" case of the form.
required(form) is the list of (axis, value) the table must hold per form; test_pm_forms_cpu.py counts them."""
import collections
import itertools
import random

import torch

from test_pm_gpu import LIN, SEQ        # the plan encodings of the tile-sequence form

Case = collections.namedtuple("Case", "form hint dt B P K1 K2 cout act bias epi py x1g bits in_slice out_slice seed")
# epi: "none" / "gather" / "add"; py: rows per frame of a gathered Y; x1g: rows per frame of a gathered x1 (0 = plain rows);
# bits: 32 / 64 (0 = the case has no index array)

FORMS = ("t1", "t2", "t3", "t4", "t5", "stream", "lds", "seq", "big")
HINTS = {"t1": (1,), "t2": (2,), "t3": (3,), "t4": (4,), "t5": (5,), "stream": (6,), "lds": (7,),
         "seq": (SEQ(2), SEQ(3), SEQ(4, 2, 1, 1), LIN(1), LIN(2, 3)), "big": (9, 9 + 256, 9 + 512)}
DTYPES = {f: ("f32", "bf16") for f in FORMS}
DTYPES.update(seq=("f32",), big=("bf16",))
# (point rows, channels) of one tile of the form: what "ragged" and "several tiles" mean for it (stream: 32 rows per wave, all channels)
TILE = {"t1": (128, 128), "t2": (256, 64), "t3": (256, 32), "t4": (64, 64), "t5": (32, 64), "stream": (128, 128), "lds": (128, 128),
        "seq": (128, 128), "big": (256, 256)}
ROWS = (1, 63, 128, 129, 257, 300)
FRAMES = (1, 2, 3)
# the tile-sequence form only: below 8 point tiles (1024 rows) launch_seq leaves every tile a single one, whatever the plan (seq_schedule
# below), and a three-region plan needs 24; a balanced sequence crosses into the next point tile of its XCD from 9 on
SEQ_ROWS = 1100
COUTS = {"tile": (1, 2, 3, 5, 31, 32, 33, 37, 63, 64, 65, 72, 127, 128, 129, 136, 200, 255, 256, 257, 260),
         "stream": (8, 16, 24, 32, 40, 56, 64, 72, 96, 120, 128),
         "lds": (8, 31, 32, 33, 37, 63, 64, 65, 72, 127, 128, 129, 136, 200, 255, 256, 257, 260),
         "seq": (4, 32, 36, 64, 68, 124, 128, 132, 136, 200, 256, 260, 392, 516),       # 516: five channel tiles, a sequence of four + one
         "big": (16, 48, 64, 80, 128, 144, 192, 256, 272, 528)}                          # 528: three channel tiles of 256
FEATURE_AXES = ("dt", "src2", "x1_gather", "epi", "bias", "act", "in_slice", "out_slice", "bits", "hint", "sched")
SHAPE_AXES = ("rag_rows", "rag_cout", "n_pt", "n_ct", "P", "B")


def kstep(dt):
    return 8 if dt == "f32" else 16


def seg(dt):
    return 32 if dt == "f32" else 64


def in_domain(c):
    """What the host code accepts for this form (see the module docstring), given operands() buffers: 16-byte aligned slices whose row
    strides are multiples of 8 elements."""
    ks, sg, K = kstep(c.dt), seg(c.dt), c.K1 + c.K2
    if c.hint not in HINTS[c.form]:
        return False
    if c.K1 < ks or c.K1 % ks or c.K2 % ks or c.cout < 1 or c.act not in (0, 1, 2, 3):
        return False
    if c.act == 3 and (c.cout > 64 or c.cout % 4):
        return False
    if c.form in ("t1", "t2", "t3", "t4", "t5"):
        return c.act != 3 or (c.form == "t2") or (c.form == "t3" and c.cout <= 32)
    if c.form == "stream":
        return c.cout <= 128 and c.cout % (4 if c.dt == "f32" else 8) == 0 and 3 * ks <= K <= 16 * ks and not c.x1g and \
            not (c.act == 3 and c.K2)
    whole = c.act != 3 and K % sg == 0 and c.K1 % sg == 0
    if c.form == "lds":
        return whole
    if c.form == "seq":
        return whole and c.dt == "f32" and K >= 128 and c.cout % 4 == 0
    if c.form == "big":
        return whole and c.dt == "bf16" and K >= 128 and c.cout % 16 == 0
    raise ValueError(c.form)


def seq_schedule(rows, cout, plan, gathered):
    """launch_seq (csrc/mlp_pm.hip) restated: how a plan cuts the 128 x 128 tiles of a launch into the sequences one workgroup multiplies.
    Returns (kind, longest sequence): kind "A" / "B" / "C" strung together for the regions of a group plan that hold point tiles (region
    C: single tiles; regions A and B begin on multiples of 8 point tiles, so below 8 point tiles EVERY tile is a single one and the riding
    epilogue of mlp_pm_seq_kernel never runs), "lin" for balanced sequences, "lin+" when one of them runs from a point tile into the
    next.  A LIN plan with gathered x1 rows (or more than 8 channel tiles) is run as the group plan 2."""
    n_ct, n_pt = -(-cout // 128), -(-rows // 128)
    if (plan >> 4) & 15 == 15 and n_ct <= 8 and not gathered:
        L = -(-n_pt // 8) * n_ct
        lin_wg = min(64 * max(1, min(plan & 15, 15)), L)
        if (plan >> 8) & 255:
            lin_wg = min((plan >> 8) & 255, L)
        longest, cross = 1, False
        for xcd in range(8):
            Lx = ((n_pt - xcd + 7) >> 3) * n_ct
            base, rem = divmod(Lx, lin_wg)
            for j in range(lin_wg):
                start, n = j * base + min(j, rem), base + (j < rem)
                longest = max(longest, n)
                cross |= start % n_ct + n > n_ct
        return ("lin+" if cross else "lin"), longest
    if (plan >> 4) & 15 == 15:
        plan = 2
    tpg = max(1, min(plan & 15, n_ct, 8))
    tpg_b = max(1, min((plan >> 4) & 15, tpg))
    tiles_b, tiles_c = ((plan >> 8) & 255) * 16, ((plan >> 16) & 127) * 16
    pts_c = min(n_pt, -(--(-tiles_c // n_ct) // 8) * 8)
    pts_b = min(n_pt - pts_c, -(--(-tiles_b // n_ct) // 8) * 8)
    pt_c = n_pt - pts_c
    pt_b = pt_c - pts_b
    pt_b -= pt_b % 8
    if pt_c % 8 and pt_c > pt_b:
        pt_c -= pt_c % 8
    pt_c = max(pt_c, pt_b)
    kind = ("A" if pt_b > 0 else "") + ("B" if pt_c > pt_b else "") + ("C" if n_pt > pt_c else "")
    return kind, max((tpg if pt_b > 0 else 1), (tpg_b if pt_c > pt_b else 1))


def features(c):
    """axis -> value of one case (bits only where there is an index array, x1_gather not for the stream form, which has none; sched, the
    forms that multiply sequences of tiles: what the plan makes of this shape, and whether any workgroup gets more than one tile)"""
    tp, tc = TILE[c.form]
    if c.form == "stream":
        tc = 32 if c.cout <= 32 else (64 if c.cout <= 64 else 128)
    rows = c.B * c.P
    f = dict(dt=c.dt, src2=int(c.K2 > 0), epi=c.epi, bias=int(c.bias), act=c.act, in_slice=int(c.in_slice), out_slice=int(c.out_slice),
             hint=c.hint, rag_rows=int(rows % tp != 0), rag_cout=int(c.cout % tc != 0), n_pt=min(2, -(-rows // tp)), P=c.P, B=c.B)
    if c.form != "stream":
        f["x1_gather"] = int(c.x1g > 0)
        f["n_ct"] = min(2, -(-c.cout // tc))
    if c.bits:
        f["bits"] = c.bits
    if c.form == "seq":
        kind, longest = seq_schedule(rows, c.cout, c.hint >> 8, c.x1g > 0)
        f["sched"] = kind + ("*" if longest > 1 else "")
    if c.form == "big":                                    # csrc/mlp_pm_big.hip: (hint >> 8) & 15 channel tiles of one point tile per workgroup
        f["sched"] = "*" if (c.hint >> 8) >= 2 and c.cout > 256 else ""
    return f


def required(form):
    """(axis, value) pairs the table must hold for `form`"""
    acts = (0, 1, 2, 3) if form in ("t2", "t3", "stream") else (0, 1, 2)
    req = dict(dt=DTYPES[form], src2=(0, 1), epi=("none", "gather", "add"), bias=(0, 1), act=acts, in_slice=(0, 1), out_slice=(0, 1),
               bits=(32, 64), hint=HINTS[form], rag_rows=(0, 1), rag_cout=(0, 1), n_pt=(1, 2), P=ROWS, B=FRAMES)
    if form != "stream":
        req.update(x1_gather=(0, 1), n_ct=(1, 2))
    if form == "seq":
        req.update(sched=("C", "A*", "AC*", "ABC*", "lin", "lin*", "lin+*"), P=ROWS + (SEQ_ROWS,))
    if form == "big":
        req.update(sched=("", "*"))
    return [(a, v) for a, vs in req.items() for v in vs]


def is_everything(c):
    """x1_gather + gathered epilogue + second source + int32 + every operand and `out` a slice + no bias (the stream form: all but
    x1_gather)"""
    return (c.x1g > 0 or c.form == "stream") and c.epi == "gather" and c.K2 > 0 and c.bits == 32 and c.in_slice and c.out_slice and not c.bias


def _draw(rng, form, dt, everything=False):
    ks, sg = kstep(dt), seg(dt)
    src2 = everything or rng.random() < 0.5
    if form in ("lds", "seq", "big"):
        lo = 1 if form == "lds" else 128 // sg
        n = rng.randint(max(lo, 2 if src2 else 1), 256 // sg)
        n1 = rng.randint(1, n - 1) if src2 else n
        K1, K2 = n1 * sg, (n - n1) * sg
    else:
        n = rng.randint(max(3 if form == "stream" else 1, 2 if src2 else 1), min(16, 256 // ks))
        n1 = rng.randint(1, n - 1) if src2 else n
        K1, K2 = n1 * ks, (n - n1) * ks
    cout = rng.choice(COUTS[form if form in COUTS else "tile"])
    if form == "stream" and dt == "bf16":
        cout = -(-cout // 8) * 8
    act = rng.choice((0, 1, 2))
    if form in ("t2", "t3", "stream") and not everything and rng.random() < 0.25:
        act = 3
        if form == "stream":
            K1, K2 = K1 + K2, 0
        cout = rng.choice((4, 12, 32) if form == "t3" else (4, 12, 32, 36, 64)) if form != "stream" else rng.choice((8, 16, 32, 40, 64))
    x1g = rng.choice((1, 50, 333)) if (everything or rng.random() < 0.4) and form != "stream" else 0
    epi = "gather" if everything else rng.choice(("none", "gather", "add"))
    py = rng.choice((1, 7, 40)) if epi == "gather" else 0
    bits = (32 if everything else rng.choice((32, 64))) if (x1g or epi == "gather") else 0
    P = SEQ_ROWS if form == "seq" and rng.random() < 0.4 else rng.choice(ROWS)
    c = Case(form, rng.choice(HINTS[form]), dt, rng.choice(FRAMES), P, K1, K2, cout, act,
             bias=not everything and rng.random() < 0.6, epi=epi, py=py, x1g=x1g, bits=bits,
             in_slice=everything or rng.random() < 0.5, out_slice=everything or rng.random() < 0.5, seed=rng.randrange(1 << 30))
    assert in_domain(c), c
    return c


def _items(c):
    """what a case contributes to the cover: its axis values, and the pairs of values of two feature axes"""
    f = features(c)
    single = {(a, v) for a, v in f.items()}
    feat = sorted((a, f[a]) for a in FEATURE_AXES if a in f)
    return single | {(x, y) for x, y in itertools.combinations(feat, 2)}


def _cover(cands, chosen):
    items = [_items(c) for c in cands]
    todo = set().union(*items) - set().union(*[_items(c) for c in chosen])
    chosen = list(chosen)
    while todo:
        best = max(range(len(cands)), key=lambda i: len(items[i] & todo))         # the first of equals: deterministic
        chosen.append(cands[best])
        todo -= items[best]
    return chosen


def candidates(form):
    """(the "everything at once" case once per dtype and plan of the form, 400 draws from the domain per dtype)"""
    ev, cands = [], []
    for di, dt in enumerate(DTYPES[form]):
        rng = random.Random(1000 * FORMS.index(form) + di + 17)
        ev += [_draw(rng, form, dt, everything=True)._replace(hint=h) for h in HINTS[form]]
        cands += [_draw(rng, form, dt) for _ in range(400)]
    return ev, cands


def _table():
    cases = []
    for form in FORMS:
        ev, cands = candidates(form)
        cases += _cover(cands, ev)
    return cases


CASES = _table()


def case_id(c):
    h = {SEQ(2): "seq2", SEQ(3): "seq3", SEQ(4, 2, 1, 1): "seq4211", LIN(1): "lin1", LIN(2, 3): "lin2_3"}.get(c.hint, str(c.hint & 255) + (
        "p%d" % (c.hint >> 8) if c.hint >> 8 else ""))
    return (f"{c.form}-h{h}-{c.dt}-{c.B}x{c.P}-k{c.K1}+{c.K2}-c{c.cout}-a{c.act}{'b' if c.bias else ''}-{c.epi}{c.py or ''}"
            f"{'-xg%d' % c.x1g if c.x1g else ''}{'-i%d' % c.bits if c.bits else ''}{'-in' if c.in_slice else ''}{'-out' if c.out_slice else ''}")


# ---------------------------------------------------------------------------------------------------------------------------------
# operands and the float64 reference
# ---------------------------------------------------------------------------------------------------------------------------------
NAN = float("nan")


def nan_slice(t, sliced, left=8):
    """(view, wide): `t` itself (wide = None), or a copy of it that is the channels [left, left + C) of a wider buffer whose other
    columns are NaN: 16-byte aligned in both precisions, row stride a multiple of 8 elements and > C"""
    if not sliced:
        return t, None
    C = t.shape[-1]
    wide = torch.full(tuple(t.shape[:-1]) + (left + -(-C // 8) * 8 + 8,), NAN, dtype=t.dtype)
    wide[..., left:left + C] = t
    return wide[..., left:left + C], wide


def operands(c, dt=None):
    """CPU tensors of a case: x1, x2, w, bias, add / gather, x1_gather as ops_pm.mlp takes them (slices where the case says so), `out`
    NaN-prefilled, and `out_wide` (the buffer `out` is a slice of, or None).  `dt` overrides the case's dtype (the rejected cases)."""
    tdt = torch.float32 if (dt or c.dt) == "f32" else torch.bfloat16
    g = torch.Generator().manual_seed(c.seed)
    r = lambda *s: torch.randn(*s, generator=g).to(tdt)                               # noqa: E731
    K = c.K1 + c.K2
    o = dict(x1=nan_slice(r(c.B, c.x1g or c.P, c.K1), c.in_slice)[0], x2=None, bias=None, add=None, gather=None, x1_gather=None)
    if c.K2:
        o["x2"] = nan_slice(r(c.B, c.P, c.K2), c.in_slice, left=16)[0]
    o["w"] = (torch.randn(c.cout, K, generator=g) / K ** 0.5).to(tdt)
    if c.bias:
        o["bias"] = torch.randn(c.cout, generator=g)
    it = torch.int32 if c.bits == 32 else torch.int64
    if c.x1g:
        o["x1_gather"] = torch.randint(0, c.x1g, (c.B, c.P), generator=g).to(it)
    if c.epi == "gather":
        o["gather"] = (nan_slice(r(c.B, c.py, c.cout), c.in_slice)[0], torch.randint(0, c.py, (c.B, c.P), generator=g).to(it))
    elif c.epi == "add":
        o["add"] = nan_slice(r(c.B, c.P, c.cout), c.in_slice)[0]
    o["out"], o["out_wide"] = nan_slice(torch.full((c.B, c.P, c.cout), NAN, dtype=tdt), c.out_slice)
    return o


def reference(o, act):
    """float64 from the operands as they are (bf16 operands: their rounded values)"""
    x1 = o["x1"].double()
    if o["x1_gather"] is not None:
        x1 = torch.gather(x1, 1, o["x1_gather"].long().unsqueeze(2).expand(-1, -1, x1.shape[2]))
    x = x1 if o["x2"] is None else torch.cat([x1, o["x2"].double()], dim=-1)
    y = x @ o["w"].double().t()
    if o["bias"] is not None:
        y = y + o["bias"].double()
    if o["gather"] is not None:
        Y, idx = o["gather"]
        y = y + torch.gather(Y.double(), 1, idx.long().unsqueeze(2).expand(-1, -1, Y.shape[2]))
    if o["add"] is not None:
        y = y + o["add"].double()
    if act == 1:
        y = torch.relu(y)
    elif act == 2:
        y = torch.nn.functional.leaky_relu(y, 0.2)
    elif act == 3:
        y = torch.log_softmax(y, dim=-1)
    return y


# ---------------------------------------------------------------------------------------------------------------------------------
# just outside the domain: one case per documented constraint.  (name, case, dtype of the tensors); every one is refused by the host
# code before anything is launched
# ---------------------------------------------------------------------------------------------------------------------------------
def _c(form, hint, dt, K1, K2, cout, act=1, x1g=0, **kw):
    d = dict(B=2, P=129, bias=True, epi="none", py=0, bits=32 if x1g else 0, in_slice=False, out_slice=True, seed=7)
    d.update(kw)
    return Case(form=form, hint=hint, dt=dt, K1=K1, K2=K2, cout=cout, act=act, x1g=x1g, **d)


REJECTED = [
    ("tile: k1 no multiple of KSTEP", _c("t1", 1, "f32", 12, 0, 16)),
    ("tile: k2 no multiple of KSTEP (bf16: 16)", _c("t4", 4, "bf16", 16, 8, 16)),
    ("tile: log-softmax over more than 64 channels", _c("t2", 2, "f32", 32, 0, 68, act=3)),
    ("tile: log-softmax over a channel count that is no multiple of 4", _c("t3", 3, "f32", 32, 0, 30, act=3)),
    ("stream: x1_gather", _c("stream", 6, "f32", 64, 0, 64, x1g=50)),
    ("stream: cout > 128", _c("stream", 6, "f32", 64, 0, 136)),
    ("stream: K < 3 KSTEP", _c("stream", 6, "f32", 16, 0, 64)),
    ("stream: K > 16 KSTEP", _c("stream", 6, "bf16", 256, 16, 64)),
    ("stream: cout rows that are no whole 16 bytes", _c("stream", 6, "f32", 64, 0, 30)),
    ("stream: log-softmax from two sources", _c("stream", 6, "f32", 32, 32, 32, act=3)),
    ("lds: k1 of 96 bytes", _c("lds", 7, "f32", 24, 8, 72)),
    ("lds: K no whole 128-byte segments", _c("lds", 7, "bf16", 64, 32, 72)),
    ("lds: log-softmax", _c("lds", 7, "f32", 64, 0, 32, act=3)),
    ("seq: bf16", _c("seq", SEQ(2), "bf16", 128, 0, 136)),
    ("seq: K < 128", _c("seq", SEQ(2), "f32", 96, 0, 136)),
    ("seq: cout % 4 != 0", _c("seq", SEQ(2), "f32", 128, 0, 134)),
    ("seq: k1 no whole segments", _c("seq", LIN(1), "f32", 144, 112, 136)),
    ("seq: log-softmax", _c("seq", SEQ(2), "f32", 128, 0, 64, act=3)),
    ("big: fp32", _c("big", 9, "f32", 128, 0, 256)),
    ("big: K < 128", _c("big", 9, "bf16", 64, 0, 256)),
    ("big: cout % 16 != 0", _c("big", 9 + 256, "bf16", 128, 0, 72)),
    ("big: k1 no whole segments", _c("big", 9, "bf16", 96, 32, 256)),
    ("big: log-softmax", _c("big", 9, "bf16", 128, 0, 64, act=3)),
    ("unknown form", _c("t1", 10, "f32", 32, 0, 16)),
]

# ---------------------------------------------------------------------------------------------------------------------------------
# the batched-weight entry (ops_pm.mlp_batched; fp32): (G, R, K, cout, hint) -- every G with every hint, every R and K, ragged channel
# counts (cout % 4 == 0) with one, two and more channel tiles
# ---------------------------------------------------------------------------------------------------------------------------------
BATCHED_HINTS = (0, 7, SEQ(2), SEQ(3))
BATCHED = [(1, 128, 128, 4, 0), (1, 384, 256, 392, 7), (1, 128, 160, 516, SEQ(2)), (1, 384, 128, 136, SEQ(3)),
           (2, 384, 160, 132, 7), (2, 128, 128, 260, SEQ(2)), (2, 128, 256, 200, SEQ(3)), (2, 384, 128, 392, 0),
           (16, 128, 256, 64, SEQ(2)), (16, 384, 160, 36, SEQ(3)), (16, 128, 128, 132, 0), (16, 128, 160, 260, 7),
           (36, 128, 128, 136, SEQ(3)), (36, 384, 128, 128, 0), (36, 128, 160, 68, 7), (36, 128, 256, 132, SEQ(2))]
BATCHED_REJECTED = [("R = 64", 2, 64, 128, 64, 0), ("R no multiple of 128", 2, 192, 128, 64, 7), ("a LIN plan", 2, 128, 128, 256, LIN(1)),
                    ("the stream form", 2, 128, 128, 64, 6), ("the tile kernels", 2, 128, 128, 64, 1), ("K < 128", 2, 128, 96, 64, 0),
                    ("K no whole segments", 2, 128, 136, 64, 7), ("cout % 4 != 0", 2, 128, 128, 66, SEQ(2))]

# ---------------------------------------------------------------------------------------------------------------------------------
# the automatic choice (tile_hint 0) on both sides of every threshold of ffb6d_mlp_pm_choice / ffb6d_mlp_pm_tile:
# (what, rows, cout, k1, k2, act, bf16, x1_gathered, form)  -- form = ffb6d_mlp_pm_choice(...) & 255, asserted in test_pm_forms_cpu.py
# ---------------------------------------------------------------------------------------------------------------------------------
BOUNDARIES = [
    # the stream form: >= 16384 rows, 96 .. 512-byte rows, cout <= 128 in whole 16 bytes, plain rows, two sources in bf16 only
    ("stream: rows", 16383, 8, 24, 0, 1, 0, 0, 5), ("stream: rows", 16384, 8, 24, 0, 1, 0, 0, 6),
    ("stream: row bytes >= 96", 16384, 8, 16, 0, 1, 0, 0, 5), ("stream: row bytes <= 512", 16384, 8, 136, 0, 1, 0, 0, 5),
    ("stream: row bytes <= 512", 16384, 8, 128, 0, 1, 0, 0, 6),
    ("stream: cout <= 128", 16384, 128, 64, 0, 2, 0, 0, 6), ("stream: cout <= 128", 16384, 132, 24, 0, 2, 0, 0, 4),
    ("stream: whole 16-byte rows", 16384, 10, 24, 0, 0, 0, 0, 5), ("stream: gathered x1", 16384, 8, 24, 0, 1, 0, 1, 5),
    ("stream: two sources, fp32", 16384, 16, 24, 24, 1, 0, 0, 5), ("stream: two sources, bf16", 16384, 16, 32, 32, 1, 1, 0, 6),
    ("stream: log-softmax", 16384, 32, 64, 0, 3, 0, 0, 6), ("stream: log-softmax from two sources", 16384, 32, 32, 32, 3, 0, 0, 3),
    # the LDS-tiled form: whole segments, >= 256 tiles of 128 x 128, fp32 only with cout > 64
    ("lds: tiles", 255 * 128, 72, 32, 32, 1, 0, 0, 4), ("lds: tiles", 255 * 128 + 1, 72, 32, 32, 1, 0, 0, 7),
    ("lds: fp32 cout > 64", 32768, 64, 32, 32, 1, 0, 0, 4), ("lds: bf16 any cout", 32768, 64, 64, 0, 1, 1, 1, 7),
    ("lds: whole segments", 32768, 72, 40, 32, 1, 0, 0, 4), ("lds: k1 whole segments", 32768, 72, 48, 16, 1, 0, 0, 4),
    # the tile-sequence form: fp32, >= 512-byte rows, cout % 4 == 0, >= 1024 tiles in >= 2 channel tiles
    ("seq: tiles", 511 * 128, 136, 128, 0, 1, 0, 0, 7), ("seq: tiles", 511 * 128 + 1, 136, 128, 0, 1, 0, 0, 8),
    ("seq: row bytes", 65536, 136, 96, 0, 1, 0, 0, 7), ("seq: cout % 4", 65536, 138, 128, 0, 1, 0, 0, 7),
    ("seq: one channel tile", 131072, 128, 128, 0, 1, 0, 1, 7), ("seq: bf16", 65536, 136, 128, 0, 1, 1, 0, 7),
    # the 256 x 256 bf16 form: >= 512-byte rows, cout >= 192, >= 512 tiles of 256 x 256
    ("big: tiles", 130816, 192, 256, 0, 1, 1, 0, 7), ("big: tiles", 130817, 192, 256, 0, 1, 1, 0, 9),
    ("big: row bytes", 131072, 192, 192, 0, 1, 1, 0, 7), ("big: cout", 131072, 176, 256, 0, 1, 1, 0, 7),
    # the tile kernels
    ("tile 2: 384 blocks of 256 x 64", 383 * 256, 64, 16, 0, 1, 0, 0, 4), ("tile 2: 384 blocks", 383 * 256 + 1, 64, 16, 0, 1, 0, 0, 2),
    ("tile 1: 384 tiles of 128 x 128", 191 * 128, 136, 40, 0, 1, 0, 0, 4), ("tile 1: 384 tiles", 191 * 128 + 1, 136, 40, 0, 1, 0, 0, 1),
    ("tile 3: 256 blocks of 256 rows", 255 * 256, 32, 16, 0, 1, 0, 0, 5), ("tile 3: 256 blocks", 255 * 256 + 1, 32, 16, 0, 1, 0, 0, 3),
    ("tile 3 / 2: cout 32 | 33", 255 * 256 + 1, 33, 16, 0, 1, 0, 0, 4),
    ("tile 4: 512 tiles of 64 x 64", 511 * 64, 64, 136, 0, 1, 0, 0, 5), ("tile 4: 512 tiles", 511 * 64 + 1, 64, 136, 0, 1, 0, 0, 4),
    ("tile 4: K < 64", 300, 40, 56, 0, 1, 0, 0, 4), ("tile 5: K >= 64", 300, 40, 64, 0, 1, 0, 0, 5),
    ("log-softmax: cout <= 32", 300, 32, 64, 0, 3, 0, 0, 3), ("log-softmax: cout > 32", 300, 36, 64, 0, 3, 0, 0, 2),
]
# tile_hint 0 with rows the chosen form cannot take: mlp_pm_impl falls back (stream -> tile kernel, seq -> lds, big -> lds).
# (what, rows, cout, k1, bf16, form chosen from the shape, extra columns of the out buffer: ldo = cout + extra)
FALLBACKS = [("stream -> tile kernel: ldo no whole 16 bytes", 16384, 8, 24, 0, 6, 2),
             ("seq -> lds: ldo % 4 != 0", 65536, 136, 128, 0, 8, 2),
             ("big -> lds: ldo % 8 != 0", 131072, 192, 256, 1, 9, 4)]

# ---------------------------------------------------------------------------------------------------------------------------------
# ops_pm.lfa_half (csrc/lfa_pm.hip): (d, p_hint, N, mode, index bits, B)
# ---------------------------------------------------------------------------------------------------------------------------------
LFA_D, LFA_HINT, LFA_N = (32, 64, 128, 256), (0, 1, 2, 3, 4, 10), (1, 17, 65, 130)
# every (d, p_hint) pair; N, mode, index type and frame count drift against the hints, so that every d and every hint meets every N,
# both modes and both index types (test_pm_forms_cpu.py counts them); + 256: every other case caps the grid at one workgroup per XCD
# (p_hint bits 8 .. 15), so that a workgroup walks several point groups even at these sizes
LFA = [(d, h + 256 * ((di + hi) % 2), LFA_N[(di + hi) % 4], 1 + (di + hi // 2) % 2, (32, 64)[(di // 2 + hi) % 2], 1 + (di + 2 * hi) % 3)
       for di, d in enumerate(LFA_D) for hi, h in enumerate(LFA_HINT)]
