"""GPU tests of bd_srv_ban_rows / bd_srv_step_ban (serving_ops.ban_rows / step_ban): EXACT bits of the whole output against the restatement of
the definition (tests/ban_ref.py), in both dtypes, at four vocabulary sizes -- one vector, exactly one block, one vector into the second block,
two blocks and a vector -- so that a ban lands in the last vector of a slice and in the first vector of the next.  One launch carries rows with
different parameters: every n-gram size and history length at which the rule changes, tails and matches that straddle the ctx / out boundary,
overlapping matches, bad words of every kind, the early-stop boundary, ids outside the vocabulary, and device values the clamps must
neutralise.  Logits rows are strided and hold NaN and -0.0 at banned and kept positions; the output sits in a poisoned canary buffer; the
turn's tokens are a strided view."""
import pytest
import torch

import ban_ref as ref
from canary import POISON, CanaryOut

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
VS = [8, 2048, 2056, 4104]
LC, CAP, Q, W, NS = 12, 10, 4, 3, 3
POISON16 = POISON * 0x0101
inf, nan = float("inf"), float("nan")
SPECIAL = [nan, -0.0, -inf, inf, 0.0, 6.0e-8, -6.0e-8, 1.0e-40, 65504.0, -65504.0, 1.5]
NAN16 = {torch.float16: 0x7e00, torch.bfloat16: 0x7fc0}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib, serving_ops
    _lib.lib()
    return serving_ops


def _syms(V):
    """distinct token ids at the vector and slice boundaries of a V-element row"""
    out = []
    for y in (0, 7, 8, 2047, 2048, 2055, V - 1, V - 8, V // 2, 1, 2, 3):
        if 0 <= y < V and y not in out:
            out.append(y)
    return out


def _rows(V):
    """the rows of one launch: dicts of ctx, ctx_len, toks, n, g, words (token lists), lens (None: the words' own), min, stops"""
    s = _syms(V)
    x, y, z, w, a, b = s[:6]
    rows = []

    def row(ctx=(), toks=(), g=0, words=(), min_new=0, stops=(), ctx_len=None, n=None, lens=None):
        rows.append(dict(ctx=list(ctx), toks=list(toks), g=g, words=[list(q) for q in words], min=min_new, stops=list(stops),
                         ctx_len=len(ctx) if ctx_len is None else ctx_len, n=len(toks) if n is None else n, lens=lens))
    row()                                                                # nothing set: a bit-identical copy
    # n-gram: the match in ctx and the tail in out; the tail straddling the boundary; matches straddling the boundary
    row(ctx=[x, y, z], toks=[x, y], g=3)
    row(ctx=[x, y, z, x], toks=[y], g=3)
    row(ctx=[x, y], toks=[z, w, x, y], g=3)
    row(ctx=[w, x], toks=[y, z, x, y], g=3)
    row(ctx=[x, y, z, w, x, y, a, b, x], toks=[y], g=2)                 # several followers of one token
    for g in (1, 2, 3, 8):                                               # m = 0, g - 2, g - 1, g with one repeated token: banned from m = g on
        for m in sorted({0, max(g - 2, 0), g - 1, g}):
            row(ctx=[a] * (m // 2), toks=[a] * (m - m // 2), g=g)
    row(ctx=[x, y], toks=[z], g=1)                                       # g = 1: the whole history
    row(ctx=[a, a], toks=[a, a], g=2)                                    # overlapping matches
    row(ctx=[a, a, a, a, a], toks=[a, a, a, a], g=3)
    seven = [x, y, z, w, a, b, x]
    row(ctx=seven + [z] + [w], toks=seven[:4] + seven[4:], g=8)         # a 7-gram seen before, followed by z; Lc and cap are nearly full
    row(ctx=seven + [z], toks=seven[:6] + [y], g=8)                      # the last token differs: no match
    # bad words: one token; W tokens whose prefix ends the history, across the boundary; longer than the history; L - 1 == m
    row(ctx=[x], toks=[y], words=[[z], [x, y, w], [y, x, a]])
    row(ctx=[x, y], words=[[x, y, z], [y, w], [b, a]])
    row(ctx=[], toks=[], words=[[x, y], [x, y, z], [w]])                 # m = 0: only the one-token word
    row(ctx=[x], words=[[x, y], [w, x, z]])                              # m = 1 = L - 1: banned (HF would skip it); L - 1 = 2 > m: not
    row(ctx=[x, y], toks=[z], words=[[z, V], [z, V + 9], [z, -3], [y, z, 2 ** 31 - 1]])       # last ids outside [0, V): nothing
    row(ctx=[x, -1], words=[[-1, y]])                                    # (equality on integers: a negative history element equals a negative id)
    # early stop: n = min - 1 and n = min; empty slots and ids outside the vocabulary
    row(ctx=[x], toks=[y, z], min_new=3, stops=[w, -1, a])
    row(ctx=[x], toks=[y, z, w], min_new=3, stops=[w, -1, a])
    row(ctx=[x], toks=[], min_new=1, stops=[V, -1, V - 1])
    row(ctx=[x], toks=[y], min_new=2 ** 31 - 1, stops=[b, b, b])
    # all three at once
    row(ctx=[x, y, z, x], toks=[y], g=2, words=[[x, y, w], [a]], min_new=2, stops=[b, -1, -1])
    # device values the host could not have written
    row(ctx=[x, y, z] + [x] * (LC - 3), toks=[x], g=2, ctx_len=LC + 7)  # ctx_len past the row: clamped to Lc
    row(ctx=[x, y, z], toks=[x, y], g=3, ctx_len=-5)                     # negative: no ctx
    row(ctx=[x, y], toks=[z, x] + [y] * (CAP - 2), g=2, n=CAP + 100)     # n past the row: clamped to cap
    row(ctx=[x, y, x], toks=[y], g=2, n=-4, min_new=1, stops=[w, -1, -1])   # negative n: 0 -- and 0 < min
    row(ctx=[x, y, x], g=9)                                              # g outside 0 .. 8: off
    row(ctx=[x, y, x], g=-1)
    row(ctx=[x], words=[[x, y, z], [x, w], [a]], lens=[W + 1, -2, 1])    # lengths outside 0 .. W: unused slots
    return rows


def _pack(rows):
    """the rows as the launch's CPU tensors and lists"""
    R = len(rows)
    ctx = torch.full((R, LC), 5, dtype=torch.int32)
    toks = torch.full((R, CAP), 6, dtype=torch.long)
    tab = torch.full((R, Q, W), -1, dtype=torch.int32)
    lens = torch.zeros(R, Q, dtype=torch.int32)
    stops = torch.full((R, NS), -1, dtype=torch.long)
    for r, d in enumerate(rows):
        assert len(d["ctx"]) <= LC and len(d["toks"]) <= CAP and len(d["words"]) <= Q and len(d["stops"]) <= NS
        ctx[r, :len(d["ctx"])] = torch.tensor(d["ctx"], dtype=torch.int32)
        toks[r, :len(d["toks"])] = torch.tensor(d["toks"], dtype=torch.long)
        for q, word in enumerate(d["words"]):
            tab[r, q, :len(word)] = torch.tensor(word, dtype=torch.int32)
            lens[r, q] = len(word) if d["lens"] is None else d["lens"][q]
        stops[r, :len(d["stops"])] = torch.tensor(d["stops"], dtype=torch.long)
    i32 = lambda k: torch.tensor([d[k] for d in rows], dtype=torch.int32)
    return dict(ctx=ctx, ctx_len=i32("ctx_len"), toks=toks, n=torch.tensor([d["n"] for d in rows], dtype=torch.long), g=i32("g"), tab=tab, lens=lens,
                min=i32("min"), stops=stops)


def _want(logits, p, n=True, active=None, out=None):
    return ref.mask(logits, p["ctx"].tolist(), p["ctx_len"].tolist(), p["toks"].tolist(), p["n"].tolist() if n else None, p["g"].tolist(),
                    p["tab"].tolist(), p["lens"].tolist(), p["min"].tolist(), p["stops"].tolist(), active=active, out=out)


_CASES = {}


def _case(dtype, V):
    """rows, packed arrays, logits and the restatement's answers -- made once per (dtype, V), never modified"""
    key = (dtype, V)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(9000 * V + (1 if dtype == torch.bfloat16 else 0))
    rows = _rows(V)
    p = _pack(rows)
    R = len(rows)
    sp = torch.tensor(SPECIAL)
    logits = torch.randn(R, V, generator=g) * 4
    for r in range(R):                                                   # special values at every symbol (banned in some row, kept in others) and next to it
        for i, y in enumerate(_syms(V)):
            logits[r, y] = sp[(i + r) % len(sp)]
            logits[r, (y + 1) % V] = sp[(i + r + 3) % len(sp)]
    logits = logits.to(dtype)
    c = dict(rows=rows, p=p, logits=logits, want=_want(logits, p), want0=_want(logits, p, n=False))
    _CASES[key] = c
    return c


def _padded(x, pad, fill):
    """x [R, V] on the device as a view of a [R, V + pad] buffer whose padding holds `fill` bits (int16)"""
    buf = torch.full((x.shape[0], x.shape[1] + pad), fill, dtype=torch.int16, device="cuda")
    view = buf.view(x.dtype)[:, :x.shape[1]]
    view.copy_(x)
    return view


def _dev(p, rows=slice(None), strided=True):
    d = {k: v[rows].cuda().contiguous() for k, v in p.items()}
    if strided:                                                          # the turn's tokens as a view of a wider buffer full of a token that would match
        buf = torch.full((d["toks"].shape[0], CAP + 6), 0, dtype=torch.long, device="cuda")
        buf[:, :CAP] = d["toks"]
        d["toks"] = buf[:, :CAP]
    return d


def _nbanned(t, dtype):
    return (t.view(torch.int16) == ref.NEG_INF_BITS[dtype]).sum(1).tolist()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("V", VS)
def test_rows_form_against_the_restatement(ops, dtype, V):
    c = _case(dtype, V)
    d = _dev(c["p"])
    R = len(c["rows"])
    lg = _padded(c["logits"], 8, NAN16[dtype])                           # sl = V + 8, the padding holds NaN
    for with_n, want in ((True, c["want"]), (False, c["want0"])):
        out = CanaryOut(1, R, V, dtype, row_margin=2, col_margin=8)      # so = V + 16
        assert out.view[0].stride(0) == V + 16 and lg.stride(0) == V + 8 and d["toks"].stride(0) == CAP + 6
        kw = dict(toks=d["toks"], n=d["n"]) if with_n else {}
        res = ops.ban_rows(lg, d["ctx"], d["ctx_len"], d["g"], d["tab"], d["lens"], d["min"], d["stops"], out=out.view[0], **kw)
        assert res.data_ptr() == out.view[0].data_ptr()
        got = out.view[0].cpu()
        for r in range(R):
            assert ref.same_bits(got[r], want[r]), (with_n, r, c["rows"][r])
        assert out.untouched_outside()
    assert ref.same_bits(c["want"][0], c["logits"][0])                   # nothing set: the row itself
    # the rows do differ, and the expected sets are the ones the definition's text gives for the first n-gram rows
    s = _syms(V)
    src_inf = _nbanned(c["logits"], dtype)
    more = [a - b for a, b in zip(_nbanned(c["want"], dtype), src_inf)]
    assert more[0] == 0 and max(more) >= 2 and sum(1 for v in more if v > 0) >= 15
    z = s[2]
    for r in (1, 2, 3, 4):
        assert c["want"][r].view(torch.int16)[z] == ref.NEG_INF_BITS[dtype], r
    # NaN and -0.0 survive at kept positions, bit for bit
    kept = c["want"].view(torch.int16) == c["logits"].view(torch.int16)
    src = c["logits"].float()
    assert bool((kept & src.isnan()).any()) and bool((kept & (src == 0) & (c["logits"].view(torch.int16) < 0)).any())
    assert bool((~kept & src.isnan()).any())                            # ... and a banned NaN is -inf


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("V", VS)
def test_step_form_leaves_an_inactive_tenant_alone(ops, dtype, V):
    c = _case(dtype, V)
    d = _dev(c["p"])
    R = len(c["rows"])
    lg = _padded(c["logits"], 8, NAN16[dtype])
    before = {k: v.clone() for k, v in d.items()}
    for active in ([r % 2 == 0 for r in range(R)], [r % 3 != 0 for r in range(R)], [True] * R):
        for as_bool in (True, False):
            out = CanaryOut(1, R, V, dtype, row_margin=2, col_margin=8)  # the rows are pre-filled with the canary's poison
            act = torch.tensor(active, dtype=torch.bool if as_bool else torch.uint8, device="cuda")
            ops.step_ban(lg, out.view[0], d["ctx"], d["ctx_len"], d["toks"], d["n"], d["g"], d["tab"], d["lens"], d["min"], d["stops"], act)
            got = out.view[0].cpu()
            for r in range(R):
                if active[r]:
                    assert ref.same_bits(got[r], c["want"][r]), (active[r], r)
                else:
                    assert bool((got[r].view(torch.int16) == POISON16).all()), r
            assert out.untouched_outside()
    prev = torch.full((R, V), POISON16, dtype=torch.int16).view(dtype)
    half = [r % 2 == 0 for r in range(R)]
    assert ref.same_bits(_want(c["logits"], c["p"], active=half, out=prev)[1], prev[1])      # (the restatement's own rule for an inactive row)
    assert all(torch.equal(d[k], before[k]) for k in d)                  # the launch only reads


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_one_row_alone_gives_the_bits_it_has_among_the_others(ops, dtype):
    V = 2056
    c = _case(dtype, V)
    for r in range(0, len(c["rows"]), 3):
        d = _dev(c["p"], slice(r, r + 1), strided=False)
        got = ops.ban_rows(c["logits"][r:r + 1].cuda(), d["ctx"], d["ctx_len"], d["g"], d["tab"], d["lens"], d["min"], d["stops"], toks=d["toks"],
                           n=d["n"])
        assert ref.same_bits(got.cpu(), c["want"][r:r + 1]), r
    # no stop list at all (a null pointer): min_new_tokens bans nothing
    d = _dev(c["p"])
    got = ops.ban_rows(c["logits"].cuda(), d["ctx"], d["ctx_len"], d["g"], d["tab"], d["lens"], d["min"], None, toks=d["toks"], n=d["n"])
    p2 = dict(c["p"], stops=torch.full((len(c["rows"]), 1), -1, dtype=torch.long))
    assert ref.same_bits(got.cpu(), _want(c["logits"], p2))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("Qx,Wx", [(1, 1), (64, 32)])
def test_table_sizes_at_both_ends(ops, dtype, Qx, Wx):
    """Q = 1 and Q = 64: words of length 1 and of length W whose W - 1 first tokens end the history across the ctx / out boundary, every word
    banning another token; one word longer than the history; one whose prefix differs in its FIRST token"""
    V, Lc, cap, R = 2056, 40, 24, 3
    g = torch.Generator().manual_seed(31 * Qx + Wx)
    hist = torch.randint(0, V, (R, Lc + cap), generator=g)
    ctx_len, n = [Lc, 17, 0], [cap, 20, 5]
    tab = torch.full((R, Qx, Wx), -1, dtype=torch.int32)
    lens = torch.zeros(R, Qx, dtype=torch.int32)
    ctx = torch.zeros(R, Lc, dtype=torch.int32)
    toks = torch.zeros(R, cap, dtype=torch.long)
    for r in range(R):
        ctx[r, :ctx_len[r]] = hist[r, :ctx_len[r]].int()
        toks[r, :n[r]] = hist[r, ctx_len[r]:ctx_len[r] + n[r]]
        h = hist[r, :ctx_len[r] + n[r]].tolist()
        for q in range(Qx):
            L = Wx if q % 2 == 0 else 1 + q % Wx
            if L - 1 > len(h):                                           # longer than the history: never banned
                tab[r, q, :L] = torch.tensor([1] * L, dtype=torch.int32)
            else:
                word = h[len(h) - (L - 1):] + [(2047 + q) % V]          # bans 2047 .. 2047 + 63: both sides of the slice boundary
                if q % 5 == 4 and L > 1:
                    word[0] = (word[0] + 1) % V                          # a near miss at the far end of the prefix
                tab[r, q, :L] = torch.tensor(word, dtype=torch.int32)
            lens[r, q] = L
    logits = (torch.randn(R, V, generator=g) * 3).to(dtype)
    zeros = torch.zeros(R, dtype=torch.int32)
    stops = torch.full((R, 1), -1, dtype=torch.long)
    want = ref.mask(logits, ctx.tolist(), ctx_len, toks.tolist(), n, [0] * R, tab.tolist(), lens.tolist(), [0] * R, stops.tolist())
    got = ops.ban_rows(logits.cuda(), ctx.cuda(), torch.tensor(ctx_len, dtype=torch.int32).cuda(), zeros.cuda(), tab.cuda(), lens.cuda(), zeros.cuda(),
                       stops.cuda(), toks=toks.cuda(), n=torch.tensor(n).cuda())
    assert ref.same_bits(got.cpu(), want)
    nb = _nbanned(want, dtype)
    assert nb[0] >= (1 if Qx == 1 else 40) and (Qx == 1 or nb[2] < nb[0])      # (row 2's history of 5 tokens is shorter than the long words)


def test_a_long_history_with_every_ngram_size(ops):
    """1024 + 200 tokens over 40 symbols, g = 1 .. 8 in one launch: hundreds of candidates per thread stride, matches on both sides of the boundary"""
    V, Lc, cap = 4104, 1024, 256
    g = torch.Generator().manual_seed(77)
    R = 8
    hist = torch.randint(2030, 2070, (R, Lc + 200), generator=g)
    hist[:, -7:] = hist[:, 500:507]                                      # the tail occurred before, in ctx ...
    hist[:, 1100:1107] = hist[:, 500:507]                                # ... and in out
    ctx, toks = hist[:, :Lc].int().contiguous(), torch.zeros(R, cap, dtype=torch.long)
    toks[:, :200] = hist[:, Lc:]
    ngram = list(range(1, 9))
    logits = (torch.randn(R, V, generator=g) * 3).to(torch.float16)
    tab, lens = torch.full((R, 1, 1), -1, dtype=torch.int32), torch.zeros(R, 1, dtype=torch.int32)
    want = ref.mask(logits, ctx.tolist(), [Lc] * R, toks.tolist(), [200] * R, ngram, tab.tolist(), lens.tolist(), [0] * R, [[-1]] * R)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).cuda()
    got = ops.ban_rows(logits.cuda(), ctx.cuda(), i32([Lc] * R), i32(ngram), tab.cuda(), lens.cuda(), i32([0] * R), None, toks=toks.cuda(),
                       n=torch.tensor([200] * R).cuda())
    assert ref.same_bits(got.cpu(), want)
    nb = _nbanned(want, torch.float16)
    assert nb[0] == 40 and all(nb[i] >= nb[i + 1] for i in range(7)) and nb[7] >= 1


def test_every_error_code_comes_back_with_nothing_launched(ops):
    """the entry points with real device buffers: each refusal returns its code and the output still holds what it held (tests/test_ban_host.py
    walks every check on host pointers)"""
    from bitdelta_amd._lib import lib, ptr
    L = lib()
    V, R = 64, 2
    lg = torch.zeros(R, V, dtype=torch.float16, device="cuda")
    out = torch.full((R, V), 3.0, dtype=torch.float16, device="cuda")
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    ctx, ctx_len, ng, tab, lens, mn = i32(R, 8), i32(R), i32(R), i32(R, 2, 3), i32(R, 2), i32(R)
    ng += 1
    ctx_len += 8
    toks, n = torch.zeros(R, 4, dtype=torch.long, device="cuda"), torch.ones(R, dtype=torch.long, device="cuda")
    stops = torch.full((R, 2), -1, dtype=torch.long, device="cuda")
    act = torch.ones(R, dtype=torch.uint8, device="cuda")
    BAD_SHAPE, BAD_DTYPE, NULL = (L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None),
                                  L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 7, None), L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 0, None))

    def call(step, V=V, sl=V, Qx=2, Wx=3, ns=2, R=R, dtype=0, logits=lg, tokp=toks, s_tok=4):
        a = (ptr(logits), sl, V, ptr(out), V, ptr(ctx), 8, ptr(ctx_len), ptr(tokp), s_tok, 4, ptr(n), ptr(ng), ptr(tab), ptr(lens), Qx, Wx, ptr(mn),
             ptr(stops), ns)
        return L.bd_srv_step_ban(*a, ptr(act), R, dtype, None) if step else L.bd_srv_ban_rows(*a, R, dtype, None)
    for step in (False, True):
        assert call(step, V=60) == BAD_SHAPE and call(step, sl=56) == BAD_SHAPE and call(step, Qx=0) == BAD_SHAPE and call(step, Wx=33) == BAD_SHAPE
        assert call(step, ns=65) == BAD_SHAPE and call(step, R=-1) == BAD_SHAPE and call(step, s_tok=3) == BAD_SHAPE
        assert call(step, dtype=2) == BAD_DTYPE and call(step, logits=None) == NULL and call(step, tokp=None) == NULL
        assert call(step, R=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    with pytest.raises(AssertionError):
        ops.ban_rows(lg, ctx.long(), ctx_len, ng, tab, lens, mn)
    with pytest.raises(AssertionError):
        ops.ban_rows(lg, ctx, ctx_len, ng, torch.zeros(R, 65, 3, dtype=torch.int32, device="cuda"), i32(R, 65), mn)
    with pytest.raises(Exception):
        ops.ban_rows(lg.cpu(), ctx, ctx_len, ng, tab, lens, mn)
    assert ops.ban_rows(lg[:0], ctx[:0], ctx_len[:0], ng[:0], tab[:0], lens[:0], mn[:0]).shape == (0, V)      # no rows: nothing is launched
