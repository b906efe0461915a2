"""GPU tests of bd_srv_token_logprobs (serving_ops.token_logprobs): the kernel against the fp64 restatement of its definition
(tests/logprobs_ref.py) and against bd_srv_token_nll, the kernel whose log-sum-exp it shares.

The ids must be EXACTLY the restatement's; every finite lp / top_lp within the header's accuracy clause, |got - ref| <= 2^-19 (1 + |ref|), which
is bd_srv_token_nll's and is derived there from the arithmetic, not from what the kernel returns; NaN-ness and infinities are compared exactly.
Every launch writes inside poisoned canary buffers and reads rows whose padding (elements V .. sl - 1) holds NaN patterns."""
import numpy as np
import pytest
import torch

import logprobs_ref as ref
from canary import POISON, CanaryOut

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
NAME = {torch.float16: "float16", torch.bfloat16: "bfloat16"}
NAN_BITS = {torch.float16: 0x7e00, torch.bfloat16: 0x7fc0}
N_CASES = 17
VS = [8, 2048, 2056, 32000, 32776, 65544]      # one vector; one vector per thread; one past it; the served vocabulary; past 32768 (register bound), twice over
PLATEAU, ZEROS, FEW, TOP_PLATEAU = 4, 5, 6, 15


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib, serving_ops
    _lib.lib()
    return serving_ops


def _to_bits(x, dtype):
    return x.to(dtype).view(torch.int16).numpy().view(np.uint16).copy()


def _spread(V, step_div, extra):
    """indices spread over the whole row: every (V // step_div)-th column -- many threads' vectors -- and both ends of the row"""
    return sorted(set(range(0, V, max(1, V // step_div))) | {e % V for e in extra})


_ROWS, _REFS = {}, {}


def _rows(dtype, V):
    """N_CASES rows of 16-bit patterns [N, V] and their tokens -- made once per (dtype, V) and never modified"""
    key = (dtype, V)
    if key in _ROWS:
        return _ROWS[key]
    g = torch.Generator().manual_seed(7000 * V + (1 if dtype == torch.bfloat16 else 0))
    inf = float("inf")
    rnd = lambda std: torch.randn(V, generator=g) * std
    pick = lambda: int(torch.randint(0, V, (1,), generator=g))
    amax = lambda r: int(r.to(dtype).float().argmax())
    rows, toks = [], []

    def add(row, tok):
        rows.append(row)
        toks.append(tok)
    r = rnd(8.0); add(r, pick())                                                     # 0  random normal, scale 8
    r = rnd(0.5); add(r, 0)                                                          # 1  scale 0.5 (many equal 16-bit values), the first token
    r = rnd(8.0); add(r, amax(r))                                                    # 2  the argmax
    add(torch.full((V,), 3.25), V - 1)                                               # 3  all equal: the ids are 0 .. top_n - 1
    r = rnd(0.25) - 4.0                                                              # 4  a plateau straddling the top_n-th place: up to 3 values above it,
    pl = _spread(V, 37, (0, 1, -1, -2))                                              #    ~40 members on many threads' columns and both ends of the row
    r[pl] = 2.5
    for i, c in enumerate(_spread(V, 3, ())[1:4]):
        if V > 8 or i == 0:
            r[min(c + 3, V - 5)] = 3.0 + i
    add(r, pl[-1])
    r = -rnd(1.0).abs() - 1.0                                                        # 5  +0 and -0 mixed at the boundary: one value, index order decides
    z = _spread(V, 29, (2, -1, -3))
    r[z[0::2]] = 0.0
    r[z[1::2]] = -0.0
    if V > 8:
        r[(z[3] + 1) % V] = 1.0
        r[(z[7] + 1) % V] = 0.5
    add(r, z[1])
    r = torch.full((V,), -inf); f = _spread(V, 2, (-1,))[:3]                         # 6  fewer than top_n finite values: -inf fills the list in index order
    r[f] = torch.tensor([0.5, -1.0, 2.0])[:len(f)]
    add(r, f[0])
    add(torch.full((V,), -inf), 0)                                                   # 7  nothing finite
    r = rnd(8.0); r[pick()] = float("nan"); add(r, 0)                                # 8  a NaN
    r = rnd(8.0); r[pick()] = inf; add(r, V - 1)                                     # 9  a +inf
    r = rnd(8.0); r[1::2] = -inf; add(r, 1)                                          # 10 the token on a -inf
    add(rnd(8.0), V)                                                                 # 11 the token out of range
    add(rnd(0.5), -1)                                                                # 12 ... below it
    r = torch.zeros(V); p = pick(); r[p] = 30.0; add(r, p)                           # 13 one-hot-dominant, the token on the peak: lp ~ -V e^-30
    r = rnd(100.0); r[::3] = 65504.0; r[1::3] = -65504.0; add(r, 0)                  # 14 spanning +-65504: a third of the row is one plateau at the top
    r = rnd(1.0); r[_spread(V, 31, (-1, 5))] = 9.0; add(r, V - 1)                    # 15 a plateau AT the top: nothing above it, every place from it
    r = rnd(0.5); add(r, amax(r))                                                    # 16 scale 0.5, the argmax
    assert len(rows) == N_CASES
    bits = np.stack([_to_bits(x, dtype) for x in rows])
    toks = np.array(toks, dtype=np.int64)
    bits.setflags(write=False)
    toks.setflags(write=False)
    _ROWS[key] = (bits, toks)
    return _ROWS[key]


def _cases(dtype, V, top_n):
    """the rows, their tokens and the fp64 answers for one top_n -- computed once and never modified"""
    key = (dtype, V, top_n)
    if key not in _REFS:
        bits, toks = _rows(dtype, V)
        out = ref.rows_logprobs(bits, NAME[dtype], toks, top_n)
        for a in out:
            a.setflags(write=False)
        _REFS[key] = (bits, toks) + out
    return _REFS[key]


def _device_rows(bits, dtype, sl):
    """rows [R, V] as a view into a [R, sl] device buffer whose other elements hold NaN patterns"""
    R, V = bits.shape
    full = np.full((R, sl), NAN_BITS[dtype], dtype=np.uint16)
    full[:, :V] = bits
    return torch.from_numpy(full.view(np.int16)).cuda().view(dtype)[:, :V]


def _launch(ops, lg, toks, top_n):
    """serving_ops.token_logprobs on the view lg [R, V] with the three outputs inside canary buffers; returns CPU copies"""
    R = lg.shape[0]
    tok = torch.as_tensor(np.array(toks), dtype=torch.long).cuda()
    cans = [CanaryOut(1, 1, R * w, dt, row_margin=1, col_margin=64) for w, dt in ((1, torch.float32), (top_n, torch.int32), (top_n, torch.float32))]
    outs = (cans[0].view[0, 0], cans[1].view[0, 0].view(R, top_n), cans[2].view[0, 0].view(R, top_n))
    got = ops.token_logprobs(lg, tok, top_n, out=outs)
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, outs))
    res = tuple(o.clone().cpu() for o in outs)
    for c, what in zip(cans, ("lp", "top_id", "top_lp")):
        assert c.untouched_outside(), "a store outside " + what
    return res


def _bits32(t):
    return t.contiguous().view(torch.int32).numpy()


def _check(got, want, toks, what):
    lp, ids, lps = (g.numpy() for g in got)
    ref_lp, ref_ids, ref_lps = want
    with np.errstate(invalid="ignore"):
        ok_lp, ok_lps = ref.within(lp, ref_lp), ref.within(lps, ref_lps)
    for r in range(len(toks)):
        ctx = (what, "row", r, "token", int(toks[r]), "lp", float(lp[r]), "ref", float(ref_lp[r]))
        assert ids[r].tolist() == ref_ids[r].tolist(), ctx + (ids[r].tolist(), ref_ids[r].tolist())
        assert ok_lp[r], ctx
        assert ok_lps[r].all(), ctx + (lps[r].tolist(), ref_lps[r].tolist())


def _start(dtype, V, top_n):
    return (V // 8 + 3 * top_n + (5 if dtype == torch.bfloat16 else 0)) % N_CASES


@pytest.mark.parametrize("top_n", [0, 1, 5, 20])
@pytest.mark.parametrize("R", [1, 17])
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_against_the_fp64_restatement_and_token_nll(ops, dtype, V, R, top_n):
    top_n = min(top_n, V)
    bits, toks, *want = _cases(dtype, V, top_n)
    # 17 is the whole table; 1 takes a row from a start that rotates with (dtype, V, top_n), so every kind of row also runs alone somewhere
    idx = list(range(N_CASES)) if R == 17 else [_start(dtype, V, top_n)]
    sl = V + (24 if (V // 8 + top_n) % 2 else 0)
    lg = _device_rows(bits[idx], dtype, sl)
    got = _launch(ops, lg, toks[idx], top_n)
    _check(got, [w[idx] for w in want], toks[idx], (NAME[dtype], V, R, top_n, sl))
    # against the existing kernel, as floats (-0 == +0): lp == -nll for a token in range, top_lp[j] == -nll(row, top_id[j])
    lp, ids, lps = got
    tok = torch.as_tensor(toks[idx].copy(), dtype=torch.long)
    inr = (tok >= 0) & (tok < V)
    nll = ops.token_nll(lg, tok.cuda()).cpu()
    same = lambda a, b: bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())
    assert same(lp[inr], -nll[inr]) and bool(torch.isnan(lp[~inr]).all())
    for j in range(top_n):
        col = ids[:, j].long()
        bad = col < 0
        nll = ops.token_nll(lg, col.clamp(min=0).cuda()).cpu()
        assert same(lps[~bad, j], -nll[~bad]) and bool(torch.isnan(lps[bad, j]).all()), j


def test_top_n_8_of_a_row_of_8(ops):
    for dtype in DTYPES:
        bits, toks, *want = _cases(dtype, 8, 8)
        got = _launch(ops, _device_rows(bits, dtype, 16), toks, 8)
        _check(got, want, toks, (NAME[dtype], 8, 17, 8))
        assert got[1][3].tolist() == list(range(8))                                  # all equal: every index, in order
        assert sorted(got[1][0].tolist()) == list(range(8))


def test_the_rows_hold_what_their_names_say():
    """the table's special rows do exercise the tie paths at the served vocabulary: checked on the restatement's answers, no kernel involved"""
    for dtype in DTYPES:
        bits, toks, lp, ids, lps = _cases(dtype, 32000, 5)
        l = ref.values(bits[PLATEAU], NAME[dtype])
        assert (l > 2.5).sum() == 3 and (l == 2.5).sum() > 20 and ids[PLATEAU][3:].tolist() == [0, 1]          # 3 above, the plateau's first two
        members = np.flatnonzero(l == 2.5)
        assert len({(int(c) // 8) % 256 for c in members}) > 20 and members[-1] == 31999
        l = ref.values(bits[ZEROS], NAME[dtype])
        zeros = np.flatnonzero(l == 0.0)
        assert (l > 0).sum() == 2 and len(zeros) > 20 and len({int(bits[ZEROS][c]) for c in zeros}) == 2      # both signs of zero
        assert ids[ZEROS][2:].tolist() == zeros[:3].tolist() and len({int(bits[ZEROS][c]) for c in zeros[:3]}) == 2
        assert np.isfinite(ref.values(bits[FEW], NAME[dtype])).sum() == 3 and np.isneginf(lps[FEW]).sum() == 2
        l = ref.values(bits[TOP_PLATEAU], NAME[dtype])
        assert (l == l.max()).sum() > 20 and ids[TOP_PLATEAU].tolist() == np.flatnonzero(l == l.max())[:5].tolist()
        assert ids[3].tolist() == [0, 1, 2, 3, 4] and ids[7].tolist() == [-1] * 5 and np.isnan(lp[[7, 8, 9, 11, 12]]).all() and lp[10] == -np.inf


@pytest.mark.parametrize("top_n", [5, 20])
@pytest.mark.parametrize("V", [2056, 32000, 32776])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_a_result_is_a_pure_function_of_row_token_and_top_n(ops, dtype, V, top_n):
    """one row alone, among 17 at other indices with other neighbours and another stride, and replayed from a captured graph: the same bits"""
    from bitdelta_amd._lib import DTYPE_CODE, lib, ptr, stream_ptr
    bits, toks, *_ = _cases(dtype, V, top_n)
    want = {}
    for k in (0, PLATEAU, ZEROS, FEW, 14):
        want[k] = _launch(ops, _device_rows(bits[k:k + 1], dtype, V), toks[k:k + 1], top_n)
    order = list(range(N_CASES))[::-1]
    lg = _device_rows(bits[order], dtype, V + 40)
    lp, ids, lps = _launch(ops, lg, toks[order], top_n)
    for k, (a, b, c) in want.items():
        r = order.index(k)
        assert _bits32(lp)[r] == _bits32(a)[0] and ids[r].tolist() == b[0].tolist() and np.array_equal(_bits32(lps)[r], _bits32(c)[0]), k
    tok = torch.as_tensor(toks[order].copy(), dtype=torch.long).cuda()
    g_lp = torch.full((N_CASES,), -7.0, dtype=torch.float32, device="cuda")
    g_id = torch.full((N_CASES, top_n), -7, dtype=torch.int32, device="cuda")
    g_lps = torch.full((N_CASES, top_n), -7.0, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc = lib().bd_srv_token_logprobs(ptr(lg), lg.stride(0), V, ptr(tok), ptr(g_lp), ptr(g_id), ptr(g_lps), top_n, N_CASES, DTYPE_CODE[dtype],
                                         stream_ptr())
    assert rc == 0
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits32(g_lp.cpu()), _bits32(lp)) and torch.equal(g_id.cpu(), ids) and np.array_equal(_bits32(g_lps.cpu()), _bits32(lps))


def test_step_form_writes_the_entry_of_the_token_just_stored_and_follows_n(ops):
    """bd_srv_step_logprobs: a tenant whose count did not move is not touched; one whose count moved gets entry [t, n - 1] (token_logprobs' bits)
    when it lies inside the buffers, and its counter follows in either case"""
    dtype, V, T, cap, k = torch.float16, 2056, 6, 4, 5
    bits, toks, *_ = _cases(dtype, V, k)
    idx = [0, 1, PLATEAU, 2, ZEROS, 16]
    lg = _device_rows(bits[idx], dtype, V + 8)
    tok = torch.as_tensor(toks[idx].copy(), dtype=torch.long).cuda().view(T, 1)
    n = torch.tensor([2, 3, 4, 5, 0, 1], device="cuda")                                 # tenant 3: past the buffers; 4: never admitted
    lp_n = torch.tensor([1, 3, 3, 4, 0, 0], device="cuda")                              # tenant 1 and 4: nothing emitted
    cans = [CanaryOut(1, 1, T * cap * w, dt, row_margin=1, col_margin=64) for w, dt in ((1, torch.float32), (k, torch.int32), (k, torch.float32))]
    lp, top_id, top_lp = cans[0].view[0, 0].view(T, cap), cans[1].view[0, 0].view(T, cap, k), cans[2].view[0, 0].view(T, cap, k)
    for o in (lp, top_id, top_lp):
        o.view(torch.int32).fill_(0x7F7F7F7F)
    ops.step_logprobs(lg, tok, n, lp_n, lp, top_id, top_lp)
    torch.cuda.synchronize()
    assert lp_n.tolist() == n.tolist() == [2, 3, 4, 5, 0, 1]
    want = ops.token_logprobs(lg, tok.view(-1), k)
    written = {0: 1, 2: 3, 5: 0}
    for t in range(T):
        for j in range(cap):
            got = (lp[t, j:j + 1], top_id[t, j], top_lp[t, j])
            if written.get(t) == j:
                assert all(np.array_equal(_bits32(a.cpu()), _bits32(b.cpu())) for a, b in zip(got, (want[0][t:t + 1], want[1][t], want[2][t]))), (t, j)
            else:
                assert all(bool((a.view(torch.int32) == 0x7F7F7F7F).all()) for a in got), (t, j)
    assert all(c.untouched_outside() for c in cans)


def test_refusals_return_their_codes_and_write_nothing(ops):
    from bitdelta_amd._lib import lib, ptr, stream_ptr
    L = lib()
    BAD_SHAPE, BAD_DTYPE, NULL = (L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None),
                                  L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 7, None), L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 0, None))
    lg = torch.zeros(2, 72, dtype=torch.float16, device="cuda")
    tok = torch.zeros(2, dtype=torch.long, device="cuda")
    outs = [torch.full((64,), POISON, dtype=torch.uint8, device="cuda") for _ in range(5)]
    good = dict(logits=ptr(lg), sl=72, V=64, tok=ptr(tok), n=ptr(outs[3]), lp_n=ptr(outs[4]), lp=ptr(outs[0]), top_id=ptr(outs[1]), top_lp=ptr(outs[2]),
                cap=1, top_n=5, R=2, dtype=0)

    def rows(**kw):
        a = dict(good, **kw)
        return L.bd_srv_token_logprobs(a["logits"], a["sl"], a["V"], a["tok"], a["lp"], a["top_id"], a["top_lp"], a["top_n"], a["R"], a["dtype"], stream_ptr())

    def step(**kw):
        a = dict(good, **kw)
        return L.bd_srv_step_logprobs(a["logits"], a["sl"], a["V"], a["tok"], a["n"], a["lp_n"], a["lp"], a["top_id"], a["top_lp"], a["cap"], a["top_n"],
                                      a["R"], a["dtype"], stream_ptr())
    for call in (rows, step):
        assert call(R=0) == 0
        assert call(top_n=-1) == call(top_n=21) == call(V=8, sl=8, top_n=9) == BAD_SHAPE
        assert call(V=60) == call(sl=68) == call(sl=56) == call(V=(1 << 22) + 8, sl=(1 << 22) + 8) == BAD_SHAPE
        assert call(logits=lg.data_ptr() + 8) == call(lp=outs[0].data_ptr() + 2) == call(tok=tok.data_ptr() + 4) == BAD_SHAPE
        assert call(logits=None) == call(tok=None) == call(lp=None) == call(top_id=None) == call(top_lp=None) == NULL
        assert call(dtype=2) == call(dtype=7) == BAD_DTYPE
    assert step(n=None) == step(lp_n=None) == NULL
    torch.cuda.synchronize()
    assert all(bool((o == POISON).all()) for o in outs)
