"""GPU tests of bd_srv_constrain_rows / bd_srv_step_constrain / bd_srv_step_constrain_advance (serving_ops.constrain_rows / step_constrain /
step_constrain_advance): EXACT bits against the restatement of the definition (tests/constraint_ref.py), in both dtypes, at four vocabulary
sizes -- one vector, exactly one block, one vector into the second block, the served row (its last block is masked) -- with one row and with
three rows that carry different automata, row strides larger than V, and the output inside a poisoned canary buffer."""
import pytest
import torch

import constraint_ref as ref
from canary import POISON, CanaryOut

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
VS = [8, 2048, 2056, 32000]
S = 6                        # states per row of the launch (the automata below have five; state 5 is padding nobody reaches)
POISON16 = POISON * 0x0101
inf, nan = float("inf"), float("nan")
SPECIAL = [nan, -inf, inf, -0.0, 0.0, 6.0e-8, -6.0e-8, 1.0e-40, 65504.0, -65504.0, 1.5]      # (6e-8: an fp16 subnormal; 1e-40: a bf16 one)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib, serving_ops
    _lib.lib()
    return serving_ops


def _multi(V, E, g):
    """an automaton of five states in CSR lists, at most 8 edges: 0 one edge; 1 edges at the vector and block boundaries 0, 7, 8, 2047, 2048,
    V - 1 (those below V); 2 empty and accepting; 3 accepting with two edges; 4 (device values the host could not have written) an edge
    token below V followed by two at and past V"""
    pick = lambda: int(torch.randint(0, V, (1,), generator=g))
    bounds = sorted({y for y in (0, 7, 8, 2047, 2048, V - 1) if 0 <= y < V})
    if V == 8:
        bounds = [0, 7]                                                  # (E = V = 8 holds 1 + 2 + 0 + 2 + 3 edges)
    two = sorted({pick(), (pick() + 1) % V} | {V // 2})[:2]
    if len(two) < 2:
        two = [0, V - 1]
    per = [[pick()], bounds, [], two, [pick(), V, V + 5]]
    off, tok = [0], []
    for p in per:
        tok += p
        off.append(len(tok))
    assert len(tok) <= E
    return off, tok, [(i * 7 + 1) % 5 for i in range(len(tok))], [0, 0, 1, 1, 0]


_CASES = {}


def _case(dtype, V):
    """three rows with their automata, the launches' state vectors and the restatement's answers -- made once per (dtype, V), never modified"""
    key = (dtype, V)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(7000 * V + (1 if dtype == torch.bfloat16 else 0))
    E = min(V, 4096)
    a0, a2 = _multi(V, E, g), _multi(V, E, g)
    full = sorted(torch.randperm(V, generator=g)[:E].tolist())          # row 1: ONE state whose slice is all E edges
    a1 = ([0, E], full, [0] * E, [1])
    off, tok, nxt, acc = ref.pack([a0, a1, a2], S, E, fill_tok=3)
    sp = torch.tensor(SPECIAL)
    logits = (torch.randn(3, V, generator=g) * 4)
    logits[1] = sp[torch.randint(0, len(sp), (V,), generator=g)]         # special values at kept and at masked positions of the full slice
    for r, a in ((0, a0), (2, a2)):                                      # ... and at every edge token and stop id of the other rows, and next to them
        for i, y in enumerate(y for y in a[1] + [V - 2, 1] if y < V):
            logits[r, y] = sp[i % len(sp)]
            logits[r, (y + 1) % V] = sp[(i + 3) % len(sp)]
    logits = logits.to(dtype)
    stops = torch.tensor([[V - 2, 1, -1], [-1, full[0], (full[0] + 1) % V], [V - 2, -1, -1]])
    # every state of the multi-state rows, no constraint, and states at and past S; row 1 is in its one state or free
    states = [[0, 0, 1], [1, 0, 2], [2, -1, 3], [3, 0, 4], [4, S, 0], [-1, 0, S + 5], [S, -1, -1], [5, 0, 2]]
    want = [ref.mask(logits, st, off, tok, acc, stops) for st in states]
    c = dict(E=E, off=off, tok=tok, nxt=nxt, acc=acc, logits=logits, stops=stops, states=states, want=want, autos=(a0, a1, a2))
    _CASES[key] = c
    return c


def _padded(x, pad, fill):
    """x [R, V] on the device as a view of a [R, V + pad] buffer whose padding holds `fill` bits (int16)"""
    buf = torch.full((x.shape[0], x.shape[1] + pad), fill, dtype=torch.int16, device="cuda")
    view = buf.view(x.dtype)[:, :x.shape[1]]
    view.copy_(x)
    return view


def _dev(c, rows=slice(None)):
    return {k: c[k][rows].cuda().contiguous() for k in ("off", "tok", "nxt", "acc", "stops")}


NAN16 = {torch.float16: 0x7e00, torch.bfloat16: 0x7fc0}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("V", VS)
def test_rows_form_against_the_restatement(ops, dtype, V):
    c, d = _case(dtype, V), _dev(_case(dtype, V))
    lg = _padded(c["logits"], 8, NAN16[dtype])                           # sl = V + 8, the padding holds NaN
    seen = set()
    for st, want in zip(c["states"], c["want"]):
        out = CanaryOut(1, 3, V, dtype, row_margin=2, col_margin=8)      # so = V + 16
        assert out.view[0].stride(0) == V + 16 and lg.stride(0) == V + 8
        res = ops.constrain_rows(lg, torch.tensor(st, dtype=torch.int32, device="cuda"), d["off"], d["tok"], d["acc"], d["stops"], out=out.view[0])
        assert res.data_ptr() == out.view[0].data_ptr()
        got = out.view[0].cpu()
        assert ref.same_bits(got, want), st
        assert out.untouched_outside(), st
        for r in range(3):
            if st[r] < 0 or st[r] >= S:
                assert ref.same_bits(got[r], c["logits"][r]), (st, r)    # a bit-identical copy
            seen.add(int((got[r].view(torch.int16) != ref.NEG_INF_BITS[dtype]).sum()))
    assert len(seen) >= 4                                                # (the launches do differ: empty sets, single tokens, whole rows)
    # the definitions the restatement's answers rest on, on this case's own rows: one edge -> one element kept; the empty accepting state keeps
    # exactly its stop ids; the tokens >= V of state 4 keep nothing; the full slice keeps its E elements
    kept = lambda w, r: (w[r].view(torch.int16) != ref.NEG_INF_BITS[dtype]).nonzero().flatten().tolist()
    masked_anyway = lambda r: (c["logits"][r].view(torch.int16) == ref.NEG_INF_BITS[dtype]).nonzero().flatten().tolist()      # (a -inf logit)
    a0 = c["autos"][0]
    assert set(kept(c["want"][0], 0)) | set(masked_anyway(0)) >= {a0[1][0]} and len(kept(c["want"][0], 0)) <= 1
    assert set(kept(c["want"][2], 0)) <= {V - 2, 1} and len(kept(c["want"][4], 0)) <= 1
    full = set(c["autos"][1][1]) | {y for y in c["stops"][1].tolist() if y >= 0}         # the full slice: its E edges and, accepting, its stop ids
    assert set(kept(c["want"][0], 1)) == full - set(masked_anyway(1)) and len(full) in (c["E"], c["E"] + 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("V", VS)
def test_one_row_alone_and_among_other_rows(ops, dtype, V):
    """R = 1: every row launched alone, with contiguous buffers, gives the bits it has among the three -- whatever the other rows hold"""
    c = _case(dtype, V)
    for r in range(3):
        d = _dev(c, slice(r, r + 1))
        lg = c["logits"][r:r + 1].cuda()
        for st, want in zip(c["states"], c["want"]):
            got = ops.constrain_rows(lg, torch.tensor(st[r:r + 1], dtype=torch.int32, device="cuda"), d["off"], d["tok"], d["acc"], d["stops"])
            assert ref.same_bits(got.cpu(), want[r:r + 1]), (r, st)
    # row 0 among rows whose logits, automata, states and stop ids are all different: unchanged
    d = _dev(c)
    lg = c["logits"].cuda()
    lg[1:] = lg[1:].flip(1)
    d["tok"][1:] = d["tok"][1:].flip(0)
    d["off"][1:] = d["off"][1:].flip(0)
    d["acc"][1:] = 1 - d["acc"][1:]
    d["stops"][1:] = 0
    got = ops.constrain_rows(lg, torch.tensor([1, 3, 0], dtype=torch.int32, device="cuda"), d["off"], d["tok"], d["acc"], d["stops"])
    assert ref.same_bits(got[0].cpu(), c["want"][1][0])
    # no stop list at all (a null pointer): the accepting states keep their edges only
    d = _dev(c)
    got = ops.constrain_rows(c["logits"].cuda(), torch.tensor([2, 0, 3], dtype=torch.int32, device="cuda"), d["off"], d["tok"], d["acc"])
    assert ref.same_bits(got.cpu(), ref.mask(c["logits"], [2, 0, 3], c["off"], c["tok"], c["acc"]))
    assert bool((got[0].view(torch.int16) == ref.NEG_INF_BITS[dtype]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("V", VS)
def test_step_form_leaves_an_inactive_tenant_alone(ops, dtype, V):
    c, d = _case(dtype, V), _dev(_case(dtype, V))
    lg = _padded(c["logits"], 8, NAN16[dtype])
    for active in ([True, False, True], [False, True, False], [True, True, True]):
        for st, want in list(zip(c["states"], c["want"]))[:4]:
            out = CanaryOut(1, 3, V, dtype, row_margin=2, col_margin=8)  # the sentinel fill of the rows is the canary's poison
            act = torch.tensor(active, device="cuda")
            ops.step_constrain(lg, out.view[0], torch.tensor(st, dtype=torch.int32, device="cuda"), d["off"], d["tok"], d["acc"], d["stops"], act)
            got = out.view[0].cpu()
            for r in range(3):
                if active[r]:
                    assert ref.same_bits(got[r], want[r]), (active, st, r)           # what constrain_rows gives (the test above)
                else:
                    assert bool((got[r].view(torch.int16) == POISON16).all()), (active, st, r)
            assert out.untouched_outside()
    prev = torch.full((3, V), POISON16, dtype=torch.int16).view(dtype)
    assert ref.same_bits(got, ref.mask(c["logits"], c["states"][3], c["off"], c["tok"], c["acc"], c["stops"], active=[True] * 3, out=prev))


# ------------------------------------------------------------------------------------------------ the transition
def _trie():
    from bitdelta_amd.constraint import TokenAutomaton
    a = TokenAutomaton.from_choices([[5, 6], [5, 7, 8], [5], [9]])      # 0 -5-> 1 (accepting) -6-> 2 final, 1 -7-> 3 -8-> 4 final, 0 -9-> 5 final
    return a, (a.off, a.edge_tok, a.edge_next, a.accepting)


def test_advance_follows_the_token_and_retires_at_a_final_state(ops):
    a, csr = _trie()
    T, Sx, Ex = 9, 8, 7
    off, tok, nxt, acc = ref.pack([csr] * T, Sx, Ex)
    #        matched   unmatched  n == c_n  final     inactive  free     >= S      garbage tokens
    state = [0,        1,         1,        1,        3,        -1,      Sx + 1,   0,        1]
    y     = [5,        2,         6,        6,        8,        5,       5,        -5,       2 ** 40 + 6]
    n     = [4,        2,         7,        3,        9,        2,       2,        2,        2]
    c_n   = [3,        1,         7,        2,        8,        1,       1,        1,        1]
    active = [1,       1,         1,        1,        0,        1,       1,        1,        1]
    done  = [0,        0,         0,        2,        1,        0,        0,        0,        0]
    want = ref.advance(y, n, c_n, state, off, tok, nxt, acc, active, done)
    assert want == ([4, 2, 7, 3, 9, 2, 2, 2, 2], [1, 1, 1, 2, 4, -1, Sx + 1, 0, 1], [1, 1, 1, 0, 0, 1, 1, 1, 1], [0, 0, 0, 10, 1, 0, 0, 0, 0])
    dev = lambda v, dt: torch.tensor(v, dtype=dt, device="cuda")
    for as_bool in (True, False):
        d_tok, d_n, d_cn, d_st = dev(y, torch.long).view(T, 1), dev(n, torch.long), dev(c_n, torch.long), dev(state, torch.int32)
        d_act = dev(active, torch.bool if as_bool else torch.uint8)
        d_done = dev(done, torch.uint8)
        ops.step_constrain_advance(d_tok, d_n, d_cn, d_st, off.cuda(), tok.cuda(), nxt.cuda(), acc.cuda(), d_act, d_done)
        got = (d_cn.tolist(), d_st.tolist(), [int(v) for v in d_act.tolist()], d_done.tolist())
        assert got == want
        assert d_tok.view(-1).tolist() == y and d_n.tolist() == n        # only read
    # a second launch with nothing new emitted touches nothing, whatever the states are now
    ops.step_constrain_advance(d_tok, d_n, d_cn, d_st, off.cuda(), tok.cuda(), nxt.cuda(), acc.cuda(), d_act, d_done)
    assert (d_cn.tolist(), d_st.tolist(), [int(v) for v in d_act.tolist()], d_done.tolist()) == want
    # one tenant alone, and 70 tenants (more than one wave) with different automata per tenant
    one = [v[3:4] for v in (y, n, c_n, state, active, done)]
    d = [dev(one[0], torch.long), dev(one[1], torch.long), dev(one[2], torch.long), dev(one[3], torch.int32), dev(one[4], torch.uint8),
         dev(one[5], torch.uint8)]
    ops.step_constrain_advance(d[0], d[1], d[2], d[3], off[3:4].cuda(), tok[3:4].cuda(), nxt[3:4].cuda(), acc[3:4].cuda(), d[4], d[5])
    assert (d[2].tolist(), d[3].tolist(), d[4].tolist(), d[5].tolist()) == ([3], [2], [0], [10])
    from bitdelta_amd.constraint import TokenAutomaton
    g = torch.Generator().manual_seed(5)
    T2 = 70
    autos = []
    for t in range(T2):
        toks = torch.randperm(40, generator=g)[:6].tolist()
        b = TokenAutomaton.from_choices([toks[:2], toks[2:5], toks[5:]])
        autos.append((b.off, b.edge_tok, b.edge_next, b.accepting))
    off2, tok2, nxt2, acc2 = ref.pack(autos, 8, 8)
    st2 = torch.randint(-1, 7, (T2,), generator=g).tolist()
    y2 = [autos[t][1][t % 6] if t % 3 else int(torch.randint(0, 40, (1,), generator=g)) for t in range(T2)]
    n2, cn2 = [3] * T2, [3 if t % 11 == 0 else 2 for t in range(T2)]
    act2, done2 = [t % 5 != 0 for t in range(T2)], [0 if t % 5 else 2 for t in range(T2)]
    want2 = ref.advance(y2, n2, cn2, st2, off2, tok2, nxt2, acc2, act2, done2)
    d = [dev(y2, torch.long), dev(n2, torch.long), dev(cn2, torch.long), dev(st2, torch.int32), dev(act2, torch.bool), dev(done2, torch.uint8)]
    ops.step_constrain_advance(d[0], d[1], d[2], d[3], off2.cuda(), tok2.cuda(), nxt2.cuda(), acc2.cuda(), d[4], d[5])
    assert (d[2].tolist(), d[3].tolist(), [int(v) for v in d[4].tolist()], d[5].tolist()) == want2
    assert 8 in want2[3] and want2[1] != st2


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_graph_replay_equals_the_eager_sequence(ops, dtype):
    """the mask launch, a stand-in for the step end that writes tok and n, and the advance launch: captured once and replayed three times, against
    the same three steps run eagerly"""
    from bitdelta_amd.constraint import TokenAutomaton
    V, T, Sx, Ex = 2056, 3, 8, 8
    g = torch.Generator().manual_seed(77)
    autos = [TokenAutomaton.from_choices([[2050, 7], [2050, 8, 2047]]), TokenAutomaton.allowed_set([0, 2048, 2055]),
             TokenAutomaton.from_choices([[3], [4, 5]])]
    off, tok, nxt, acc = (x.cuda() for x in ref.pack([(a.off, a.edge_tok, a.edge_next, a.accepting) for a in autos], Sx, Ex))
    logits = [(torch.randn(T, V, generator=g) * 3).to(dtype).cuda() for _ in range(3)]
    stops = torch.tensor([[-1], [2055], [-1]], device="cuda")
    lg = torch.zeros(T, V, dtype=dtype, device="cuda")
    out = torch.zeros(T, V, dtype=dtype, device="cuda")
    st = dict(state=torch.zeros(T, dtype=torch.int32, device="cuda"), tokv=torch.zeros(T, 1, dtype=torch.long, device="cuda"),
              n=torch.ones(T, dtype=torch.long, device="cuda"), c_n=torch.ones(T, dtype=torch.long, device="cuda"),
              active=torch.ones(T, dtype=torch.bool, device="cuda"), done=torch.zeros(T, dtype=torch.uint8, device="cuda"))
    init = {k: v.clone() for k, v in st.items()}

    def seq():
        ops.step_constrain(lg, out, st["state"], off, tok, acc, stops, st["active"])
        st["tokv"].copy_(torch.where(st["active"], out.float().argmax(-1), st["tokv"].view(-1)).view(T, 1))      # the stand-in: argmax, n += 1
        st["n"].add_(st["active"].long())
        ops.step_constrain_advance(st["tokv"], st["n"], st["c_n"], st["state"], off, tok, nxt, acc, st["active"], st["done"])

    eager = []
    for i in range(3):
        lg.copy_(logits[i])
        seq()
        eager.append({k: v.cpu().clone() for k, v in st.items()} | {"out": out.cpu().clone()})
    assert eager[2]["done"].tolist() == [8, 0, 8] and eager[2]["active"].tolist() == [False, True, False]
    assert eager[0]["tokv"].view(-1).tolist()[0] == 2050 and eager[0]["state"].tolist()[0] == 1
    for k, v in init.items():
        st[k].copy_(v)
    out.zero_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        seq()
    torch.cuda.synchronize()
    for k, v in init.items():                                            # (a capture runs nothing; put back anyway)
        st[k].copy_(v)
    for i in range(3):
        lg.copy_(logits[i])
        graph.replay()
        torch.cuda.synchronize()
        for k in st:
            assert torch.equal(st[k].cpu(), eager[i][k]), (i, k)
        assert ref.same_bits(out.cpu(), eager[i]["out"]), i


def test_every_error_code_comes_back_with_nothing_launched(ops):
    """the entry points with real device buffers: each refusal of include/bitdelta_hip.h returns its code and the output, the state and the
    flags still hold what they held (tests/test_constraint_host.py walks every check on host pointers)"""
    from bitdelta_amd._lib import lib, ptr
    L = lib()
    V, R, Sx, Ex = 64, 2, 4, 8
    lg = torch.zeros(R, V, dtype=torch.float16, device="cuda")
    out = torch.full((R, V), 3.0, dtype=torch.float16, device="cuda")
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    state, off, et, en, acc = i32(R), i32(R, Sx + 1), i32(R, Ex), i32(R, Ex), torch.zeros(R, Sx, dtype=torch.uint8, device="cuda")
    stops = torch.full((R, 2), -1, dtype=torch.long, device="cuda")
    act, done = torch.ones(R, dtype=torch.uint8, device="cuda"), torch.zeros(R, dtype=torch.uint8, device="cuda")
    tok, n, c_n = (torch.zeros(R, dtype=torch.long, device="cuda") for _ in range(3))
    n += 1
    BAD_SHAPE, BAD_DTYPE, NULL = (L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None),
                                  L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 7, None), L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 0, None))

    def rows(V=V, sl=V, S=Sx, E=Ex, ns=2, R=R, dtype=0, logits=lg, edge_tok=et, step=False):
        a = (ptr(logits), sl, V, ptr(out), V, ptr(state), ptr(off), ptr(edge_tok), ptr(acc), S, E, ptr(stops), ns)
        return L.bd_srv_step_constrain(*a, ptr(act), R, dtype, None) if step else L.bd_srv_constrain_rows(*a, R, dtype, None)
    for step in (False, True):
        assert rows(V=60, step=step) == BAD_SHAPE and rows(sl=56, step=step) == BAD_SHAPE and rows(S=0, step=step) == BAD_SHAPE
        assert rows(E=-1, step=step) == BAD_SHAPE and rows(ns=65, step=step) == BAD_SHAPE and rows(R=-1, step=step) == BAD_SHAPE
        assert rows(dtype=2, step=step) == BAD_DTYPE and rows(logits=None, step=step) == NULL and rows(edge_tok=None, step=step) == NULL
        assert rows(R=0, step=step) == 0

    def adv(T=R, S=Sx, E=Ex, tokp=tok, nextp=en):
        return L.bd_srv_step_constrain_advance(ptr(tokp), ptr(n), ptr(c_n), ptr(state), ptr(off), ptr(et), ptr(nextp), ptr(acc), S, E, ptr(act),
                                               ptr(done), T, None)
    assert adv(T=-1) == BAD_SHAPE and adv(T=1025) == BAD_SHAPE and adv(S=0) == BAD_SHAPE and adv(E=(1 << 20) + 1) == BAD_SHAPE
    assert adv(tokp=None) == NULL and adv(nextp=None) == NULL and adv(T=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and c_n.tolist() == [0, 0] and act.tolist() == [1, 1] and done.tolist() == [0, 0] and state.tolist() == [0, 0]
    with pytest.raises(AssertionError):
        ops.constrain_rows(lg, state.long(), off, et, acc)
    with pytest.raises(AssertionError):
        ops.constrain_rows(lg, state, off, et, acc, torch.zeros(R, 65, dtype=torch.long, device="cuda"))
    with pytest.raises(Exception):
        ops.constrain_rows(lg.cpu(), state, off, et, acc)
    assert ops.constrain_rows(lg[:0], state[:0], off[:0], et[:0], acc[:0]).shape == (0, V)       # no rows: nothing is launched
