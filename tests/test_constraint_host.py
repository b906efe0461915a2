"""CPU-only checks of the constraint path: TokenAutomaton's three constructors build the CSR form they document, refuse what they document and
admission's check refuses the rest before anything is touched; the restatement (constraint_ref) agrees with the automaton's own host rule on
hand-made automata; a session made without constraints=True refuses a constraint; the three C-ABI symbols are in the header, the library, the
ctypes table and INTEGRATION.md, and answer their argument checks before any device call."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import constraint_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _csr(a):
    return a.n_states, a.off, a.edge_tok, a.edge_next, a.accepting


# ------------------------------------------------------------------------------------------------ 1. constructors
def test_from_choices_builds_the_trie():
    from bitdelta_amd.constraint import TokenAutomaton
    a = TokenAutomaton.from_choices([[5, 6], [5, 7], [5], [9]])
    # nodes in creation order: 0 root, 1 = [5], 2 = [5, 6], 3 = [5, 7], 4 = [9]
    assert _csr(a) == (5, [0, 2, 4, 4, 4, 4], [5, 9, 6, 7], [1, 4, 2, 3], [0, 1, 1, 1, 1])
    assert a.edges(0) == [(5, 1), (9, 4)] and a.edges(1) == [(6, 2), (7, 3)] and a.n_edges == 4
    assert a.accepting[1] and not a.is_final(1)                          # [5] is a prefix of two others: accepting, and it goes on
    assert [a.is_final(s) for s in range(5)] == [False, False, True, True, True]
    assert a.allowed(0) == [5, 9] and a.allowed(1, [3, -1]) == [3, 6, 7] and a.allowed(0, [3]) == [5, 9] and a.allowed(2, [3]) == [3]
    assert a.step(0, 5) == 1 and a.step(1, 7) == 3 and a.step(1, 3) == 1 and a.step(4, 9) == 4
    # duplicates collapse, the order of the choices only numbers the nodes, edges are sorted by token whatever the order
    assert _csr(TokenAutomaton.from_choices([[5, 6], [5, 7], [5], [9], [5, 7], [9], [5]])) == _csr(a)
    b = TokenAutomaton.from_choices([[9], [5, 7], (5, 6), [5]])
    assert b.edges(0) == [(5, 2), (9, 1)] and b.edges(2) == [(6, 4), (7, 3)] and b.accepting == [0, 1, 1, 1, 1]
    assert all(type(v) is int for v in b.off + b.edge_tok + b.edge_next + b.accepting)
    one = TokenAutomaton.from_choices([[3]])
    assert _csr(one) == (2, [0, 1, 1], [3], [1], [0, 1]) and one.is_final(1)
    for bad in ([], [[]], [[1], []], [[1, -2]], [[1.5]], [[True]], [["a"]]):
        with pytest.raises(ValueError):
            TokenAutomaton.from_choices(bad)


def test_from_edges_and_allowed_set_round_trip():
    from bitdelta_amd.constraint import TokenAutomaton
    edges = [(0, 40, 1), (0, 7, 0), (1, 3, 2), (1, 2, 1), (0, 8, 2)]
    a = TokenAutomaton.from_edges(3, edges, [False, True, True])
    assert _csr(a) == (3, [0, 3, 5, 5], [7, 8, 40, 2, 3], [0, 2, 1, 1, 2], [0, 1, 1])
    back = [(s, y, nx) for s in range(a.n_states) for y, nx in a.edges(s)]
    assert sorted(back) == sorted(edges)
    assert _csr(TokenAutomaton.from_edges(a.n_states, back, a.accepting)) == _csr(a)
    assert a.is_final(2) and not a.is_final(1) and not a.is_final(0)
    s = TokenAutomaton.allowed_set([9, 3, 3, 511, 0])
    assert _csr(s) == (1, [0, 4], [0, 3, 9, 511], [0, 0, 0, 0], [1]) and not s.is_final(0)
    assert s.allowed(0, [7]) == [0, 3, 7, 9, 511] and s.step(0, 9) == 0 and s.step(0, 7) == 0
    assert _csr(TokenAutomaton.allowed_set(torch.tensor([511, 9, 3, 0]).tolist())) == _csr(s)


@pytest.mark.parametrize("n_states,edges,accepting", [
    (2, [(0, -1, 1)], [0, 1]),                       # a negative token
    (2, [(0, 1 << 31, 1)], [0, 1]),                  # ... one that does not fit
    (2, [(0, 5, 2)], [0, 1]),                        # a next state out of range
    (2, [(0, 5, -1)], [0, 1]),
    (2, [(2, 5, 1)], [0, 1]),                        # a source state out of range
    (2, [(0, 5, 1), (0, 5, 0)], [0, 1]),             # a token twice within a state
    (2, [(0, 5, 1), (0, 6, 1), (0, 5, 1)], [0, 1]),
    (2, [(0, 5, 1)], [0, 0]),                        # state 1: not accepting, no edges
    (1, [], [0]),
    (0, [], []),                                     # no start state
    (2, [(0, 5, 1)], [0, 1, 1]),                     # flags for another number of states
    (2, [(0, 5)], [0, 1]),                           # not a triple
    (2, [(0, 5.5, 1)], [0, 1]),
    (2, [(0, True, 1)], [0, 1]),
])
def test_from_edges_refuses(n_states, edges, accepting):
    from bitdelta_amd.constraint import TokenAutomaton
    with pytest.raises(ValueError):
        TokenAutomaton.from_edges(n_states, edges, accepting)


def test_allowed_set_refuses():
    from bitdelta_amd.constraint import TokenAutomaton
    for bad in ([], [-1], [1.5], [None]):
        with pytest.raises(ValueError):
            TokenAutomaton.allowed_set(bad)


def test_admission_check_refuses_before_anything_is_touched():
    """TokenAutomaton.check is a pure function of host integers: what it refuses never reaches a device array"""
    from bitdelta_amd.constraint import TokenAutomaton
    a = TokenAutomaton.from_choices([[5, 6], [5, 7], [5], [9]])
    before = _csr(a)
    assert a.check(512, 5, 4, False) is a and a.check(10, 256, 4096, True) is a
    for kw in (dict(vocab=9), dict(max_states=4), dict(max_edges=3)):     # token 9 >= vocab; 5 states; 4 edges
        args = dict(dict(vocab=512, max_states=256, max_edges=4096, has_stop_ids=False), **kw)
        with pytest.raises(ValueError):
            a.check(**args)
    assert _csr(a) == before
    # a start state that is accepting and has no edges allows the request's stop ids and nothing else: without one, nothing at all
    lone = TokenAutomaton.from_edges(1, [], [1])
    with pytest.raises(ValueError):
        lone.check(512, 256, 4096, False)
    assert lone.check(512, 256, 4096, True) is lone
    # ... any OTHER such state is final and needs none: the request ends on reaching it (every leaf of a trie is one)
    assert a.is_final(2) and a.check(512, 256, 4096, False) is a
    # an accepting state WITH edges needs none either
    assert TokenAutomaton.allowed_set([1, 2]).check(512, 1, 2, False)


# ------------------------------------------------------------------------------------------------ 2. the restatement
def test_restatement_agrees_with_the_automatons_own_rule():
    from bitdelta_amd.constraint import TokenAutomaton
    V = 16
    autos = [TokenAutomaton.from_choices([[5, 6], [5, 7], [5], [9]]), TokenAutomaton.allowed_set([0, 7, 8, 15]),
             TokenAutomaton.from_edges(3, [(0, 1, 1), (1, 2, 2), (1, 1, 1), (2, 3, 0)], [0, 1, 0])]
    S, E = 6, 9
    off, tok, nxt, acc = ref.pack([(a.off, a.edge_tok, a.edge_next, a.accepting) for a in autos], S, E)
    stops = [[3, -1], [], [14, 2]]
    for r, a in enumerate(autos):
        for s in range(a.n_states):
            assert sorted(ref.allowed(s, off[r].tolist(), tok[r].tolist(), acc[r].tolist(), stops[r], V)) == a.allowed(s, stops[r])
            assert ref.is_final(s, off[r].tolist(), acc[r].tolist(), E) == a.is_final(s)
            for y in range(V):
                got = ref.advance([y], [2], [1], [s], off[r:r + 1], tok[r:r + 1], nxt[r:r + 1], acc[r:r + 1], [1], [0])
                want = a.step(s, y)
                assert got == ([2], [want], [0 if a.is_final(want) else 1], [8 if a.is_final(want) else 0]), (r, s, y)
        for s in (-1, S, S + 7):                                         # nothing is constrained
            assert ref.allowed(s, off[r].tolist(), tok[r].tolist(), acc[r].tolist(), stops[r], V) is None
    # the mask on a hand-made row: kept bits are the input's, the rest is -inf; an unconstrained row is a copy; an inactive row keeps `out`
    l = torch.tensor([[float(i) - 4.0 for i in range(V)]] * 3, dtype=torch.float16)
    l[0, 5], l[0, 6], l[1, 0] = float("nan"), -0.0, float("inf")
    m = ref.mask(l, [1, 0, -1], off, tok, acc, torch.tensor([[3, -1], [-1, -1], [14, 2]]))
    ninf = float("-inf")
    assert [i for i in range(V) if m[0, i] != ninf] == [3, 6, 7] and [i for i in range(V) if m[1, i] != ninf] == [0, 7, 8, 15]
    assert ref.same_bits(m[0, [3, 6, 7]], l[0, [3, 6, 7]]) and ref.same_bits(m[2], l[2]) and float(m[1, 0]) == float("inf")
    assert bool((m[0, 5].view(torch.int16) == ref.NEG_INF_BITS[torch.float16]))      # a NaN outside the set is masked like anything else
    prev = torch.full_like(l, 9.0)
    m2 = ref.mask(l, [1, 0, -1], off, tok, acc, None, active=[True, False, True], out=prev)
    assert [i for i in range(V) if m2[0, i] != ninf] == [6, 7] and ref.same_bits(m2[1], prev[1]) and ref.same_bits(m2[2], l[2])
    # the counter discipline: n == c_n touches nothing; an inactive tenant's state moves and its done byte stays; -1 stays -1
    r0 = (off[0:1], tok[0:1], nxt[0:1], acc[0:1])
    assert ref.advance([6], [3], [3], [1], *r0, [1], [0]) == ([3], [1], [1], [0])
    assert ref.advance([6], [4], [3], [1], *r0, [0], [2]) == ([4], [2], [0], [2])
    assert ref.advance([6], [4], [3], [1], *r0, [1], [1]) == ([4], [2], [0], [9])
    assert ref.advance([6], [4], [3], [-1], *r0, [1], [0]) == ([4], [-1], [1], [0])


# ------------------------------------------------------------------------------------------------ 3. a session without the flag
def test_a_session_without_constraints_refuses_one():
    """the refusal sits where _params' does, in front of every device call: it needs no device"""
    from bitdelta_amd.constraint import TokenAutomaton
    from bitdelta_amd.serving_loop import TenantDecoder, TenantSession
    a = TokenAutomaton.allowed_set([1, 2])
    plain = object.__new__(TenantSession)
    plain.constraints = False
    assert plain._constraint_arg(None) is None
    with pytest.raises(ValueError, match="constraints=True"):
        plain._constraint_arg(a)
    with_flag = object.__new__(TenantSession)
    with_flag.constraints = True
    assert with_flag._constraint_arg(a) is a and with_flag._constraint_arg(None) is None
    for bad in ([[1, 2]], "x", 5, {1: 2}):
        with pytest.raises(ValueError):
            with_flag._constraint_arg(bad)
    for fn in (TenantSession.submit, TenantSession.extend, TenantSession.submit_all):
        assert inspect.signature(fn).parameters["constraint"].default is None
    p = inspect.signature(TenantDecoder.session).parameters
    assert (p["constraints"].default, p["max_constraint_states"].default, p["max_constraint_edges"].default) == (False, 256, 4096)


# ------------------------------------------------------------------------------------------------ 4. symbols and argument checks
NAMES = {"bd_srv_constrain_rows": 16, "bd_srv_step_constrain": 17, "bd_srv_step_constrain_advance": 14}


def test_symbols_in_header_library_ctypes_table_and_integration_notes():
    from bitdelta_amd import _lib, serving_ops
    src = open(os.path.join(ROOT, "include", "bitdelta_hip.h")).read()
    for name, val in (("STATES", serving_ops.CONSTRAINT_STATES_MAX), ("EDGES", serving_ops.CONSTRAINT_EDGES_MAX), ("STOP", serving_ops.CONSTRAINT_STOP_MAX)):
        assert re.search(r"#define\s+BD_CONSTRAINT_%s_MAX\s+%d\b" % (name, val), src)
    txt = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    for name, nargs in NAMES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert decl, name + " is not declared in include/bitdelta_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == nargs
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
        assert hasattr(_lib.lib(), name)
    assert callable(serving_ops.constrain_rows) and callable(serving_ops.step_constrain) and callable(serving_ops.step_constrain_advance)


def test_entry_points_validate_before_any_device_call():
    from bitdelta_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255            # an aligned, non-null host address: never dereferenced by the checks
    BAD_SHAPE, BAD_DTYPE, NULL = (L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None),
                                  L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 7, None), L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 0, None))
    assert len({BAD_SHAPE, BAD_DTYPE, NULL, 0}) == 4
    good = dict(logits=base, sl=72, V=64, out=base, so=80, state=base, off=base, edge_tok=base, accepting=base, S=4, E=9, stop_ids=base, ns=2,
                active=base, R=2, dtype=0)

    def rows(**kw):
        a = dict(good, **kw)
        return L.bd_srv_constrain_rows(a["logits"], a["sl"], a["V"], a["out"], a["so"], a["state"], a["off"], a["edge_tok"], a["accepting"], a["S"],
                                       a["E"], a["stop_ids"], a["ns"], a["R"], a["dtype"], None)

    def step(**kw):
        a = dict(good, **kw)
        return L.bd_srv_step_constrain(a["logits"], a["sl"], a["V"], a["out"], a["so"], a["state"], a["off"], a["edge_tok"], a["accepting"], a["S"],
                                       a["E"], a["stop_ids"], a["ns"], a["active"], a["R"], a["dtype"], None)
    ptrs = ("logits", "out", "state", "off", "edge_tok", "accepting", "stop_ids")
    for call in (rows, step):
        assert call(R=0) == 0 and call(R=0, active=None, **{q: None for q in ptrs}) == 0                            # launches nothing
        assert call(R=-1) == BAD_SHAPE
        assert call(V=60) == BAD_SHAPE and call(V=0) == BAD_SHAPE and call(V=-8) == BAD_SHAPE                       # V % 8, V < 1
        assert call(V=(1 << 22) + 8, sl=(1 << 22) + 8, so=(1 << 22) + 8) == BAD_SHAPE                                # V > 2^22
        for q in ("sl", "so"):
            assert call(**{q: 68}) == BAD_SHAPE and call(**{q: 56}) == BAD_SHAPE, q                                   # stride % 8, stride < V
        for q in ("logits", "out"):
            assert call(**{q: base + 8}) == BAD_SHAPE, q                                                              # 16-byte alignment
        for q in ("state", "off", "edge_tok"):
            assert call(**{q: base + 2}) == BAD_SHAPE, q
        assert call(stop_ids=base + 4) == BAD_SHAPE
        assert call(S=0) == BAD_SHAPE and call(S=65537) == BAD_SHAPE and call(E=-1) == BAD_SHAPE and call(E=(1 << 20) + 1) == BAD_SHAPE
        assert call(ns=-1) == BAD_SHAPE and call(ns=65) == BAD_SHAPE and call(R=65536) == BAD_SHAPE
        for q in ptrs:
            assert call(**{q: None}) == NULL, q
        # null lists are fine at E = 0 / ns = 0, and the largest sizes are: the call gets past the NULL and range checks to the layout check
        assert call(E=0, edge_tok=None, ns=0, stop_ids=None, sl=68) == BAD_SHAPE and call(S=65536, E=1 << 20, ns=64, sl=68) == BAD_SHAPE
        assert call(E=1, edge_tok=None, sl=68) == NULL and call(ns=1, stop_ids=None, sl=68) == NULL
        assert call(dtype=2) == BAD_DTYPE and call(dtype=7) == BAD_DTYPE and call(dtype=-1) == BAD_DTYPE
        # the order of bd_srv_penalize_rows: shape of R / V, dtype, R == 0, the sizes, null pointers, layout
        assert call(R=-1, dtype=7) == BAD_SHAPE and call(R=0, dtype=7) == BAD_DTYPE and call(R=0, S=0, V=60) == 0
        assert call(S=0, logits=None) == BAD_SHAPE and call(logits=None, V=60) == NULL
    assert step(active=None) == NULL

    g2 = dict(tok=base, n=base, c_n=base, state=base, off=base, edge_tok=base, edge_next=base, accepting=base, S=4, E=9, active=base, done=base, T=3)

    def adv(**kw):
        a = dict(g2, **kw)
        return L.bd_srv_step_constrain_advance(a["tok"], a["n"], a["c_n"], a["state"], a["off"], a["edge_tok"], a["edge_next"], a["accepting"],
                                               a["S"], a["E"], a["active"], a["done"], a["T"], None)
    p2 = ("tok", "n", "c_n", "state", "off", "edge_tok", "edge_next", "accepting", "active", "done")
    assert adv(T=0) == 0 and adv(T=0, **{q: None for q in p2}) == 0 and adv(T=0, S=0) == 0
    assert adv(T=-1) == BAD_SHAPE and adv(T=1025) == BAD_SHAPE
    assert adv(S=0) == BAD_SHAPE and adv(S=65537) == BAD_SHAPE and adv(E=-1) == BAD_SHAPE and adv(E=(1 << 20) + 1) == BAD_SHAPE
    for q in p2:
        assert adv(**{q: None}) == NULL, q
    assert adv(S=0, tok=None) == BAD_SHAPE
    for q in ("tok", "n", "c_n"):
        assert adv(**{q: base + 4}) == BAD_SHAPE, q
    for q in ("state", "off", "edge_tok", "edge_next"):
        assert adv(**{q: base + 2}) == BAD_SHAPE, q
    # E = 0: no edge arrays needed; the call gets past the NULL check to the layout check behind it
    assert adv(E=0, edge_tok=None, edge_next=None, tok=base + 4) == BAD_SHAPE and adv(E=1, edge_next=None, tok=base + 4) == NULL
