"""CPU-only checks of the stop-sequence path: the table builder keeps the caller's order, pads, and refuses what it documents; the package's
host scanner (the rule admission applies to the first token) agrees with the restatement (stop_seq_ref) on random token lists over three
symbols -- overlaps, self-overlapping sequences, one sequence a suffix or a prefix of another all occur -- and on hand cases for the tie rule,
hold on a hit, k <= n and the prompt never taking part; a session made without stop_sequences=True refuses them; submit_all tells one list for
all from a list per tenant by depth; the C-ABI symbol is in the header, the library, the ctypes table and INTEGRATION.md and answers its
argument checks, in the documented order, before any device call."""
import ctypes
import inspect
import os
import random
import re

import pytest

import stop_seq_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the table
def test_table_keeps_order_and_pads():
    from bitdelta_amd.serving_loop import stop_sequence_table
    tok, lens = stop_sequence_table([[7, 8, 9], (3,), [8, 9]], 4, 5, 16)
    assert tok == [[7, 8, 9, -1, -1], [3, -1, -1, -1, -1], [8, 9, -1, -1, -1], [-1] * 5] and lens == [3, 1, 2, 0]
    assert all(type(v) is int for row in tok for v in row) and all(type(v) is int for v in lens)
    for none in (None, (), []):
        assert stop_sequence_table(none, 2, 3, 16) == ([[-1] * 3, [-1] * 3], [0, 0])
    # equal sequences are kept twice, in place: hit is an index into the caller's list
    assert stop_sequence_table([[1], [1]], 2, 1)[1] == [1, 1]
    # the sizes at the ABI maxima, and ids at both ends of the vocabulary
    from bitdelta_amd import serving_ops as ops
    Q, W = ops.STOP_SEQ_MAX, ops.STOP_SEQ_LEN_MAX
    assert (Q, W) == (16, 32)
    full = [[(q + j) % 512 for j in range(W)] for q in range(Q)]
    tok, lens = stop_sequence_table(full, Q, W, 512)
    assert tok == full and lens == [W] * Q
    assert stop_sequence_table([[0, 511]], 1, 2, 512) == ([[0, 511]], [2])
    import numpy as np
    assert stop_sequence_table([[np.int64(4), np.int32(5)]], 1, 2, 8) == ([[4, 5]], [2])       # integers by __index__, as sampling_params takes them


@pytest.mark.parametrize("bad,Q,W,vocab", [
    ([[]], 4, 8, 512),                              # an empty sequence
    ([[1, 2], []], 4, 8, 512),
    ([[1.0]], 4, 8, 512),                           # a non-integer id
    ([[True]], 4, 8, 512),
    ([["a"]], 4, 8, 512),
    ([[None]], 4, 8, 512),
    ([[512]], 4, 8, 512),                           # outside the vocabulary
    ([[3, -1]], 4, 8, 512),
    ([[2 ** 31]], 4, 8, None),
    ([[1]] * 5, 4, 8, 512),                         # one sequence too many
    ([[1] * 9], 4, 8, 512),                         # one token too long
    ([[1]] * 17, 16, 32, 512),                      # ... past the ABI maxima
    ([[1] * 33], 16, 32, 512),
    ([1, 2], 4, 8, 512),                            # a flat list of ids is not a list of sequences
    ("ab", 4, 8, 512),
    (5, 4, 8, 512),
    ({1: 2}, 4, 8, 512),
])
def test_table_refuses(bad, Q, W, vocab):
    from bitdelta_amd.serving_loop import stop_sequence_table
    with pytest.raises(ValueError):
        stop_sequence_table(bad, Q, W, vocab)


def test_sizes_at_the_maxima_pass_and_one_past_fail():
    from bitdelta_amd.serving_loop import stop_sequence_table
    assert stop_sequence_table([[1]] * 4, 4, 8, 512)[1] == [1] * 4
    assert stop_sequence_table([[1] * 8], 4, 8, 512)[1] == [8, 0, 0, 0]
    assert stop_sequence_table([[1]] * 16, 16, 32, 512)[1] == [1] * 16
    assert stop_sequence_table([[1] * 32], 16, 32, 512)[1][0] == 32


# ------------------------------------------------------------------------------------------------ 2. the scanner
def test_host_scanner_against_the_restatement_on_three_symbols():
    from bitdelta_amd.serving_loop import stop_sequence_scan
    rng = random.Random(20240521)
    fixed = [[[0, 0, 0]], [[0, 1, 0, 1]], [[0, 1], [1]], [[1, 2], [0, 1, 2]], [[0, 1, 2], [1, 2]], [[2, 2], [2, 2, 2]], [[0], [0]]]
    hits = holds = 0
    for i in range(600):
        seqs = fixed[i] if i < len(fixed) else [[rng.randrange(3) for _ in range(rng.randint(1, 5))] for _ in range(rng.randint(0, 4))]
        y = [rng.randrange(3) for _ in range(rng.randint(0, 9))]
        for m in range(len(y) + 1):
            want = ref.scan(y[:m], seqs)
            assert stop_sequence_scan(y[:m], seqs) == want, (y[:m], seqs)
            hits += want[0] >= 0
            holds += want[1] > 0
    assert hits > 300 and holds > 300


def test_hand_cases():
    from bitdelta_amd.serving_loop import stop_sequence_scan
    for scan in (ref.scan, stop_sequence_scan):
        assert scan([5, 6, 7], [[9], [6, 7], [7]]) == (1, 0)            # two match: the lowest index wins ...
        assert scan([5, 6, 7], [[9], [7], [6, 7]]) == (1, 0)            # ... not the longest
        assert scan([5, 6, 7], [[7, 8], [6, 7]]) == (1, 0)              # hold is 0 on a hit although [7] begins sequence 0
        assert scan([5, 6, 7], [[7, 8], [6, 7, 8, 9]]) == (-1, 2)       # the longest prefix over all sequences
        assert scan([7], [[7, 7, 7]]) == (-1, 1) and scan([7, 7], [[7, 7, 7]]) == (-1, 2) and scan([7, 7, 7], [[7, 7, 7]]) == (0, 0)
        assert scan([7, 7, 7, 7], [[7, 7, 7]]) == (0, 0)                # (a session has stopped a step earlier)
        assert scan([6, 7], [[5, 6, 7]]) == (-1, 0)                     # len > n: no hit; and [6, 7] is no PREFIX of it
        assert scan([5, 6], [[5, 6, 7]]) == (-1, 2)                     # k == n is allowed, k <= n
        assert scan([6], [[5, 6], [6, 5, 6]]) == (-1, 1)
        assert scan([], [[5]]) == (-1, 0) and scan([5], []) == (-1, 0) and scan([5], [[5]]) == (0, 0)
        assert scan([5, 6, 5], [[5, 6]]) == (-1, 1)                     # a match earlier in the turn is not a match at its end
        # the prompt never takes part: the functions see the turn only, so a sequence whose head sits in the prompt does not match
        prompt, turn = [1, 2, 3], [4, 5]
        assert scan(turn, [[3, 4, 5]]) == (-1, 0) and scan(prompt + turn, [[3, 4, 5]]) == (0, 0)
    assert ref.scan([5, -1], [[5, -1]]) == (-1, 0)                       # a negative table entry matches nothing
    assert ref.first_hit([1, 2, 3, 2, 3], [[2, 3]]) == (3, 0) and ref.first_hit([1, 2], [[3]]) == (2, -1)


def test_restatement_of_the_launch():
    out = [[5, 6, 7, 0], [5, 6, 7, 0], [5, 6, 7, 0], [5, 6, 7, 0]]
    tab = [[[6, 7], [7, -1]]] * 4
    got = ref.step(out, [3, 3, 5, 3], [2, 3, 4, 2], tab, [[2, 1], [2, 1], [2, 1], [3, 1]], [-1, 4, 1, -1], [1, 1, 1, 1], [1, 1, 1, 0], [0, 0, 0, 2])
    # tenant 0 hits sequence 0; 1 did not move (a stale hit stays); 2 is past the row; 3: length 3 > W counts as unused, [7] hits, done 2 | 16
    assert got == ([3, 3, 5, 3], [0, 4, -1, 1], [0, 1, 0, 0], [0, 1, 1, 0], [16, 0, 0, 18])


# ------------------------------------------------------------------------------------------------ 3. the session's arguments
def _bare(flag, T=4, Q=4, W=8, vocab=512):
    import torch
    from bitdelta_amd.serving_loop import TenantSession
    s = object.__new__(TenantSession)
    s.stop_sequences, s.T = flag, T
    if flag:
        s.ss_tok = torch.zeros(T, Q, W, dtype=torch.int32)

        class _Dec:
            lm_head = torch.zeros(1, vocab, 8)
        s.dec = _Dec()
    return s


def test_a_session_without_the_feature_refuses_them():
    from bitdelta_amd.serving_loop import TenantDecoder, TenantSession
    plain = _bare(False)
    for empty in ((), [], None):
        assert plain._stop_sequences_arg(empty) is None
    for v in ([[1]], [[]], "x", 5):
        with pytest.raises(ValueError, match="stop_sequences=True"):
            plain._stop_sequences_arg(v)
    on = _bare(True)
    seqs, (tok, lens) = on._stop_sequences_arg([[3, 4], (5,)])
    assert seqs == [[3, 4], [5]] and lens == [2, 1, 0, 0] and tok[0] == [3, 4] + [-1] * 6
    assert on._stop_sequences_arg(())[0] == [] and on._stop_sequences_arg(None)[1][1] == [0] * 4
    for bad in ([[]], [[512]], [[1]] * 5, [[1] * 9], [[1.5]]):
        with pytest.raises(ValueError):
            on._stop_sequences_arg(bad)
    for fn in (TenantSession.submit, TenantSession.extend, TenantSession.submit_all):
        assert inspect.signature(fn).parameters["stop_sequences"].default == ()
    p = inspect.signature(TenantDecoder.session).parameters
    assert (p["stop_sequences"].default, p["max_stop_sequences"].default, p["max_stop_sequence_len"].default) == (False, 4, 8)
    for name in ("stop_match", "streamable"):
        with pytest.raises(ValueError, match="stop_sequences=True"):
            getattr(plain, name)(0)
    assert "16 = " in TenantSession.__doc__


def test_submit_all_tells_one_list_for_all_from_a_list_per_tenant():
    s = _bare(True, T=2)
    one = [[5, 6], [7]]
    assert s._per_tenant_stop_sequences(one) == [one, one]               # elements hold ids directly: ONE list of two sequences, for all
    assert s._per_tenant_stop_sequences(()) == [(), ()] and s._per_tenant_stop_sequences(None) == [None, None]
    per = [[[5, 6]], [[7], [8, 9]]]
    assert s._per_tenant_stop_sequences(per) == per                      # elements are lists of lists: one list per tenant
    assert s._per_tenant_stop_sequences([[[5, 6]], []]) == [[[5, 6]], []]
    assert s._per_tenant_stop_sequences([[], []]) == [[], []]            # two tenants without sequences
    assert s._per_tenant_stop_sequences(([(5, 6)], ())) == [[(5, 6)], ()]
    with pytest.raises(ValueError, match="for 2 tenants"):
        s._per_tenant_stop_sequences([[[5]], [[6]], [[7]]])
    with pytest.raises(ValueError, match="for 2 tenants"):
        s._per_tenant_stop_sequences([[]])
    mixed = s._per_tenant_stop_sequences([[5], []])                      # an id at depth two: one list for all -- whose empty sequence is refused
    assert mixed == [[[5], []]] * 2
    with pytest.raises(ValueError, match="empty"):
        s._stop_sequences_arg(mixed[0])
    four = _bare(True, T=4)
    assert four._per_tenant_stop_sequences(one) == [one] * 4


def test_session_sizes_are_validated_against_the_abi_maxima():
    from bitdelta_amd.serving_loop import TenantSession
    for kw in (dict(max_stop_sequences=0), dict(max_stop_sequences=17), dict(max_stop_sequence_len=0), dict(max_stop_sequence_len=33),
               dict(max_stop_sequences=True), dict(max_stop_sequence_len=2.0)):
        with pytest.raises(ValueError, match="max_stop_sequence"):
            TenantSession(None, stop_sequences=True, **kw)               # refused before the decoder is looked at


# ------------------------------------------------------------------------------------------------ 4. the symbol and its argument checks
def test_symbol_in_header_library_ctypes_table_and_integration_notes():
    from bitdelta_amd import _lib, serving_ops
    src = open(os.path.join(ROOT, "include", "bitdelta_hip.h")).read()
    assert re.search(r"#define\s+BD_STOP_SEQ_MAX\s+%d\b" % serving_ops.STOP_SEQ_MAX, src)
    assert re.search(r"#define\s+BD_STOP_SEQ_LEN_MAX\s+%d\b" % serving_ops.STOP_SEQ_LEN_MAX, src)
    txt = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    name = "bd_srv_step_stop_sequences"
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
    assert decl, name + " is not declared in include/bitdelta_hip.h"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == 15
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert hasattr(_lib.lib(), name) and callable(serving_ops.step_stop_sequences)


def test_entry_point_validates_before_any_device_call():
    from bitdelta_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255            # an aligned, non-null host address: never dereferenced by the checks
    BAD_SHAPE, NULL = L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None), L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 0, None)
    assert len({BAD_SHAPE, NULL, 0}) == 3
    good = dict(out=base, s_out=48, out_cap=40, n=base, ss_n=base, seq_tok=base, seq_len=base, Q=4, W=8, hit=base, hold=base, active=base,
                done=base, T=3)
    order = ("out", "s_out", "out_cap", "n", "ss_n", "seq_tok", "seq_len", "Q", "W", "hit", "hold", "active", "done", "T")
    ptrs = ("out", "n", "ss_n", "seq_tok", "seq_len", "hit", "hold", "active", "done")

    def call(**kw):
        a = dict(good, **kw)
        return L.bd_srv_step_stop_sequences(*[a[k] for k in order], None)
    nulls = {q: None for q in ptrs}
    # 1. the shape of T / Q / W / out_cap / s_out
    assert call(T=-1) == BAD_SHAPE and call(T=65536) == BAD_SHAPE
    assert call(Q=0) == BAD_SHAPE and call(Q=17) == BAD_SHAPE and call(W=0) == BAD_SHAPE and call(W=33) == BAD_SHAPE
    assert call(out_cap=-1) == BAD_SHAPE and call(s_out=39) == BAD_SHAPE
    assert call(T=-1, **nulls) == BAD_SHAPE and call(Q=17, **nulls) == BAD_SHAPE and call(T=0, Q=0) == BAD_SHAPE      # ... before anything else
    # 2. T == 0: nothing is launched, whatever the pointers are
    assert call(T=0) == 0 and call(T=0, **nulls) == 0 and call(T=0, out=base + 4) == 0
    # 3. null pointers, in front of the alignment
    for q in ptrs:
        assert call(**{q: None}) == NULL, q
    assert call(out=None, n=base + 4) == NULL and call(done=None, hit=base + 2) == NULL
    # 4. alignment: 8 bytes for the int64 arrays, 4 for the int32 ones; the flags are bytes
    for q in ("out", "n", "ss_n"):
        assert call(**{q: base + 4}) == BAD_SHAPE, q
    for q in ("seq_tok", "seq_len", "hit", "hold"):
        assert call(**{q: base + 2}) == BAD_SHAPE, q
    # the largest sizes get past the range checks to the ones behind them
    assert call(Q=16, W=32, T=65535, out=None) == NULL and call(out_cap=0, s_out=0, out=None) == NULL
