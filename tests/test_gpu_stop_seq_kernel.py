"""GPU tests of bd_srv_step_stop_sequences (serving_ops.step_stop_sequences): EXACT equality of hit / hold / ss_n / active / done with the
restatement of the definition (tests/stop_seq_ref.py), at T in {1, 3, 16} and (Q, W) in {(1, 1), (4, 3), (16, 32)} with rows of 40 tokens,
through a contiguous `out` and through a strided view of a wider poisoned buffer whose gaps must survive; every case the header names; the
same answers from a second launch and from a captured graph; every argument-check return code in its documented order."""
import random

import pytest
import torch

import stop_seq_ref as ref
from canary import POISON

pytestmark = pytest.mark.gpu

CAP = 40
TS = [1, 3, 16]
QWS = [(1, 1), (4, 3), (16, 32)]
POISON64 = int.from_bytes(bytes([POISON]) * 8, "little")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib, serving_ops
    _lib.lib()
    return serving_ops


class Out:
    """the output rows [T, cap] on the device: contiguous, or (strided) rows 1 .. T, columns 8 .. 8 + cap of a poisoned [T + 2, cap + 24]
    buffer -- row stride cap + 24, every gap and margin holding the canary pattern"""

    def __init__(self, rows, strided, cap=CAP):
        T = len(rows)
        host = torch.tensor([list(r[:cap]) for r in rows], dtype=torch.long).reshape(T, cap)
        self.host = host
        if strided:
            self.buf = torch.full((T + 2, cap + 24), POISON64, dtype=torch.long, device="cuda")
            self.view = self.buf[1:T + 1, 8:8 + cap]
            self.view.copy_(host)
            assert self.view.stride(0) == cap + 24 or T == 1
        else:
            self.buf = None
            self.view = host.cuda()

    def intact(self):
        """the launch only reads `out`: the rows hold what they held, and no byte of the gaps changed"""
        if not torch.equal(self.view.cpu(), self.host):
            return False
        if self.buf is None:
            return True
        keep = self.view.clone()
        self.view.fill_(POISON64)
        ok = bool((self.buf.view(torch.uint8) == POISON).all())
        self.view.copy_(keep)
        return ok


def launch(ops, case, strided=False, as_bool=True, cap=CAP):
    """one launch of a host case (dict of lists, stop_seq_ref.step's arguments); returns (ss_n, hit, hold, active, done) as lists"""
    dev = lambda v, dt: torch.tensor(v, dtype=dt, device="cuda")
    out = Out(case["out"], strided, cap)
    T = len(case["n"])
    Q, W = len(case["seq_tok"][0]), len(case["seq_tok"][0][0])
    d = dict(n=dev(case["n"], torch.long), ss_n=dev(case["ss_n"], torch.long), seq_tok=dev(case["seq_tok"], torch.int32).reshape(T, Q, W),
             seq_len=dev(case["seq_len"], torch.int32).reshape(T, Q), hit=dev(case["hit"], torch.int32), hold=dev(case["hold"], torch.int32),
             active=dev(case["active"], torch.bool if as_bool else torch.uint8), done=dev(case["done"], torch.uint8))
    ops.step_stop_sequences(out.view, d["n"], d["ss_n"], d["seq_tok"], d["seq_len"], d["hit"], d["hold"], d["active"], d["done"])
    torch.cuda.synchronize()
    assert out.intact()
    assert d["n"].tolist() == list(case["n"]) and d["seq_tok"].tolist() == [list(map(list, t)) for t in case["seq_tok"]]      # only read
    assert d["seq_len"].tolist() == [list(t) for t in case["seq_len"]]
    return d["ss_n"].tolist(), d["hit"].tolist(), d["hold"].tolist(), [int(v) for v in d["active"].tolist()], d["done"].tolist()


def want(case, cap=CAP):
    return ref.step(case["out"], case["n"], case["ss_n"], case["seq_tok"], case["seq_len"], case["hit"], case["hold"], case["active"],
                    case["done"], out_cap=cap)


def table(seqs_per_tenant, Q, W):
    """[T][Q][W] ids padded with -1 and [T][Q] lengths from one list of sequences per tenant"""
    tok = [[list(s) + [-1] * (W - len(s)) for s in seqs] + [[-1] * W] * (Q - len(seqs)) for seqs in seqs_per_tenant]
    return tok, [[len(s) for s in seqs] + [0] * (Q - len(seqs)) for seqs in seqs_per_tenant]


def random_case(T, Q, W, rng, cap=CAP):
    """tenants over a 3-symbol alphabet: random tables (short and long sequences, unused slots), random rows, every n from 0 to cap, moved and
    unmoved counters, stale results, live and retired tenants; every third tenant has one of its sequences planted at the end of its tokens"""
    c = dict(out=[], n=[], ss_n=[], seq_tok=[], seq_len=[], hit=[], hold=[], active=[], done=[])
    for t in range(T):
        seqs = [[rng.randrange(3) for _ in range(rng.choice([0, 1, min(2, W), min(3, W), W, rng.randint(0, W)]))] for _ in range(Q)]
        row = [rng.randrange(3) for _ in range(cap)]
        n = rng.choice([0, 1, 2, cap, rng.randint(0, cap), rng.randint(0, cap)])
        full = [s for s in seqs if s]
        if t % 3 == 0 and full:
            s = rng.choice(full)
            if len(s) <= n:
                row[n - len(s):n] = s
        tok, lens = table([seqs], Q, W)
        c["out"].append(row)
        c["n"].append(n)
        c["ss_n"].append(n if rng.random() < 0.15 else n - 1)
        c["seq_tok"].append(tok[0])
        c["seq_len"].append(lens[0])
        c["hit"].append(rng.choice([-1, -1, 0, Q - 1]))
        c["hold"].append(rng.choice([0, 0, 1, W - 1]))
        a = rng.random() < 0.7
        c["active"].append(int(a))
        c["done"].append(0 if a else rng.choice([1, 2, 4, 3]))
    return c


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("QW", QWS, ids=lambda v: "Q%dW%d" % v)
@pytest.mark.parametrize("T", TS)
def test_against_the_restatement(ops, T, QW, strided):
    Q, W = QW
    rng = random.Random(1000 * T + 10 * Q + W)
    hits = holds = 0
    for _ in range(max(6, 48 // T)):                                     # (at least 48 tenant-launches per case)
        c = random_case(T, Q, W, rng)
        got, exp = launch(ops, c, strided), want(c)
        assert got == exp
        moved = [t for t in range(T) if c["n"][t] != c["ss_n"][t]]
        hits += sum(exp[1][t] >= 0 for t in moved)
        holds += sum(exp[2][t] > 0 for t in moved)
    assert hits > 0 and (holds > 0 or W == 1)                            # (a one-token sequence has no proper prefix to hold)


def _one(y, seqs, Q=16, W=32, n=None, cap=CAP, **kw):
    """a one-tenant case: tokens y (the row is padded with 7s), the moved counter, nothing stale"""
    n = len(y) if n is None else n
    tok, lens = table([seqs], Q, W)
    c = dict(out=[list(y) + [7] * (cap - len(y))], n=[n], ss_n=[n - 1], seq_tok=tok, seq_len=lens, hit=[-1], hold=[0], active=[1], done=[0])
    c.update(kw)
    return c


def test_lengths_around_n_and_the_row_capacity(ops):
    s = [1, 2, 3]
    for strided in (False, True):
        # n < len: no hit, the tokens are a prefix (hold) or not
        assert launch(ops, _one([1, 2], [s]), strided) == ([2], [-1], [2], [1], [0])
        assert launch(ops, _one([2, 3], [s]), strided) == ([2], [-1], [0], [1], [0])
        # n == len
        assert launch(ops, _one([1, 2, 3], [s]), strided) == ([3], [0], [0], [0], [16])
        # n == out_cap: the last element of the row is read
        y = [0] * (CAP - 3) + s
        assert launch(ops, _one(y, [s]), strided) == ([CAP], [0], [0], [0], [16])
        full = list(range(100, 100 + 32))
        y = [0] * (CAP - 32) + full
        assert launch(ops, _one(y, [[9], full]), strided) == ([CAP], [1], [0], [0], [16])
        # n > out_cap: nothing is compared -- a stale hit and hold are replaced by -1 / 0, the tenant goes on, the counter follows
        c = _one(y, [s, full], n=CAP + 1, hit=[1], hold=[5])
        assert launch(ops, c, strided) == want(c) == ([CAP + 1], [-1], [0], [1], [0])
        c = _one(y, [full], n=2 ** 40, hit=[0])
        assert launch(ops, c, strided) == want(c) == ([2 ** 40], [-1], [0], [1], [0])
        c = _one(y, [full], n=-3, hit=[0])
        assert launch(ops, c, strided) == want(c) == ([-3], [-1], [0], [1], [0])
        # n == 0 (a counter that moved back): nothing to compare either
        c = dict(_one([], [[7]]), ss_n=[5])
        assert launch(ops, c, strided) == want(c) == ([0], [-1], [0], [1], [0])


def test_a_near_miss_at_every_position_of_a_32_token_sequence(ops):
    s = [3 + (j * 5) % 11 for j in range(32)]                            # (self-overlaps are few: 11 values over 32 places)
    T = 33
    rows, exp_hold = [], []
    for j in range(32):
        y = list(s)
        y[j] = 2                                                         # (2 does not occur in s)
        rows.append([0] * (CAP - 32) + y)
    rows.append([0] * (CAP - 32) + s)
    tok, lens = table([[[1, 1], s]] * T, 16, 32)
    c = dict(out=rows, n=[CAP] * T, ss_n=[CAP - 1] * T, seq_tok=tok, seq_len=lens, hit=[-1] * T, hold=[0] * T, active=[1] * T, done=[0] * T)
    got = launch(ops, c)
    assert got == want(c)
    assert got[1] == [-1] * 32 + [1] and got[4] == [0] * 32 + [16]
    assert got[2][:31] == [ref.scan(r, [s])[1] for r in rows[:31]] and max(got[2]) < 32
    # the same miss in the TABLE: one negative entry at each position matches nothing, not even a -1 that a broken token row could hold
    toks = []
    for j in range(32):
        x = list(s)
        x[j] = -1
        toks.append([x] + [[-1] * 32] * 15)
    c2 = dict(c, out=[rows[32]] * 32, n=[CAP] * 32, ss_n=[0] * 32, seq_tok=toks, seq_len=[[32] + [0] * 15] * 32, hit=[-1] * 32, hold=[0] * 32,
              active=[1] * 32, done=[0] * 32)
    got = launch(ops, c2)
    assert got == want(c2) and got[1] == [-1] * 32


def test_earlier_match_two_matches_and_the_tie_rule(ops):
    # a match that exists earlier in the turn but not at its end
    c = _one([5, 1, 2, 3, 5, 1], [[1, 2, 3]])
    assert launch(ops, c) == want(c) == ([6], [-1], [1], [1], [0])
    # two sequences match at once: the lowest index, whatever the lengths; hold is 0 although [3] also begins sequence 2
    c = _one([5, 1, 2, 3], [[9, 9], [3], [3, 4], [2, 3], [1, 2, 3]])
    assert launch(ops, c) == want(c) == ([4], [1], [0], [0], [16])
    c = _one([5, 1, 2, 3], [[9, 9], [5, 1, 2, 3], [3]])
    assert launch(ops, c) == want(c) == ([4], [1], [0], [0], [16])
    # the longest held prefix over all sequences; a self-overlapping sequence
    c = _one([4, 4, 4], [[4, 4, 4, 4, 9], [4, 4, 5], [4, 6]])
    assert launch(ops, c) == want(c) == ([3], [-1], [3], [1], [0])
    c = _one([4, 4, 4, 4], [[4, 4, 4]])
    assert launch(ops, c) == want(c) == ([4], [0], [0], [0], [16])


def test_unmoved_retired_and_total_rule(ops):
    full = [1, 2, 3]
    tok, lens = table([[full]] * 6, 4, 3)
    lens[3] = [4, -1, 7, 3]                                              # lengths outside 0 .. W count as 0; slot 3 is a real one
    tok[3] = [[1, 2, 3], [1, 2, 3], [1, 2, 3], [2, 2, 3]]
    tok[4] = [[1, -2, 3], [-1, -1, -1], [2, 3, -1], [-7, 2, 3]]          # negative entries match nothing
    lens[4] = [3, 1, 3, 3]
    c = dict(out=[[0, 1, 2, 3] + [0] * (CAP - 4)] * 4 + [[0, 1, -2, 3] + [0] * (CAP - 4), [2 ** 32 + 1, 2 ** 32 + 2, 2 ** 32 + 3] + [0] * (CAP - 3)],
             n=[4, 4, 4, 4, 4, 3],
             ss_n=[4, 3, 3, 3, 3, 2],
             seq_tok=tok, seq_len=lens,
             hit=[2, -1, -1, 0, 0, -1], hold=[1, 0, 0, 0, 0, 0], active=[1, 0, 0, 1, 1, 1], done=[0, 2, 1, 0, 0, 0])
    for as_bool in (True, False):
        got = launch(ops, c, strided=True, as_bool=as_bool)
        assert got == want(c, CAP)
        # 0: the count did not move -- every word unchanged, the stale hit and hold included, and the tenant stays active
        # 1: retired by max_new_tokens in this very step and matching: 2 | 16; 2: the same next to a stop token
        # 3: only garbage lengths and a sequence that does not match: nothing; 4: negative ids on both sides match nothing
        # 5: tokens that equal the ids only in their low 32 bits do not match
        assert got == ([4, 4, 4, 4, 4, 3], [2, 0, 0, -1, -1, -1], [1, 0, 0, 0, 0, 0], [1, 0, 0, 1, 1, 1], [0, 18, 17, 0, 0, 0])


def test_soak_of_200_tenant_steps_and_two_launches_agree(ops):
    """50 tenants over three symbols through four consecutive steps on the device's own state, against the restatement step by step; then the
    first of those launches again from the same inputs"""
    rng = random.Random(99)
    T, Q, W = 50, 4, 3
    c = random_case(T, Q, W, rng)
    c["n"] = [rng.randint(1, CAP - 4) for _ in range(T)]
    c["ss_n"] = [n - 1 for n in c["n"]]
    c["active"], c["done"], c["hit"], c["hold"] = [1] * T, [0] * T, [-1] * T, [0] * T
    first = dict(c)
    retired = 0
    for step in range(4):
        got, exp = launch(ops, c, strided=bool(step % 2)), want(c)
        assert got == exp, step
        ss_n, hit, hold, active, done = got
        # the next step: a still-active tenant emits one more token (its row already holds it), a retired one stands still
        c = dict(c, ss_n=ss_n, hit=hit, hold=hold, active=active, done=done, n=[n + a for n, a in zip(c["n"], active)])
        retired = T - sum(active)
    assert retired > 5                                                   # (tenants did hit their sequences along the way)
    assert launch(ops, first) == launch(ops, first) == want(first)


def test_inside_a_captured_graph_on_a_side_stream(ops):
    rng = random.Random(5)
    T, Q, W = 16, 16, 32
    c = random_case(T, Q, W, rng)
    exp = want(c)
    dev = lambda v, dt: torch.tensor(v, dtype=dt, device="cuda")
    out = Out(c["out"], True)
    init = dict(ss_n=dev(c["ss_n"], torch.long), hit=dev(c["hit"], torch.int32), hold=dev(c["hold"], torch.int32),
                active=dev(c["active"], torch.bool), done=dev(c["done"], torch.uint8))
    st = {k: v.clone() for k, v in init.items()}
    n, tok, lens = dev(c["n"], torch.long), dev(c["seq_tok"], torch.int32), dev(c["seq_len"], torch.int32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # (a warm-up launch on the capture stream, then the state put back)
        ops.step_stop_sequences(out.view, n, st["ss_n"], tok, lens, st["hit"], st["hold"], st["active"], st["done"])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = {k: v.cpu().clone() for k, v in st.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.step_stop_sequences(out.view, n, st["ss_n"], tok, lens, st["hit"], st["hold"], st["active"], st["done"])
    torch.cuda.synchronize()
    for _ in range(2):
        for k, v in init.items():
            st[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        for k in st:
            assert torch.equal(st[k].cpu(), eager[k]), k
    assert (st["ss_n"].tolist(), st["hit"].tolist(), st["hold"].tolist(), [int(v) for v in st["active"].tolist()], st["done"].tolist()) == exp
    assert out.intact()


def test_every_error_code_in_its_documented_order_with_nothing_launched(ops):
    from bitdelta_amd._lib import lib
    L = lib()
    T, Q, W = 2, 4, 8
    out = torch.full((T, CAP), 5, dtype=torch.long, device="cuda")
    n = torch.ones(T, dtype=torch.long, device="cuda")
    ss_n = torch.zeros(T, dtype=torch.long, device="cuda")
    tok = torch.full((T, Q, W), 5, dtype=torch.int32, device="cuda")
    lens = torch.ones(T, Q, dtype=torch.int32, device="cuda")
    hit, hold = torch.full((T,), -1, dtype=torch.int32, device="cuda"), torch.zeros(T, dtype=torch.int32, device="cuda")
    act, done = torch.ones(T, dtype=torch.uint8, device="cuda"), torch.zeros(T, dtype=torch.uint8, device="cuda")
    BAD_SHAPE, NULL = L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None), L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 0, None)
    good = dict(out=out.data_ptr(), s_out=CAP, out_cap=CAP, n=n.data_ptr(), ss_n=ss_n.data_ptr(), seq_tok=tok.data_ptr(), seq_len=lens.data_ptr(),
                Q=Q, W=W, hit=hit.data_ptr(), hold=hold.data_ptr(), active=act.data_ptr(), done=done.data_ptr(), T=T)
    order = ("out", "s_out", "out_cap", "n", "ss_n", "seq_tok", "seq_len", "Q", "W", "hit", "hold", "active", "done", "T")

    def call(**kw):
        a = dict(good, **kw)
        return L.bd_srv_step_stop_sequences(*[a[k] for k in order], None)
    # shape first (even with T == 0 or a null pointer) ...
    for kw in (dict(T=-1), dict(T=65536), dict(Q=0), dict(Q=17), dict(W=0), dict(W=33), dict(out_cap=-1), dict(s_out=CAP - 1)):
        assert call(**kw) == BAD_SHAPE and call(out=None, **kw) == BAD_SHAPE, kw
    assert call(T=0, Q=17) == BAD_SHAPE
    # ... then T == 0, then null pointers, then alignment
    assert call(T=0) == 0 and call(T=0, out=None, done=None) == 0
    for k in ("out", "n", "ss_n", "seq_tok", "seq_len", "hit", "hold", "active", "done"):
        assert call(**{k: None}) == NULL, k
    assert call(hit=None, out=good["out"] + 4) == NULL
    for k in ("out", "n", "ss_n"):
        assert call(**{k: good[k] + 4}) == BAD_SHAPE, k
    for k in ("seq_tok", "seq_len", "hit", "hold"):
        assert call(**{k: good[k] + 2}) == BAD_SHAPE, k
    torch.cuda.synchronize()
    assert ss_n.tolist() == [0, 0] and hit.tolist() == [-1, -1] and act.tolist() == [1, 1] and done.tolist() == [0, 0]      # nothing ran
    # the wrapper's own refusals
    with pytest.raises(AssertionError):
        ops.step_stop_sequences(out, n, ss_n, tok.long(), lens, hit, hold, act, done)
    with pytest.raises(AssertionError):
        ops.step_stop_sequences(out, n, ss_n, torch.zeros(T, 17, 2, dtype=torch.int32, device="cuda"), torch.zeros(T, 17, dtype=torch.int32, device="cuda"),
                                hit, hold, act, done)
    with pytest.raises(AssertionError):
        ops.step_stop_sequences(out.int(), n, ss_n, tok, lens, hit, hold, act, done)
    with pytest.raises(Exception):
        ops.step_stop_sequences(out.cpu(), n, ss_n, tok, lens, hit, hold, act, done)
    # and the good call does run: both tenants end with [5]
    assert call() == 0
    torch.cuda.synchronize()
    assert hit.tolist() == [0, 0] and done.tolist() == [16, 16] and act.tolist() == [0, 0] and ss_n.tolist() == [1, 1]
