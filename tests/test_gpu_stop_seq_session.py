"""GPU tests of stop sequences in a TenantSession (serving_loop.py, session(stop_sequences=True)) on a two-layer synthetic decoder, V = 512.
A FREE run comes first, greedy and sampled at fixed seeds; every expectation is derived from its tokens through the restatement of the
definition (tests/stop_seq_ref.py) -- never from where a sequence is assumed to occur first: a tiny model repeats itself.  A tenant stopped on a
slice of its own output yields the free output cut at the first hit, with reason 16, while the other tenants' tokens and reasons stay
bit-identical, whatever the stepping mode; streamable / hold after every step; admission; a sequence straddling the prompt; one capture for
changing sequences; extend and load_tenant; every other feature switched on next to it; and a session made without the feature has none of
it."""
import math

import pytest
import torch

import stop_seq_ref as ref

pytestmark = pytest.mark.gpu

V = 512
N = 24                       # tokens of a free turn
SAMPLING = [dict(temperature=1.0, top_k=0, top_p=1.0, seed=2 ** 63 + 17), dict(temperature=0.7, top_k=20, top_p=0.9, seed=11),
            dict(temperature=0.0, top_k=0, top_p=1.0, seed=0), dict(temperature=1.5, top_k=0, top_p=0.8, seed=2 ** 64 - 1)]
PEN = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25, logit_bias={5: 2.0, 17: -math.inf, 300: -1.5})
KINDS = ["greedy", "sampling"]


@pytest.fixture(scope="module")
def dec128():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib
    from bitdelta_amd.serving_loop import TenantDecoder
    _lib.lib()
    return TenantDecoder.synthetic("tiny128", 4, "cuda", dtype=torch.float16, seed=31, max_len=256)


def _toks(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, 500, (n,), generator=g).tolist()


PROMPTS = [_toks(n, 40 + n) for n in (9, 64, 33, 70)]


def _par(kind, t):
    return SAMPLING[t] if kind == "sampling" else {}


def _results(sess):
    return [(sess.result(t)[0].tolist(), sess.result(t)[1]) for t in range(sess.T)]


def _submit_each(sess, kind, seqs, max_new_tokens=N):
    """the free run's requests, tenant by tenant; seqs: {tenant: its stop sequences}"""
    for t in range(4):
        kw = dict(stop_sequences=seqs[t]) if t in seqs else {}
        sess.submit(t, PROMPTS[t], max_new_tokens=max_new_tokens, **_par(kind, t), **kw)


@pytest.fixture(scope="module")
def free(dec128):
    """{kind: [(tokens, reason)] * 4}: sessions made WITHOUT the feature, run once, never modified"""
    res = {}
    for kind in KINDS:
        sess = dec128.session(sampling=kind == "sampling")
        _submit_each(sess, kind, {})
        sess.run()
        res[kind] = _results(sess)
        assert all(len(y) == N and r == 2 for y, r in res[kind])
    return res


def _cut(y, seqs, limit=None):
    """what a session gives for a turn whose free tokens are y under the stop sequences seqs: (tokens, reason, stop_match)"""
    m, h = ref.first_hit(y, seqs)
    limit = len(y) if limit is None else limit
    if h < 0:
        return y[:limit], 2, None
    return y[:m], 16 | (2 if m == limit else 0), (h, len(seqs[h]))


def _run(sess, mode):
    if mode == "graph":
        sess.run()
    elif mode == "every4":
        sess.run(check_every=4)
    else:
        sess.run(use_graph=False)


# ------------------------------------------------------------------------------------------------ 1. a hit on one tenant, every stepping mode
@pytest.mark.parametrize("mode", ["graph", "every4", "eager"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_tenant_stops_at_its_sequence_and_nobody_else_notices(dec128, free, kind, mode):
    y = free[kind][1][0]
    seq = y[5:8]
    want, reason, match = _cut(y, [[400, 401], seq])                     # (sequence 0 is never emitted whole here, or the restatement says so)
    assert match is not None and len(want) <= 8
    sess = dec128.session(sampling=kind == "sampling", stop_sequences=True)
    _submit_each(sess, kind, {1: [[400, 401], seq]})
    _run(sess, mode)
    got = _results(sess)
    assert got[1] == (want, reason) and reason & 16
    assert sess.stop_match(1) == match and sess.streamable(1) == len(want)
    assert want[len(want) - match[1]:] == [[400, 401], seq][match[0]]    # the matched tokens are in the result, as a stop token is
    for t in (0, 2, 3):
        assert got[t] == free[kind][t], t                               # bit-identical to the free run
        assert sess.stop_match(t) is None and sess.streamable(t) == N
    assert sess.hit.tolist()[1] == match[0] and sess.hold.tolist() == [0] * 4 and sess.ss_n.tolist() == [N, len(want), N, N]
    assert not any(sess.active())


# ------------------------------------------------------------------------------------------------ 2. what a streaming caller sees
def test_streamable_rises_and_falls_back_step_by_step(dec128, free):
    """a sequence whose first two tokens occur in the output and are then not completed: hold goes to 2 and back"""
    pick = None
    for kind in KINDS:
        for t in range(4):
            y = free[kind][t][0]
            x = next(v for v in range(1, V) if v not in y)               # the third token: never emitted, so nothing ever hits
            for i in range(len(y) - 2):
                holds = [ref.scan(y[:m], [[y[i], y[i + 1], x]])[1] for m in range(1, len(y) + 1)]
                if 2 in holds and min(holds[holds.index(2):]) < 2 and pick is None:
                    pick = (kind, t, [[y[i], y[i + 1], x]], holds)
    assert pick is not None, "no free run holds two different neighbouring tokens"
    kind, t, seqs, holds = pick
    y = free[kind][t][0]
    sess = dec128.session(sampling=kind == "sampling", stop_sequences=True)
    sess.submit(t, PROMPTS[t], max_new_tokens=N, stop_sequences=seqs, **_par(kind, t))
    seen = []
    for m in range(1, N + 1):
        assert int(sess.n[t]) == m and int(sess.hold[t]) == holds[m - 1] and sess.streamable(t) == m - holds[m - 1], m
        assert sess.stop_match(t) is None
        seen.append(sess.streamable(t))
        if m < N:
            assert sess.active()[t]
            sess.step(1)
    assert _results(sess)[t] == (y, 2)
    assert max(holds) == 2 and any(b == a for a, b in zip(seen, seen[1:])) and any(b > a + 1 for a, b in zip(seen, seen[1:]))      # it stalls, then catches up
    assert all(0 <= s_ <= m for m, s_ in enumerate(seen, 1))


# ------------------------------------------------------------------------------------------------ 3. admission and the prompt
def test_the_first_token_is_matched_at_admission(dec128, free):
    y = free["greedy"][0][0]
    sess = dec128.session(stop_sequences=True)
    sess.submit(0, PROMPTS[0], max_new_tokens=N, stop_sequences=[[y[0] + 1 if y[0] + 1 < V else 0], [y[0]]])
    assert not sess.active()[0] and _results(sess)[0] == ([y[0]], 16)
    assert sess.stop_match(0) == (1, 1) and sess.streamable(0) == 1 and sess.ss_n.tolist()[0] == 1
    sess.submit(0, PROMPTS[0], max_new_tokens=1, stop_sequences=[[y[0]]])                 # next to max_new_tokens: both reasons
    assert _results(sess)[0] == ([y[0]], 18)
    x = next(v for v in range(1, V) if v not in y)
    sess.submit(0, PROMPTS[0], max_new_tokens=N, stop_sequences=[[y[0], x]])             # its first token only: held back from the start
    assert sess.active()[0] and sess.stop_match(0) is None and int(sess.hold[0]) == 1 and sess.streamable(0) == 0
    sess.run()
    assert _results(sess)[0] == (y, 2) and sess.stop_match(0) is None


def test_a_sequence_straddling_prompt_and_output_does_not_match(dec128, free):
    y = free["greedy"][0][0]
    for seqs in ([[PROMPTS[0][-1], y[0]]], [[PROMPTS[0][-2], PROMPTS[0][-1], y[0]]]):
        want, reason, match = _cut(y, seqs)                              # on the TURN's tokens alone
        on_all = ref.first_hit(PROMPTS[0] + y, seqs)[0] - len(PROMPTS[0])
        assert on_all == 1                                               # with the prompt in front the first token WOULD complete it
        sess = dec128.session(stop_sequences=True)
        sess.submit(0, PROMPTS[0], max_new_tokens=N, stop_sequences=seqs)
        sess.run()
        assert _results(sess)[0] == (want, reason) and sess.stop_match(0) == match and len(want) > on_all


# ------------------------------------------------------------------------------------------------ 4. one capture
def test_sequences_change_between_requests_on_one_capture(dec128, free):
    y = free["greedy"][2][0]
    sess = dec128.session(stop_sequences=True)
    per_request = [[y[3:5]], [y[10:13], y[6:7]], (), [[1, 2, 3, 4, 5, 6, 7, 8]] * 4, [y[0:2]], None, [y[N - 1:N]]]
    for seqs in per_request:
        sess.submit(2, PROMPTS[2], max_new_tokens=N, **({} if seqs is None else dict(stop_sequences=seqs)))
        sess.run()
        want, reason, match = _cut(y, list(seqs or []))
        assert _results(sess)[2] == (want, reason) and sess.stop_match(2) == match, seqs
        assert len(sess._graphs) <= 1
    assert len(sess._graphs) == 1
    (key,) = sess._graphs
    assert key[-3:] == (True, 4, 8)
    # the refusals come before anything is touched
    before = [x.clone() for x in (sess.ss_tok, sess.ss_len, sess.ss_n, sess.hit, sess.hold, sess.n, sess.done, sess.out)] + \
             [c.clone() for c in sess.cache["k"] + sess.cache["v"]]
    for bad in ([[]], [[V]], [[1.5]], [[1]] * 5, [[1] * 9], [[True]]):
        with pytest.raises(ValueError):
            sess.submit(2, PROMPTS[2], stop_sequences=bad)
        with pytest.raises(ValueError):
            sess.extend(2, [5], stop_sequences=bad)
        with pytest.raises(ValueError):
            sess.submit_all(PROMPTS, stop_sequences=[[], [], bad, []])
    after = [sess.ss_tok, sess.ss_len, sess.ss_n, sess.hit, sess.hold, sess.n, sess.done, sess.out] + sess.cache["k"] + sess.cache["v"]
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and not any(sess.active())
    # other sizes are another session and another graph key
    big = dec128.session(stop_sequences=True, max_stop_sequences=16, max_stop_sequence_len=32)
    assert big.ss_tok.shape == (4, 16, 32) and big.ss_len.shape == (4, 16)
    big.submit(2, PROMPTS[2], max_new_tokens=N, stop_sequences=[[9] * 32] * 15 + [y[4:6]])
    big.run()
    want, reason, match = _cut(y, [[9] * 32] * 15 + [y[4:6]])
    assert _results(big)[2] == (want, reason) and big.stop_match(2) == match and match[0] == 15
    assert next(iter(big._graphs))[-3:] == (True, 16, 32)


def test_submit_all_takes_one_list_for_all_or_one_per_tenant(dec128):
    plain = dec128.session()
    plain.submit_all(PROMPTS, max_new_tokens=N)
    plain.run()
    y = [r[0] for r in _results(plain)]
    sess = dec128.session(stop_sequences=True)
    per = [[y[0][4:6]], [], [y[2][2:3], y[2][7:9]], []]
    sess.submit_all(PROMPTS, max_new_tokens=N, stop_sequences=per)
    sess.run()
    for t in range(4):
        want, reason, match = _cut(y[t], per[t])
        assert _results(sess)[t] == (want, reason) and sess.stop_match(t) == match, t
    one = [y[1][5:7], y[3][5:7]]                                         # ONE list of two sequences: every tenant gets both
    sess.submit_all(PROMPTS, max_new_tokens=N, stop_sequences=one)
    sess.run()
    for t in range(4):
        want, reason, match = _cut(y[t], one)
        assert _results(sess)[t] == (want, reason) and sess.stop_match(t) == match, t
    assert sess.stop_match(1) is not None and sess.stop_match(3) is not None and len(sess._graphs) == 1


# ------------------------------------------------------------------------------------------------ 5. extend and load_tenant
def test_extend_after_a_match_and_load_tenant(dec128, free):
    import bitdelta_amd as bd
    from test_gpu_session_extend import _truth
    dec, t = dec128, 1
    y = free["greedy"][t][0]
    seq = y[3:6]
    turn1, reason, match = _cut(y, [seq])
    assert reason == 16
    more = _toks(7, 77)
    # the twin: a session without the feature whose turn ends at the same token by max_new_tokens, extended by the same tokens, free
    twin = dec.session()
    twin.submit(t, PROMPTS[t], max_new_tokens=len(turn1))
    twin.run()
    assert _results(twin)[t] == (turn1, 2)
    twin.extend(t, more, max_new_tokens=12)
    twin.run()
    y2 = _results(twin)[t][0]
    assert len(y2) == 12
    sess = dec.session(stop_sequences=True)
    sess.submit(t, PROMPTS[t], max_new_tokens=N, stop_sequences=[seq])
    sess.submit(2, PROMPTS[2], max_new_tokens=N, stop_sequences=[[3, 4]])
    sess.run()
    assert _results(sess)[t] == (turn1, 16) and int(sess.pos[t]) == int(twin.pos[t]) - len(more) - 12
    other = (sess.ss_tok[2].clone(), sess.ss_len[2].clone(), int(sess.hit[2]), int(sess.ss_n[2]))
    # the new turn's sequences: one that straddles the two turns (no match), the old turn's (no match unless the new turn spells it), a real one
    seqs2 = [[turn1[-1], y2[0]], seq, y2[4:6]]
    want2, reason2, match2 = _cut(y2, seqs2)
    assert ref.scan(turn1 + y2[:1], seqs2)[0] == 0                       # over both turns the first one WOULD match at once
    sess.extend(t, more, max_new_tokens=12, stop_sequences=seqs2)
    assert int(sess.ss_n[t]) == 1 and sess.ss_len[t].tolist() == [2, 3, 2, 0]
    sess.run()
    assert _results(sess)[t] == (want2, reason2) and sess.stop_match(t) == match2 and match2 is not None and len(want2) > 1
    _truth(bd, dec, t, 64 - len(PROMPTS[t]), PROMPTS[t] + turn1 + more, torch.tensor(want2))      # the existing extend tests' rule
    sess.extend(t, [], max_new_tokens=3)                                 # no sequences: the turn before's are gone
    sess.run()
    assert _results(sess)[t][1] == 2 and sess.ss_len[t].tolist() == [0] * 4 and sess.stop_match(t) is None
    assert torch.equal(sess.ss_tok[2], other[0]) and torch.equal(sess.ss_len[2], other[1]) and (int(sess.hit[2]), int(sess.ss_n[2])) == other[2:]
    # load_tenant clears the slot
    sess.submit(t, PROMPTS[t], max_new_tokens=N, stop_sequences=[seq])
    sess.run()
    assert sess.stop_match(t) == match
    sess.load_tenant(t, {k: v for k, v in dec.tenant_state(t).items()})
    assert sess.stop_match(t) is None and (int(sess.hit[t]), int(sess.hold[t]), int(sess.ss_n[t])) == (-1, 0, 0)
    assert sess.ss_len[t].tolist() == [0] * 4 and bool((sess.ss_tok[t] == -1).all()) and sess.streamable(t) == 0
    assert torch.equal(sess.ss_tok[2], other[0]) and int(sess.hit[2]) == other[2]
    sess.submit(t, PROMPTS[t], max_new_tokens=N, stop_sequences=[seq])   # the same fine-tune, the same request: the first turn again
    sess.run()
    assert _results(sess)[t] == (turn1, 16)


# ------------------------------------------------------------------------------------------------ 6. next to every other feature
def test_with_every_other_feature_switched_on(dec128):
    from bitdelta_amd.constraint import TokenAutomaton as TA
    dec = dec128
    allowed = TA.allowed_set(range(64, 192, 3))
    kw = dict(sampling=True, logprobs=5, penalties=True, constraints=True)
    par = lambda t: dict(PEN, **SAMPLING[t])
    plain = dec.session(**kw)
    for t in (0, 1):
        plain.submit(t, PROMPTS[t], max_new_tokens=16, constraint=allowed, **par(t))
    plain.run()
    base = _results(plain)
    y = base[1][0]
    assert len(y) == 16 and set(y) <= set(range(64, 192, 3))
    seq = y[6:8]
    want, reason, match = _cut(y, [seq])
    assert reason == 16
    sess = dec.session(stop_sequences=True, **kw)
    sess.submit(0, PROMPTS[0], max_new_tokens=16, constraint=allowed, **par(0))
    sess.submit(1, PROMPTS[1], max_new_tokens=16, constraint=allowed, stop_sequences=[seq], **par(1))
    sess.run()
    assert _results(sess)[1] == (want, 16) and _results(sess)[0] == base[0] and sess.stop_match(1) == match
    lp, ids, lps = sess.result_logprobs(1)
    assert lp.shape == (len(want),) and ids.shape == (len(want), 5) and lps.shape == (len(want), 5)
    p_lp, p_ids, _ = plain.result_logprobs(1)
    assert torch.equal(lp.view(torch.int32), p_lp[:len(want)].view(torch.int32)) and torch.equal(ids, p_ids[:len(want)])
    # the last token of a forced choice is also the last of a stop sequence: the constraint's reason 8 and 16 together
    sess.submit(1, PROMPTS[1], max_new_tokens=16, constraint=TA.from_choices([[70, 71, 72]]), stop_sequences=[[71, 72]], **par(1))
    sess.run()
    assert _results(sess)[1] == ([70, 71, 72], 24) and sess.stop_match(1) == (0, 2) and sess.result_logprobs(1)[0].shape == (3,)
    # the automaton does not learn the sequence: a stop sequence it never lets through never matches
    sess.submit(1, PROMPTS[1], max_new_tokens=6, constraint=allowed, stop_sequences=[[65]], **par(1))
    sess.run()
    assert _results(sess)[1][1] == 2 and sess.stop_match(1) is None and len(sess._graphs) == 1


# ------------------------------------------------------------------------------------------------ 7. a session made without the feature
def test_a_session_without_the_feature_has_none_of_it(dec128, free, monkeypatch):
    from bitdelta_amd import serving_ops as ops
    dec = dec128
    calls = []
    for name in [n for n in dir(ops) if n.startswith("step_")]:
        def wrap(fn, name):
            def f(*a, **k):
                calls.append(name)
                return fn(*a, **k)
            return f
        monkeypatch.setattr(ops, name, wrap(getattr(ops, name), name))
    for kind in KINDS:
        plain = dec.session(sampling=kind == "sampling")
        assert plain.stop_sequences is False
        assert not any(hasattr(plain, n) for n in ("ss_tok", "ss_len", "ss_n", "hit", "hold"))
        with pytest.raises(ValueError, match="stop_sequences=True"):
            plain.submit(0, PROMPTS[0], stop_sequences=[[5]])
        with pytest.raises(ValueError, match="stop_sequences=True"):
            plain.submit_all(PROMPTS, stop_sequences=[[5]])
        with pytest.raises(ValueError, match="stop_sequences=True"):
            plain.submit_all(PROMPTS, stop_sequences=[[], [[5]], [], []])
        for fn in (plain.stop_match, plain.streamable):
            with pytest.raises(ValueError, match="stop_sequences=True"):
                fn(0)
        assert not any(plain.active())
        del calls[:]
        _submit_each(plain, kind, {0: (), 1: []})                        # an empty value is no request for the feature
        plain.step(1, use_graph=False)
        before = list(calls)
        assert "step_stop_sequences" not in before
        plain.run()
        assert _results(plain) == free[kind]
        (key,) = plain._graphs
        assert len(key) == 10                                            # the key it had
        with_flag = dec.session(sampling=kind == "sampling", stop_sequences=True)
        del calls[:]
        _submit_each(with_flag, kind, {})
        with_flag.step(1, use_graph=False)
        assert calls == before + ["step_stop_sequences"]                 # the same launches in the same order, and one more at the very end
        with_flag.run()
        assert _results(with_flag) == free[kind]                         # no sequences: the free run bit for bit
    with pytest.raises(ValueError):
        dec.session(stop_sequences=True, max_stop_sequences=17)
    with pytest.raises(ValueError):
        dec.session(stop_sequences=True, max_stop_sequence_len=33)
