"""GPU tests of the token-automaton constraint in a TenantSession (serving_loop.py, session(constraints=True)) on two-layer synthetic decoders,
V = 512: at every step the row the step end chose from is the restatement's mask (tests/constraint_ref.py) of the row the step was given, for
the state before the step, the emitted token lies in the allowed set and the state afterwards is the restatement's; a request under a trie of
choices emits exactly one of them and retires with reason 8 in the step that completes it; a prefix choice ends by the stop id (reason 1) or
goes on (reason 8); the other tenants, graph replay, and changing the automaton between requests change nothing else; extend, load_tenant, the
raw log-probabilities, the other retirement reasons; and a session made without constraints=True has none of it."""
import math

import pytest
import torch

import constraint_ref as ref

pytestmark = pytest.mark.gpu

V = 512
SAMPLING = [dict(temperature=1.0, top_k=0, top_p=1.0, seed=2 ** 63 + 17), dict(temperature=0.7, top_k=20, top_p=0.9, seed=11),
            dict(temperature=0.0, top_k=0, top_p=1.0, seed=0), dict(temperature=1.5, top_k=0, top_p=0.8, seed=2 ** 64 - 1)]
PEN = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25, logit_bias={5: 2.0, 17: -math.inf, 300: -1.5})
CHOICES = [[11], [20, 21], [20, 22, 23], [30, 31, 32, 33], [40, 41]]     # lengths 1 to 4, none a prefix of another


@pytest.fixture(scope="module")
def dec128():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib
    from bitdelta_amd.serving_loop import TenantDecoder
    _lib.lib()
    return TenantDecoder.synthetic("tiny128", 4, "cuda", dtype=torch.float16, seed=31, max_len=256)


@pytest.fixture(scope="module")
def TA():
    from bitdelta_amd.constraint import TokenAutomaton
    return TokenAutomaton


def _toks(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, 500, (n,), generator=g).tolist()


PROMPTS = [_toks(n, 40 + n) for n in (9, 64, 33, 70)]


def _results(sess):
    return [(sess.result(t)[0].tolist(), sess.result(t)[1]) for t in range(sess.T)]


class Recorder:
    """serving_ops.constrain_rows / step_constrain / step_constrain_advance wrapped to keep what they were given and what they wrote"""

    def __init__(self, monkeypatch):
        from bitdelta_amd import serving_ops as ops
        self.first, self.steps, self.advances = [], [], []
        o_rows, o_step, o_adv = ops.constrain_rows, ops.step_constrain, ops.step_constrain_advance
        cp = lambda x: x.detach().cpu().clone()

        def rows(logits, state, off, edge_tok, accepting, stop_ids=None, out=None):
            res = o_rows(logits, state, off, edge_tok, accepting, stop_ids, out)
            self.first.append(dict(logits=cp(logits), state=cp(state), off=cp(off), tok=cp(edge_tok), acc=cp(accepting), stops=cp(stop_ids),
                                   out=cp(res)))
            return res

        def step(logits, out, state, off, edge_tok, accepting, stop_ids, active):
            if torch.cuda.is_current_stream_capturing():             # (a capture takes no copies to the host; replays do not come through here)
                return o_step(logits, out, state, off, edge_tok, accepting, stop_ids, active)
            rec = dict(logits=cp(logits), ptr=logits.data_ptr(), state=cp(state), off=cp(off), tok=cp(edge_tok), acc=cp(accepting),
                       stops=cp(stop_ids), active=cp(active), prev=cp(out))
            res = o_step(logits, out, state, off, edge_tok, accepting, stop_ids, active)
            rec.update(out=cp(res))
            self.steps.append(rec)
            return res

        def adv(tok, n, c_n, state, off, edge_tok, edge_next, accepting, active, done):
            if torch.cuda.is_current_stream_capturing():
                return o_adv(tok, n, c_n, state, off, edge_tok, edge_next, accepting, active, done)
            rec = dict(tok=cp(tok), n=cp(n), c_n=cp(c_n), state=cp(state), off=cp(off), etok=cp(edge_tok), nxt=cp(edge_next), acc=cp(accepting),
                       active=cp(active), done=cp(done))
            o_adv(tok, n, c_n, state, off, edge_tok, edge_next, accepting, active, done)
            rec.update(after=(c_n.tolist(), state.tolist(), [int(v) for v in active.tolist()], done.tolist()))
            self.advances.append(rec)
        monkeypatch.setattr(ops, "constrain_rows", rows)
        monkeypatch.setattr(ops, "step_constrain", step)
        monkeypatch.setattr(ops, "step_constrain_advance", adv)


def _allowed(rec, t):
    return ref.allowed(int(rec["state"][t]), rec["off"][t].tolist(), rec["tok"][t].tolist(), rec["acc"][t].tolist(), rec["stops"][t].tolist(), V)


# ------------------------------------------------------------------------------------------------ 1. every step against the restatement
@pytest.mark.parametrize("sampling", [False, True], ids=["greedy", "sampling"])
def test_every_step_agrees_with_the_restatement(dec128, TA, monkeypatch, sampling):
    """eager steps of a session with penalties AND constraints, the three constraint launches wrapped"""
    dec = dec128
    rec = Recorder(monkeypatch)
    sess = dec.session(sampling=sampling, penalties=True, constraints=True)
    par = (lambda t: dict(PEN, **SAMPLING[t])) if sampling else (lambda t: PEN)
    g = torch.Generator().manual_seed(3)
    ring = [(s, y, (s + 1 + y % 2) % 5) for s in range(5) for y in sorted(set(torch.randint(0, V, (30,), generator=g).tolist()))]
    cons = [TA.from_choices([[100, 101, 102, 103, 104, 105], [100, 17, 5], [7, 8, 9, 10, 11, 12, 13]]),
            TA.allowed_set(range(64, 192, 3)), None, TA.from_edges(5, ring, [0, 1, 0, 0, 1])]
    stops = [[], [70, 300], [], [499]]
    emitted = {t: [] for t in range(4)}
    host_state = {}

    def admitted(t):
        r = rec.first[-1]
        a = cons[t]
        assert r["logits"].shape == (1, V) and r["state"].tolist() == [0 if a is not None else -1]
        assert ref.same_bits(r["out"], ref.mask(r["logits"], r["state"], r["off"], r["tok"], r["acc"], r["stops"]))
        first = int(sess.tok[t, 0])
        emitted[t] = [first]
        if a is not None:
            assert _allowed(r, 0) == set(a.allowed(0, stops[t])) and first in _allowed(r, 0)
            host_state[t] = a.step(0, first)
        else:
            host_state[t] = -1
        assert int(sess.c_state[t]) == host_state[t] and int(sess.c_n[t]) == 1

    def run(k):
        for _ in range(k):
            act = sess.active()
            if not any(act):
                break
            sess.step(1, use_graph=False)
            r, a = rec.steps[-1], rec.advances[-1]
            assert r["ptr"] == sess.plogits.data_ptr() and r["active"].tolist() == act      # it reads the penalised row
            assert r["state"].tolist() == [host_state.get(t, -1) for t in range(4)]
            out = ref.mask(r["logits"], r["state"], r["off"], r["tok"], r["acc"], r["stops"], active=r["active"], out=r["prev"])
            assert ref.same_bits(out, r["out"]) and ref.same_bits(r["out"], sess.clogits.cpu())
            want = ref.advance(a["tok"], a["n"], a["c_n"], a["state"], a["off"], a["etok"], a["nxt"], a["acc"], a["active"], a["done"])
            assert a["after"] == want
            for t in range(4):
                if not act[t]:
                    continue
                y = int(sess.tok[t, 0])
                emitted[t].append(y)
                al = _allowed(r, t)
                if al is None:
                    assert ref.same_bits(r["out"][t], r["logits"][t])
                else:
                    inside = torch.zeros(V, dtype=torch.bool)
                    inside[torch.tensor(sorted(al))] = True
                    assert y in al and ref.same_bits(r["out"][t][inside], r["logits"][t][inside])          # the penalised row's bits inside the set
                    assert bool((r["out"][t][~inside].view(torch.int16) == ref.NEG_INF_BITS[torch.float16]).all())          # -inf exactly outside it
                    host_state[t] = cons[t].step(host_state[t], y)
                assert int(sess.c_state[t]) == host_state[t] == want[1][t]
    sess.submit(0, PROMPTS[0], max_new_tokens=12, stop_token_ids=stops[0], constraint=cons[0], **par(0)); admitted(0)
    run(2)
    sess.submit(1, PROMPTS[1], max_new_tokens=6, stop_token_ids=stops[1], constraint=cons[1], **par(1)); admitted(1)
    sess.submit(2, PROMPTS[2], max_new_tokens=5, **par(2)); admitted(2)
    run(2)
    sess.submit(3, PROMPTS[3], max_new_tokens=9, stop_token_ids=stops[3], constraint=cons[3], **par(3)); admitted(3)
    run(40)
    assert not any(sess.active()) and [sess.result(t)[0].tolist() for t in range(4)] == [emitted[t] for t in range(4)]
    assert emitted[0] in ([100, 101, 102, 103, 104, 105], [100, 17, 5], [7, 8, 9, 10, 11, 12, 13]) and sess.result(0)[1] == 8
    assert emitted[0] != [100, 17, 5]                                    # (17 is banned by the request's bias: the mask reads the penalised row)
    assert set(emitted[1]) <= set(range(64, 192, 3)) | {70, 300} and sess.result(1)[1] in (1, 2)
    assert len(emitted[2]) == 5 and sess.result(2)[1] == 2 and len(rec.steps) <= 16


# ------------------------------------------------------------------------------------------------ 2. a trie of choices
def test_a_request_under_choices_emits_exactly_one_of_them(dec128, TA):
    dec = dec128
    a = TA.from_choices(CHOICES)
    greedy, samp = dec.session(constraints=True), dec.session(sampling=True, constraints=True)
    greedy.submit_all(PROMPTS, max_new_tokens=16, constraint=a)
    if any(greedy.active()):
        greedy.run()
    got = []
    for t in range(4):
        toks, reason = greedy.result(t)
        assert toks.tolist() in CHOICES and reason == 8 and int(greedy.n[t]) == toks.numel(), t
        got.append(toks.tolist())
    steps = 0
    for rnd in range(2):                                                 # 8 seeds at temperature 1.5
        for t in range(4):
            samp.submit(t, PROMPTS[t], max_new_tokens=16, temperature=1.5, seed=1000 + 4 * rnd + t, constraint=a)
        while any(samp.active()):
            samp.step(1)
            steps += 1
        for t in range(4):
            toks, reason = samp.result(t)
            assert toks.tolist() in CHOICES and reason == 8 and int(samp.n[t]) == toks.numel(), (rnd, t)
            got.append(toks.tolist())
    assert steps <= 2 * 3                                                # the longest choice: 1 token at admission + 3 steps, no extra step
    assert len(greedy._graphs) <= 1 and len(samp._graphs) == 1
    # every choice a single token: the first token completes it, the tenant retires at admission and no step runs for it
    single = TA.from_choices([[7], [9], [100]])
    greedy.submit(2, PROMPTS[2], max_new_tokens=16, constraint=single)
    assert not any(greedy.active())
    toks, reason = greedy.result(2)
    assert toks.tolist() in ([7], [9], [100]) and reason == 8 and int(greedy.c_state[2]) in (1, 2, 3)
    greedy.submit(2, PROMPTS[2], max_new_tokens=1, stop_token_ids=[9, 7, 100], constraint=single)       # ... alongside the existing bits
    assert greedy.result(2)[1] == 8 | 2 | 1 and greedy.result(2)[0].tolist() == toks.tolist()


def test_a_prefix_choice_ends_by_the_stop_id_or_goes_on(dec128, TA):
    dec = dec128
    a = TA.from_choices([[5], [5, 6]])
    sess = dec.session(penalties=True, constraints=True)
    sess.submit(0, PROMPTS[0], max_new_tokens=16, stop_token_ids=[2], constraint=a, logit_bias={2: 100.0})      # the model "picks" the stop id
    assert sess.active()[0] and int(sess.c_state[0]) == 1               # after [5]: accepting, not final
    sess.run()
    assert sess.result(0)[0].tolist() == [5, 2] and sess.result(0)[1] == 1
    sess.submit(0, PROMPTS[0], max_new_tokens=16, stop_token_ids=[2], constraint=a, logit_bias={6: 100.0})
    sess.run()
    assert sess.result(0)[0].tolist() == [5, 6] and sess.result(0)[1] == 8
    # without a stop id the shorter choice cannot end on its own: 6 is all state 1 allows
    sess.submit(0, PROMPTS[0], max_new_tokens=16, constraint=a, logit_bias={6: -50.0})
    sess.run()
    assert sess.result(0)[0].tolist() == [5, 6] and sess.result(0)[1] == 8


# ------------------------------------------------------------------------------------------------ 3. isolation, graph / eager, one capture
@pytest.mark.parametrize("sampling", [False, True], ids=["greedy", "sampling"])
def test_other_tenants_and_neutral_use_are_the_plain_session(dec128, TA, sampling):
    dec = dec128
    par = {q: [P[q] for P in SAMPLING] for q in SAMPLING[0]} if sampling else {}
    plain, cons = dec.session(sampling=sampling), dec.session(sampling=sampling, constraints=True)
    stops = [[], [3], [], [5]]
    plain.submit_all(PROMPTS, max_new_tokens=10, stop_token_ids=stops, **par)
    plain.run()
    want = _results(plain)
    cons.submit_all(PROMPTS, max_new_tokens=10, stop_token_ids=stops, constraint=None, **par)       # neutral use everywhere
    cons.run()
    assert _results(cons) == want and cons.c_state.tolist() == [-1] * 4
    cons.submit_all(PROMPTS, max_new_tokens=10, stop_token_ids=stops, constraint=[TA.allowed_set(range(200, 260)), None, TA.from_choices(CHOICES), None], **par)
    cons.run()
    got = _results(cons)
    assert got[1] == want[1] and got[3] == want[3]                       # bit for bit the unconstrained tokens
    assert set(got[0][0]) <= set(range(200, 260)) and len(got[0][0]) == 10 and got[2][0] in CHOICES and got[2][1] == 8
    assert got[0] != want[0] and len(cons._graphs) == 1 and cons.clogits.dtype == torch.float16
    one = lambda t: {q: par[q][t] for q in par}
    plain.submit(3, PROMPTS[3], max_new_tokens=10, stop_token_ids=stops[3], **one(3))      # one tenant at a time, another order
    plain.step(2)
    plain.submit(2, PROMPTS[2], max_new_tokens=10, **one(2))
    plain.run()
    want3 = _results(plain)[3]
    for use_graph in (False, True):                                      # ... eager and replayed, the neighbour constrained
        cons.submit(3, PROMPTS[3], max_new_tokens=10, stop_token_ids=stops[3], **one(3))
        cons.step(2, use_graph=use_graph)
        cons.submit(2, PROMPTS[2], max_new_tokens=10, constraint=TA.from_choices(CHOICES), **one(2))
        cons.run(use_graph=use_graph)
        assert _results(cons)[3] == want3 and _results(cons)[2][0] in CHOICES and _results(cons)[2][1] == 8, use_graph


@pytest.mark.parametrize("sampling", [False, True], ids=["greedy", "sampling"])
def test_graph_replay_equals_eager(dec128, TA, sampling):
    dec = dec128
    sess = dec.session(sampling=sampling, constraints=True)
    g = torch.Generator().manual_seed(9)
    ring = [(s, y, (s + 1 + y % 3) % 6) for s in range(6) for y in sorted(set(torch.randint(0, V, (40,), generator=g).tolist()))]
    cons = [TA.from_edges(6, ring, [1, 0, 0, 1, 0, 0]), TA.allowed_set(range(0, 512, 5)), TA.from_choices(CHOICES), None]
    runs = []
    for use_graph in (False, True, True):
        for t in range(4):
            sess.submit(t, PROMPTS[t], max_new_tokens=12, stop_token_ids=[499], constraint=cons[t], **(SAMPLING[t] if sampling else {}))
        sess.run(use_graph=use_graph)
        runs.append((_results(sess), sess.c_state.tolist(), sess.c_n.tolist()))
    assert runs[0] == runs[1] == runs[2] and len(sess._graphs) == 1
    assert runs[0][1][3] == -1 and runs[0][0][2][1] == 8 and runs[0][0][2][0] in CHOICES
    for t in (0, 1):                                                     # (the walk through the ring is the automaton's: replayed on the host)
        s = 0
        for y in runs[0][0][t][0]:
            if not (runs[0][0][t][1] & 1 and y == 499):
                assert y in cons[t].allowed(s), (t, s, y)
            s = cons[t].step(s, y)
        assert s == runs[0][1][t]


def test_constraints_change_between_requests_on_one_capture(dec128, TA):
    dec = dec128
    sess, plain = dec.session(constraints=True), dec.session()
    plain.submit(1, PROMPTS[1], max_new_tokens=8)
    plain.run()
    base = plain.result(1)[0].tolist()
    seen = []
    for a in (TA.allowed_set([3, 4, 5]), TA.from_choices([[9, 8, 7, 6, 5, 4]]), TA.from_edges(2, [(0, 1, 1), (1, 2, 0)], [0, 1]), None):
        sess.submit(1, PROMPTS[1], max_new_tokens=8, constraint=a)
        sess.run()
        seen.append((sess.result(1)[0].tolist(), sess.result(1)[1]))
        assert len(sess._graphs) == 1
    assert set(seen[0][0]) <= {3, 4, 5} and seen[0][1] == 2 and seen[1] == ([9, 8, 7, 6, 5, 4], 8) and seen[2] == ([1, 2] * 4, 2)
    assert seen[3] == (base, 2) and int(sess.c_state[1]) == -1          # back to none: the plain tokens again
    # refusals at admission, before anything is touched
    before = [x.clone() for x in (sess.c_state, sess.c_n, sess.c_off, sess.c_tok, sess.c_next, sess.c_acc, sess.n, sess.stop_ids, sess.done)]
    small = dec.session(constraints=True, max_constraint_states=4, max_constraint_edges=6)
    assert small.c_off.shape == (4, 5) and small.c_tok.shape == small.c_next.shape == (4, 6) and small.c_acc.shape == (4, 4)
    for s_, bad, kw in ((sess, TA.allowed_set([V]), {}), (sess, TA.from_edges(1, [], [1]), {}), (small, TA.from_choices(CHOICES), {}),
                        (small, TA.allowed_set(range(7)), {}), (sess, [[1, 2]], {}), (sess, TA.allowed_set([1]), dict(stop_token_ids=range(9)))):
        with pytest.raises(ValueError):
            s_.submit(0, PROMPTS[0], constraint=bad, **kw)
        with pytest.raises(ValueError):
            s_.submit_all(PROMPTS, constraint=[None, None, bad, None], **({"stop_token_ids": [list(kw["stop_token_ids"])] * 4} if kw else {}))
    with pytest.raises(ValueError):
        sess.extend(1, [4, 5], constraint=TA.allowed_set([V + 3]))
    after = (sess.c_state, sess.c_n, sess.c_off, sess.c_tok, sess.c_next, sess.c_acc, sess.n, sess.stop_ids, sess.done)
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and not any(sess.active())
    sess.submit(0, PROMPTS[0], max_new_tokens=1, stop_token_ids=[8], constraint=TA.from_edges(1, [], [1]))      # with a stop id the lone state is fine
    assert sess.result(0)[0].tolist() == [8] and sess.result(0)[1] & 1
    small.submit(0, PROMPTS[0], max_new_tokens=3, constraint=TA.allowed_set(range(6)))                          # exactly what it holds
    small.run()
    assert set(small.result(0)[0].tolist()) <= set(range(6))
    assert not any(sess.active()) and not any(small.active())
    for bad in (dict(max_constraint_states=0), dict(max_constraint_edges=0), dict(max_constraint_states=(1 << 16) + 1), dict(max_constraint_edges=True)):
        with pytest.raises(ValueError):
            dec.session(constraints=True, **bad)


# ------------------------------------------------------------------------------------------------ 4. extend, load_tenant, log-probabilities
def test_extend_constrains_the_new_turn_and_load_tenant_resets_the_slot(dec128, TA):
    dec = dec128
    sess = dec.session(constraints=True)
    sess.submit(1, PROMPTS[1], max_new_tokens=8, constraint=TA.from_choices(CHOICES))
    sess.submit(2, PROMPTS[2], max_new_tokens=6, constraint=TA.allowed_set([50, 51]))
    sess.run()
    turn1, other = sess.result(1), sess.result(2)
    assert turn1[0].tolist() in CHOICES and turn1[1] == 8
    sess.extend(1, _toks(5, 9), max_new_tokens=8, constraint=TA.from_choices([[60, 61, 62]]))
    assert int(sess.c_n[1]) == 1 and int(sess.c_state[1]) == 1          # the new automaton, from ITS start state, advanced by the first token
    sess.run()
    assert sess.result(1)[0].tolist() == [60, 61, 62] and sess.result(1)[1] == 8       # this turn's tokens only; the turn before was what it was
    assert turn1[0].tolist() in CHOICES and sess.result(2)[0].tolist() == other[0].tolist() and int(sess.c_state[2]) == 0
    sess.extend(1, _toks(3, 4), max_new_tokens=4)                        # no constraint: the turn is free
    assert int(sess.c_state[1]) == -1
    sess.run()
    free = sess.result(1)
    assert free[0].numel() == 4 and free[1] == 2
    sess.extend(1, [], max_new_tokens=4, constraint=TA.allowed_set([70, 71, 72]))
    sess.run()
    assert set(sess.result(1)[0].tolist()) <= {70, 71, 72} and sess.result(1)[0].numel() == 4
    sess.load_tenant(1, {k: v for k, v in dec.tenant_state(1).items()})
    assert int(sess.c_state[1]) == -1 and int(sess.c_n[1]) == 0 and int(sess.c_state[2]) == 0
    with pytest.raises(RuntimeError):
        sess.extend(1, [3], constraint=TA.allowed_set([1]))
    sess.submit(1, PROMPTS[1], max_new_tokens=8, constraint=TA.from_choices(CHOICES))      # the same fine-tune, the same request: the first turn again
    sess.run()
    assert sess.result(1)[0].tolist() == turn1[0].tolist() and sess.result(1)[1] == 8


def test_log_probabilities_are_the_raw_logits(dec128, TA, monkeypatch):
    from bitdelta_amd import serving_ops as ops
    dec, K = dec128, 5
    plain = dec.session()
    plain.submit(0, PROMPTS[0], max_new_tokens=8)
    plain.run()
    model_choice = set(plain.result(0)[0].tolist())
    allowed = [i for i in range(V) if i not in model_choice][:200]       # everything the model would have said is forbidden
    rec = Recorder(monkeypatch)
    sess = dec.session(logprobs=K, constraints=True)
    sess.submit(0, PROMPTS[0], max_new_tokens=8, constraint=TA.allowed_set(allowed))
    sess.run(use_graph=False)
    toks = sess.result(0)[0]
    raws = [rec.first[-1]["logits"][0]] + [r["logits"][0] for r in rec.steps]
    assert toks.numel() == 8 and len(raws) == 8 and set(toks.tolist()) <= set(allowed)
    lp, ids, lps = sess.result_logprobs(0)
    w_lp, w_ids, w_lps = ops.token_logprobs(torch.stack(raws).cuda(), toks.cuda(), K)
    assert torch.equal(lp.view(torch.int32), w_lp.cpu().view(torch.int32)) and torch.equal(ids, w_ids.cpu())
    assert torch.equal(lps.view(torch.int32), w_lps.cpu().view(torch.int32))
    # the lists are the model's own: a masked token heads them, with a finite probability the request could never have drawn it at
    assert int(ids[0, 0]) in model_choice and bool(torch.isfinite(lps[:, 0]).all()) and bool(torch.isfinite(lp).all())
    assert set(ids[:, 0].tolist()) - set(allowed)
    graph = dec.session(logprobs=K, constraints=True)
    graph.submit(0, PROMPTS[0], max_new_tokens=8, constraint=TA.allowed_set(allowed))
    graph.run()
    assert torch.equal(graph.result(0)[0], toks) and torch.equal(graph.result_logprobs(0)[1], ids)
    assert torch.equal(graph.result_logprobs(0)[0].view(torch.int32), lp.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 5. the other reasons, and a plain session
def test_limits_still_end_a_constrained_tenant(dec128, TA):
    from bitdelta_amd.serving_loop import TenantDecoder
    dec = dec128
    sess = dec.session(constraints=True)
    sess.submit(0, PROMPTS[0], max_new_tokens=2, constraint=TA.from_choices([[30, 31, 32, 33]]))
    sess.submit(3, PROMPTS[3], max_new_tokens=5, constraint=TA.allowed_set([1, 2, 3]))
    sess.run()
    assert sess.result(0)[0].tolist() == [30, 31] and sess.result(0)[1] == 2 and int(sess.c_state[0]) == 2      # max_new_tokens, before completion
    assert sess.result(3)[0].numel() == 5 and sess.result(3)[1] == 2 and set(sess.result(3)[0].tolist()) <= {1, 2, 3}
    sess.submit(0, PROMPTS[0], max_new_tokens=4, constraint=TA.from_choices([[30, 31, 32, 33]]))              # both in one step: the step end's reason
    sess.run()
    assert sess.result(0)[0].tolist() == [30, 31, 32, 33] and sess.result(0)[1] == 2 and int(sess.c_state[0]) == 4
    small = TenantDecoder.synthetic("tiny128", 2, "cuda", dtype=torch.float16, seed=3, max_len=72)
    s2 = small.session(constraints=True)
    s2.submit(1, PROMPTS[0], max_new_tokens=50, constraint=TA.allowed_set(range(100, 140)))      # 64 padded rows + 8 more: the cache is full first
    s2.run()
    assert s2.result(1)[1] == 4 and s2.result(1)[0].numel() == 9 and set(s2.result(1)[0].tolist()) <= set(range(100, 140))
    assert int(s2.c_state[0]) == -1 and int(s2.c_n[0]) == 0              # the idle slot was not touched


def test_a_session_without_constraints_has_none_of_it(dec128, TA, monkeypatch):
    from bitdelta_amd import serving_ops as ops
    dec = dec128
    calls = []
    for name in [n for n in dir(ops) if n.startswith("step_") or n in ("constrain_rows", "penalize_rows", "sample_rows", "token_logprobs")]:
        def wrap(fn, name):
            def f(*a, **k):
                calls.append(name)
                return fn(*a, **k)
            return f
        monkeypatch.setattr(ops, name, wrap(getattr(ops, name), name))
    a = TA.allowed_set([1, 2])
    launches = {}
    for kind, kw in (("greedy", {}), ("sampling", dict(sampling=True)), ("logprobs", dict(logprobs=3)), ("penalties", dict(penalties=True))):
        plain = dec.session(**kw)
        assert plain.constraints is False
        assert not any(hasattr(plain, n) for n in ("c_state", "c_n", "c_off", "c_tok", "c_next", "c_acc", "clogits"))
        with pytest.raises(ValueError, match="constraints=True"):
            plain.submit(0, PROMPTS[0], constraint=a)
        with pytest.raises(ValueError, match="constraints=True"):
            plain.submit_all(PROMPTS, constraint=a)
        with pytest.raises(ValueError, match="constraints=True"):
            plain.submit_all(PROMPTS, constraint=[None, a, None, None])
        assert not any(plain.active())
        del calls[:]
        plain.submit(0, PROMPTS[0], max_new_tokens=4, constraint=None)
        plain.step(1, use_graph=False)
        launches[kind] = list(calls)
        assert not [c for c in calls if "constrain" in c]
        plain.run()
        (key,) = plain._graphs
        assert key[-1] is False and len(key) == 10                      # the parent's key and the flag
        with_flag = dec.session(constraints=True, **kw)
        del calls[:]
        with_flag.submit(0, PROMPTS[0], max_new_tokens=4)
        with_flag.step(1, use_graph=False)
        extra = list(calls)
        for c in launches[kind]:                                         # the same launches in the same order, plus the three of the constraint
            extra.remove(c)
        assert sorted(extra) == ["constrain_rows", "step_constrain", "step_constrain_advance"], kind
        assert calls[-1] == "step_constrain_advance"
        with_flag.run()
        assert with_flag.result(0)[0].tolist() == plain.result(0)[0].tolist()
    assert "step_end_ragged" in launches["greedy"] and "step_end_sample" in launches["sampling"] and "step_penalize" in launches["penalties"]
