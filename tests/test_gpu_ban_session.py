"""GPU tests of the hard bans in a TenantSession (serving_loop.py, session(bans=True)) on a two-layer synthetic decoder, V = 512, 24-token
turns, prompts of pairwise distinct tokens.  A FREE run comes first; the greedy expectations are exact: a session with logprobs=20 reports the
20 most probable tokens of every step's RAW row, and token j of a banned tenant must be the first of them that the restatement of the definition
(tests/ban_ref.py) does not ban after the history of step j.  Fewer than 20 tokens are ever banned at a step -- asserted at every step, not
assumed -- so that entry exists.  The free run is asserted to do what the bans forbid (it repeats a g-gram, contains the bad word, stops after
four tokens): no test passes vacuously."""
import math

import pytest
import torch

import ban_ref as ref

pytestmark = pytest.mark.gpu

V = 512
N = 24                       # tokens of a free turn
K = 20                       # logprobs: the alternatives kept per step
SAMPLING = [dict(temperature=1.0, top_k=0, top_p=1.0, seed=2 ** 63 + 17), dict(temperature=0.7, top_k=20, top_p=0.9, seed=11),
            dict(temperature=0.9, top_k=50, top_p=1.0, seed=5), dict(temperature=1.5, top_k=0, top_p=0.8, seed=2 ** 64 - 1)]
PEN = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25, logit_bias={5: 2.0, 17: -math.inf, 300: -1.5})


@pytest.fixture(scope="module")
def dec128():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib
    from bitdelta_amd.serving_loop import TenantDecoder
    _lib.lib()
    return TenantDecoder.synthetic("tiny128", 4, "cuda", dtype=torch.float16, seed=31, max_len=256)


def _distinct(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randperm(499, generator=g)[:n] + 1).tolist()


PROMPTS = [_distinct(n, 60 + n) for n in (9, 64, 33, 70)]


def test_prompts_hold_pairwise_distinct_tokens():
    assert all(len(set(p)) == len(p) and all(1 <= v < V for v in p) for p in PROMPTS)


def _results(sess):
    return [(sess.result(t)[0].tolist(), sess.result(t)[1]) for t in range(sess.T)]


def _run(sess, mode):
    if mode == "graph":
        sess.run()
    elif mode == "every4":
        sess.run(check_every=4)
    else:
        sess.run(use_graph=False)


@pytest.fixture(scope="module")
def free(dec128):
    """greedy and sampled free runs in sessions made WITHOUT the feature, run once, never modified: {kind: [(tokens, reason)] * 4}"""
    res = {}
    for kind in ("greedy", "sampling"):
        sess = dec128.session(sampling=kind == "sampling", logprobs=K)
        for t in range(4):
            sess.submit(t, PROMPTS[t], max_new_tokens=N, **(SAMPLING[t] if kind == "sampling" else {}))
        sess.run()
        res[kind] = _results(sess)
        assert all(len(y) == N and r == 2 for y, r in res[kind])
    return res


def _follows_the_rule(sess, t, conv, g=0, words=(), min_new=0, stops=()):
    """every token of tenant t's turn is the first of its step's 20 most probable raw tokens that is not banned after conv + the turn so far;
    returns (tokens, the number of steps at which the raw argmax was banned)"""
    y = sess.result(t)[0].tolist()
    top = sess.result_logprobs(t)[1].tolist()
    assert len(top) == len(y) >= 1 and all(len(row) == K for row in top)
    moved = 0
    for j in range(len(y)):                                              # no step is skipped
        b = ref.banned(list(conv) + y[:j], g, words, j, min_new, stops)
        assert len(b) < K, (t, j, len(b))                                # the condition the top-20 rule rests on
        want = next(v for v in top[j] if v not in b)
        assert y[j] == want, (t, j, y, top[j][:4], sorted(b))
        moved += top[j][0] in b
    return y, moved


# ------------------------------------------------------------------------------------------------ 1. exact greedy trajectories, every stepping mode
@pytest.mark.parametrize("mode", ["graph", "every4", "eager"])
def test_ngram_bans_give_the_exact_greedy_trajectory_and_nobody_else_notices(dec128, free, mode):
    fr = free["greedy"]
    assert ref.repeats_ngram(PROMPTS[1] + fr[1][0], 2) and ref.repeats_ngram(PROMPTS[2] + fr[2][0], 3)      # the free run does repeat itself
    sess = dec128.session(logprobs=K, bans=True)
    sess.submit(0, PROMPTS[0], max_new_tokens=N)
    sess.submit(1, PROMPTS[1], max_new_tokens=N, no_repeat_ngram_size=2)
    sess.submit(2, PROMPTS[2], max_new_tokens=N, no_repeat_ngram_size=3)
    sess.submit(3, PROMPTS[3], max_new_tokens=N, no_repeat_ngram_size=0, bad_words=(), min_new_tokens=0)
    _run(sess, mode)
    got = _results(sess)
    assert got[0] == fr[0] and got[3] == fr[3]                           # bit-identical to the run without the feature
    for t, g in ((1, 2), (2, 3)):
        y, moved = _follows_the_rule(sess, t, PROMPTS[t], g=g)
        assert len(y) == N and got[t][1] == 2 and moved >= 1 and y != fr[t][0]
        assert not ref.repeats_ngram(PROMPTS[t] + y, g)
        assert max(y.count(v) for v in set(y)) <= 13 or g != 2           # x x can occur once: at most 13 of 24
    assert not any(sess.active())
    if mode != "graph":                                                  # all three modes give identical tokens for the banned tenants too
        twin = dec128.session(logprobs=K, bans=True)
        twin.submit(1, PROMPTS[1], max_new_tokens=N, no_repeat_ngram_size=2)
        twin.submit(2, PROMPTS[2], max_new_tokens=N, no_repeat_ngram_size=3)
        twin.run()
        assert _results(twin)[1] == got[1] and _results(twin)[2] == got[2]


def test_bad_words_from_the_free_run_and_the_first_token_at_admission(dec128, free):
    y0 = free["greedy"][1][0]
    words = [[PROMPTS[1][-1], y0[0]], [y0[3], y0[4]], [y0[7]]]           # the first completes at ADMISSION, across the prompt; a pair; a single token
    assert ref.completes_word(PROMPTS[1], y0, words[:1]) and ref.completes_word(PROMPTS[1], y0, words[1:2]) and y0[7] in y0
    sess = dec128.session(logprobs=K, bans=True)
    sess.submit(1, PROMPTS[1], max_new_tokens=N, bad_words=words)
    assert int(sess.n[1]) == 1 and sess.result(1)[0].tolist()[0] != y0[0]      # the first token obeys the bans
    sess.run()
    y, moved = _follows_the_rule(sess, 1, PROMPTS[1], words=words)
    assert len(y) == N and moved >= 1 and y0[7] not in y and not ref.completes_word(PROMPTS[1], y, words)
    # a two-token bad word right behind a ONE-token prompt is banned (where HF skips it)
    sess.submit(0, PROMPTS[0][:1], max_new_tokens=4, logit_bias=None)
    first = sess.result(0)[0].tolist()[0]
    sess.run()
    sess.submit(0, PROMPTS[0][:1], max_new_tokens=4, bad_words=[[PROMPTS[0][0], first]])
    assert sess.result(0)[0].tolist()[0] != first
    sess.run()
    _follows_the_rule(sess, 0, PROMPTS[0][:1], words=[[PROMPTS[0][0], first]])


def test_min_new_tokens_holds_back_the_stop_id(dec128, free):
    y0 = free["greedy"][0][0]
    stop = y0[3]
    plain = dec128.session(logprobs=K)
    plain.submit(0, PROMPTS[0], max_new_tokens=N, stop_token_ids=[stop])
    plain.run()
    assert _results(plain)[0] == (y0[:4], 1)                             # the free run stops at 4 tokens
    sess = dec128.session(logprobs=K, bans=True)
    sess.submit(0, PROMPTS[0], max_new_tokens=N, stop_token_ids=[stop], min_new_tokens=8)
    sess.run()
    y, moved = _follows_the_rule(sess, 0, PROMPTS[0], min_new=8, stops=[stop])
    assert moved >= 1 and stop not in y[:8] and len(y) >= 8 and y[:3] == y0[:3]
    reason = sess.result(0)[1]
    assert bool(reason & 1) == (y[-1] == stop) and bool(reason & 2) == (len(y) == N) and reason in (1, 2, 3) and stop not in y[:-1]
    # n = min - 1 is still held back, n = min is not: with min_new_tokens = 3 the free run's own fourth token ends the turn
    sess.submit(0, PROMPTS[0], max_new_tokens=N, stop_token_ids=[stop], min_new_tokens=3)
    sess.run()
    assert _results(sess)[0] == (y0[:4], 1)
    # it holds back stop IDS only: a stop sequence still ends the turn early (reason 16)
    both = dec128.session(logprobs=K, bans=True, stop_sequences=True)
    both.submit(0, PROMPTS[0], max_new_tokens=N, stop_token_ids=[stop], min_new_tokens=8, stop_sequences=[y0[1:3]])
    both.run()
    assert _results(both)[0] == (y0[:3], 16)


# ------------------------------------------------------------------------------------------------ 2. sampling sessions: properties
@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_sampling_sessions_obey_every_ban(dec128, free, mode):
    fr = free["sampling"]
    words = [[fr[1][0][2]], [PROMPTS[1][-1], fr[1][0][0]], [fr[1][0][5], fr[1][0][6]]]
    stop = fr[2][0][1]
    sess = dec128.session(sampling=True, bans=True)
    sess.submit(0, PROMPTS[0], max_new_tokens=N, no_repeat_ngram_size=1, **SAMPLING[0])
    sess.submit(1, PROMPTS[1], max_new_tokens=N, no_repeat_ngram_size=3, bad_words=words, **SAMPLING[1])
    sess.submit(2, PROMPTS[2], max_new_tokens=N, stop_token_ids=[stop], min_new_tokens=8, no_repeat_ngram_size=2, **SAMPLING[2])
    sess.submit(3, PROMPTS[3], max_new_tokens=N, **SAMPLING[3])
    _run(sess, mode)
    got = _results(sess)
    assert got[3] == fr[3]
    assert len(set(PROMPTS[0] + got[0][0])) == len(PROMPTS[0]) + N       # g = 1: no token twice, the prompt's included
    assert not ref.repeats_ngram(PROMPTS[1] + got[1][0], 3) and not ref.completes_word(PROMPTS[1], got[1][0], words) and len(got[1][0]) == N
    assert ref.completes_word(PROMPTS[1], fr[1][0], words)               # (the free sampled run does complete one)
    assert stop not in got[2][0][:8] and len(got[2][0]) >= 8 and not ref.repeats_ngram(PROMPTS[2] + got[2][0], 2)
    assert fr[2][0].index(stop) < 8


# ------------------------------------------------------------------------------------------------ 3. one capture, extend, load_tenant
def test_parameters_change_between_requests_on_one_capture(dec128, free):
    y0 = free["greedy"][2][0]
    sess = dec128.session(logprobs=K, bans=True)
    reqs = [dict(no_repeat_ngram_size=2), dict(bad_words=[[y0[1]], [y0[2], y0[3]]]), dict(), dict(no_repeat_ngram_size=8),
            dict(no_repeat_ngram_size=4, bad_words=[[y0[0]]] * 16, min_new_tokens=5, stop_token_ids=[y0[2]])]
    for kw in reqs:
        sess.submit(2, PROMPTS[2], max_new_tokens=N, **kw)
        sess.run()
        y, _ = _follows_the_rule(sess, 2, PROMPTS[2], g=kw.get("no_repeat_ngram_size", 0), words=kw.get("bad_words", ()),
                                 min_new=kw.get("min_new_tokens", 0), stops=kw.get("stop_token_ids", ()))
        if not kw:
            assert (y, 2) == free["greedy"][2]
        assert len(sess._graphs) == 1
    (key,) = sess._graphs
    assert key[-3:] == ("bans", 16, 8) and len(key) == 13
    # the refusals come before anything is touched
    names = ("ctx", "ctx_len", "ban_ngram", "ban_tok", "ban_len", "ban_min", "n", "done", "out")
    before = [getattr(sess, k).clone() for k in names] + [c.clone() for c in sess.cache["k"] + sess.cache["v"]]
    for bad in (dict(no_repeat_ngram_size=9), dict(no_repeat_ngram_size=True), dict(bad_words=[[]]), dict(bad_words=[[V]]), dict(bad_words=[[1]] * 17),
                dict(bad_words=[[1] * 9]), dict(min_new_tokens=-1), dict(min_new_tokens=1.5)):
        with pytest.raises(ValueError):
            sess.submit(2, PROMPTS[2], **bad)
        with pytest.raises(ValueError):
            sess.extend(2, [5], **bad)
    with pytest.raises(ValueError):
        sess.submit_all(PROMPTS, no_repeat_ngram_size=[0, 0, 9, 0])
    with pytest.raises(ValueError):
        sess.submit_all(PROMPTS, bad_words=[[], [], [[V]], []])
    after = [getattr(sess, k) for k in names] + sess.cache["k"] + sess.cache["v"]
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and not any(sess.active())
    # other sizes are another session and another graph key; submit_all takes one value or one per tenant
    big = dec128.session(logprobs=K, bans=True, max_bad_words=64, max_bad_word_len=32)
    assert big.ban_tok.shape == (4, 64, 32) and big.ctx.shape == (4, big.Lc) and big.blogits.shape == (4, V)
    plain = dec128.session(logprobs=K)
    plain.submit_all(PROMPTS, max_new_tokens=N)
    plain.run()
    long_word = PROMPTS[1][-31:] + [_results(plain)[1][0][0]]
    big.submit_all(PROMPTS, max_new_tokens=N, no_repeat_ngram_size=[0, 0, 2, 3], bad_words=[[], [long_word] + [[9] * 32] * 63, [], []],
                   min_new_tokens=0)
    big.run()
    assert next(iter(big._graphs))[-3:] == ("bans", 64, 32)
    assert _results(big)[0] == _results(plain)[0]
    assert _results(big)[1][0][0] != long_word[-1]                       # a 32-token word across the whole table width, completed at admission
    _follows_the_rule(big, 1, PROMPTS[1], words=[long_word])
    _follows_the_rule(big, 2, PROMPTS[2], g=2)
    _follows_the_rule(big, 3, PROMPTS[3], g=3)


def test_extend_bans_over_the_whole_conversation_and_load_tenant_clears(dec128):
    dec, t = dec128, 1
    # the twin: the same two turns, free.  Its second turn repeats a 2-gram whose first occurrence lies wholly in turn one
    twin = dec.session(logprobs=K)
    twin.submit(t, PROMPTS[t], max_new_tokens=12)
    twin.run()
    y1 = _results(twin)[t][0]
    twin.extend(t, [], max_new_tokens=12)
    twin.run()
    y2_free = _results(twin)[t][0]
    conv1 = PROMPTS[t] + y1
    full = conv1 + y2_free
    seen_in_turn_one = {(a, b) for a, b in zip(conv1, conv1[1:])}
    assert any((full[k], full[k + 1]) in seen_in_turn_one for k in range(len(conv1) - 1, len(full) - 1)), "the free second turn repeats nothing"
    sess = dec.session(logprobs=K, bans=True)
    sess.submit(t, PROMPTS[t], max_new_tokens=12)                        # turn one carries no ban
    sess.submit(2, PROMPTS[2], max_new_tokens=N, no_repeat_ngram_size=2)
    sess.run()
    assert _results(sess)[t] == (y1, 2) and sess._ctx_tokens[t] == PROMPTS[t]
    other = _results(sess)[2]
    sess.extend(t, [], max_new_tokens=12, no_repeat_ngram_size=2)
    assert sess._ctx_tokens[t] == conv1 and int(sess.ctx_len[t]) == len(conv1) and sess.ctx[t, :len(conv1)].tolist() == conv1
    sess.run()
    y2, moved = _follows_the_rule(sess, t, conv1, g=2)                   # the same top-20 rule over the whole conversation
    assert moved >= 1 and y2 != y2_free and len(y2) == 12
    assert not any((a, b) in seen_in_turn_one for a, b in zip((conv1 + y2)[len(conv1) - 1:], (conv1 + y2)[len(conv1):]))
    more = _distinct(5, 7)
    sess.extend(t, more, max_new_tokens=8, no_repeat_ngram_size=3, bad_words=[[more[-1], y2[0]]], min_new_tokens=2)
    conv2 = conv1 + y2 + more
    assert sess._ctx_tokens[t] == conv2 and sess.ctx[t, :len(conv2)].tolist() == conv2
    sess.run()
    _follows_the_rule(sess, t, conv2, g=3, words=[[more[-1], y2[0]]], min_new=2)
    assert _results(sess)[2] == other                                    # the other tenant's turn was not touched
    # load_tenant clears the slot; the same fine-tune and request give the same turn again
    sess.submit(t, PROMPTS[t], max_new_tokens=N, no_repeat_ngram_size=2, bad_words=[[y1[0]]], min_new_tokens=3)
    sess.run()
    first = _results(sess)[t]
    sess.load_tenant(t, {k: v for k, v in dec.tenant_state(t).items()})
    assert (int(sess.ban_ngram[t]), int(sess.ban_min[t]), int(sess.ctx_len[t])) == (0, 0, 0) and sess.ban_len[t].tolist() == [0] * 16
    assert bool((sess.ban_tok[t] == -1).all()) and sess._ctx_tokens[t] == [] and int(sess.ban_ngram[2]) == 2
    sess.submit(t, PROMPTS[t], max_new_tokens=N, no_repeat_ngram_size=2, bad_words=[[y1[0]]], min_new_tokens=3)
    sess.run()
    assert _results(sess)[t] == first and first[0][0] != y1[0]


# ------------------------------------------------------------------------------------------------ 4. next to every other feature
def test_with_every_other_feature_switched_on_and_a_ban_beats_a_positive_bias(dec128):
    from bitdelta_amd.constraint import TokenAutomaton as TA
    dec = dec128
    allowed_ids = list(range(64, 192, 3))
    allowed = TA.allowed_set(allowed_ids)
    kw = dict(sampling=True, logprobs=5, penalties=True, constraints=True, stop_sequences=True)
    par = lambda t: dict(PEN, **SAMPLING[t])
    plain = dec.session(**kw)
    for t in (0, 1):
        plain.submit(t, PROMPTS[t], max_new_tokens=16, constraint=allowed, **par(t))
    plain.run()
    base = _results(plain)
    y0 = base[1][0]
    assert len(y0) == 16 and set(y0) <= set(allowed_ids)
    stop = y0[1]
    sess = dec.session(bans=True, **kw)
    sess.submit(0, PROMPTS[0], max_new_tokens=16, constraint=allowed, **par(0))
    sess.submit(1, PROMPTS[1], max_new_tokens=16, constraint=allowed, stop_token_ids=[stop], no_repeat_ngram_size=1, bad_words=[[y0[0]]],
                min_new_tokens=6, stop_sequences=[[400, 401]], **par(1))
    sess.run()
    got = _results(sess)
    assert got[0] == base[0]
    y = got[1][0]
    assert set(y) <= set(allowed_ids) and len(set(y)) == len(y) and y0[0] not in y and stop not in y[:6] and len(y) >= 6
    assert sess.result_logprobs(1)[0].shape == (len(y),) and len(sess._graphs) == 1
    # a ban wins over a positive logit bias: +100 forces the token at every step, the bad word removes it
    pen = dec.session(logprobs=K, penalties=True, bans=True)
    pen.submit(2, PROMPTS[2], max_new_tokens=6, logit_bias={77: 100.0})
    pen.run()
    assert _results(pen)[2][0] == [77] * 6
    pen.submit(2, PROMPTS[2], max_new_tokens=6, logit_bias={77: 100.0}, bad_words=[[77]])
    pen.run()
    assert 77 not in _results(pen)[2][0]
    lp, ids, _ = pen.result_logprobs(2)                                  # ... and the log-probabilities still describe the RAW row
    free_run = dec.session(logprobs=K)
    free_run.submit(2, PROMPTS[2], max_new_tokens=1)
    assert torch.equal(ids[0], free_run.result_logprobs(2)[1][0])


# ------------------------------------------------------------------------------------------------ 5. a session made without the feature
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
    for kind in ("greedy", "sampling"):
        par = (lambda t: SAMPLING[t]) if kind == "sampling" else (lambda t: {})
        plain = dec.session(sampling=kind == "sampling", logprobs=K)
        assert plain.bans is False
        assert not any(hasattr(plain, n) for n in ("ctx", "ctx_len", "ban_ngram", "ban_tok", "ban_len", "ban_min", "blogits", "_ctx_tokens"))
        for bad in (dict(no_repeat_ngram_size=2), dict(bad_words=[[5]]), dict(min_new_tokens=1)):
            with pytest.raises(ValueError, match="bans=True"):
                plain.submit(0, PROMPTS[0], **bad)
            with pytest.raises(ValueError, match="bans=True"):
                plain.submit_all(PROMPTS, **bad)
        with pytest.raises(ValueError, match="bans=True"):
            plain.submit_all(PROMPTS, no_repeat_ngram_size=[0, 0, 2, 0])
        assert not any(plain.active())
        del calls[:]
        for t in range(4):
            plain.submit(t, PROMPTS[t], max_new_tokens=N, no_repeat_ngram_size=0, bad_words=[], min_new_tokens=0, **par(t))      # defaults are no request
        plain.step(1, use_graph=False)
        before = list(calls)
        assert "step_ban" not in before
        plain.run()
        assert _results(plain) == free[kind]
        (key,) = plain._graphs
        assert len(key) == 10                                            # the key it had
        with_flag = dec.session(sampling=kind == "sampling", logprobs=K, bans=True)
        del calls[:]
        for t in range(4):
            with_flag.submit(t, PROMPTS[t], max_new_tokens=N, **par(t))
        with_flag.step(1, use_graph=False)
        assert calls == ["step_begin_ragged", "step_ban"] + before[1:]   # the same launches in the same order, and one more in front of the step end
        with_flag.run()
        assert _results(with_flag) == free[kind]                         # nothing banned: the free run bit for bit
    with pytest.raises(ValueError):
        dec.session(bans=True, max_bad_words=65)
    with pytest.raises(ValueError):
        dec.session(bans=True, max_bad_word_len=33)
    with pytest.raises(ValueError):
        dec.session(bans=True, max_stop_ids=65)
