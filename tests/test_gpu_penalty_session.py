"""GPU tests of the request penalties in a TenantSession (serving_loop.py, session(penalties=True)) on two-layer synthetic decoders, V = 512: a
penalty session with neutral parameters is the plain session; with non-neutral ones every emitted token is chosen from the restatement's row
(tests/penalty_ref.py) for the logits the step saw and the history so far, the first token from the prefill included; graph replay, the other
tenants and the order of admission do not change a tenant's tokens or its history; the history holds exactly the prompt's tokens and the counts
of the tokens fed back; extend folds it; parameters change between requests on one capture; bans and forced tokens; load_tenant; the raw
log-probabilities; retirement reasons; and a session made without penalties=True has none of it."""
import math

import pytest
import torch

import penalty_ref as ref

pytestmark = pytest.mark.gpu

V = 512
SAMPLING = [dict(temperature=1.0, top_k=0, top_p=1.0, seed=2 ** 63 + 17), dict(temperature=0.7, top_k=20, top_p=0.9, seed=11),
            dict(temperature=0.0, top_k=0, top_p=1.0, seed=0), dict(temperature=1.5, top_k=0, top_p=0.8, seed=2 ** 64 - 1)]
PEN = [dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25, logit_bias={5: 2.0, 17: -math.inf, 300: -1.5}),
       dict(repetition_penalty=0.8, frequency_penalty=1.0),
       dict(presence_penalty=-0.5, logit_bias={i: 0.125 * i for i in range(16)}),
       dict(repetition_penalty=2.0, presence_penalty=1.0, frequency_penalty=1.0)]


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


def _results(sess):
    return [(sess.result(t)[0].tolist(), sess.result(t)[1]) for t in range(sess.T)]


def _bits(h):
    return h.cpu().to(torch.int32) & 0xffff


def _history_is(sess, t, context, fed):
    """tenant t's history row: bit 15 exactly at the tokens of `context`, the count bits the number of times each token of `fed` was fed back"""
    h = _bits(sess.hist[t])
    want = torch.zeros(V, dtype=torch.int32)
    want[torch.tensor(sorted(set(context)))] = 0x8000
    want += torch.bincount(torch.tensor(fed, dtype=torch.long), minlength=V).to(torch.int32)
    return torch.equal(h, want)


class Recorder:
    """serving_ops.penalize_rows / step_penalize wrapped to keep what they were given and what they wrote"""

    def __init__(self, monkeypatch):
        from bitdelta_amd import serving_ops as ops
        self.first, self.steps = [], []
        orig_rows, orig_step = ops.penalize_rows, ops.step_penalize
        cp = lambda x: x.detach().cpu().clone()

        def rows(logits, hist, pen, bias_id=None, bias_val=None, out=None):
            res = orig_rows(logits, hist, pen, bias_id, bias_val, out)
            self.first.append(dict(logits=cp(logits), hist=cp(hist), pen=cp(pen), bias_id=cp(bias_id), bias_val=cp(bias_val), out=cp(res)))
            return res

        def step(logits, out, hist, tok, active, pen, bias_id=None, bias_val=None):
            if torch.cuda.is_current_stream_capturing():             # (a capture takes no copies to the host; replays do not come through here)
                return orig_step(logits, out, hist, tok, active, pen, bias_id, bias_val)
            rec = dict(logits=cp(logits), hist=cp(hist), pen=cp(pen), bias_id=cp(bias_id), bias_val=cp(bias_val), tok=cp(tok).reshape(-1),
                       active=cp(active), prev=cp(out))
            res = orig_step(logits, out, hist, tok, active, pen, bias_id, bias_val)
            rec.update(out=cp(res), hist_after=cp(hist))
            self.steps.append(rec)
            return res
        monkeypatch.setattr(ops, "penalize_rows", rows)
        monkeypatch.setattr(ops, "step_penalize", step)

    def check_first(self, rec):
        """the restatement's rows for a recorded admission; the launch wrote exactly them"""
        out, _ = ref.penalize(rec["logits"], rec["hist"], rec["pen"], rec["bias_id"], rec["bias_val"])
        assert ref.same_bits(out, rec["out"])
        return out

    def check_step(self, rec):
        out, hist = ref.penalize(rec["logits"], rec["hist"], rec["pen"], rec["bias_id"], rec["bias_val"], tok=rec["tok"], active=rec["active"],
                                 out=rec["prev"])
        assert ref.same_bits(out, rec["out"]) and torch.equal(hist, rec["hist_after"])
        return out


# ------------------------------------------------------------------------------------------------ 1. neutral parameters: the plain session
@pytest.mark.parametrize("sampling", [False, True], ids=["greedy", "sampling"])
@pytest.mark.parametrize("name,T,dtype", [("tiny128", 4, torch.float16), ("tiny2048", 3, torch.bfloat16)])
def test_penalty_session_with_neutral_parameters_is_the_plain_session(name, T, dtype, sampling):
    from bitdelta_amd.serving_loop import TenantDecoder
    dec = TenantDecoder.synthetic(name, T, "cuda", dtype=dtype, seed=31, max_len=192, shared_heads=True)
    plain, pens = dec.session(sampling=sampling), dec.session(sampling=sampling, penalties=True)
    par = {q: [P[q] for P in SAMPLING[:T]] for q in SAMPLING[0]} if sampling else {}
    one = (lambda t: SAMPLING[t]) if sampling else (lambda t: {})
    for use_graph in (True, False):
        got = []
        for sess in (plain, pens):
            sess.submit_all(PROMPTS[:T], max_new_tokens=12, stop_token_ids=[[], [3], [], [5]][:T], **par)
            sess.run(use_graph=use_graph)
            got.append(_results(sess))
        assert got[0] == got[1], use_graph
        assert all(len(toks) >= 1 and reason in (1, 2) for toks, reason in got[0])
    got = []
    for sess in (plain, pens):                                           # one tenant at a time, another order, an extension
        for t in (2, 0):
            sess.submit(t, PROMPTS[t], max_new_tokens=5, **one(t))
        sess.run()
        sess.extend(0, _toks(7, 3), max_new_tokens=4, **one(0))
        sess.run()
        got.append(_results(sess))
    assert got[0] == got[1]
    assert pens.plogits.dtype == dtype and pens.hist.shape == (T, V) and len(pens._graphs) == 1


# ------------------------------------------------------------------------------------------------ 2. every token against the restatement
@pytest.mark.parametrize("sampling", [False, True], ids=["greedy", "sampling"])
def test_every_emitted_token_is_chosen_from_the_restatements_row(dec128, monkeypatch, sampling):
    """eager steps with the two penalty launches wrapped: the row each launch wrote is the restatement's for the logits it was given and the
    history so far, and the token the step emitted is the choice from THAT row -- the argmax, or sample_rows' draw with the request's own
    parameters and draw index"""
    from bitdelta_amd import serving_ops as ops
    dec = dec128
    rec = Recorder(monkeypatch)
    sess = dec.session(sampling=sampling, penalties=True)
    par = (lambda t: dict(PEN[t], **SAMPLING[t])) if sampling else (lambda t: PEN[t])
    emitted = {t: [] for t in range(4)}

    def choose(rows, ts, draw):
        if not sampling:
            return torch.argmax(rows.float(), dim=-1).tolist()
        ts = torch.tensor(ts, device="cuda")
        return ops.sample_rows(rows.cuda(), sess.temperature[ts], sess.top_k[ts], sess.top_p[ts], sess.seed[ts], draw.cuda()).tolist()

    def admitted(t, context):
        r = rec.first[-1]
        assert r["logits"].shape == (1, V) and torch.equal(_bits(r["hist"][0]), _bits(ref.history(context, V=V)))
        want = choose(rec.check_first(r), [t], sess.pos[t:t + 1].cpu())
        emitted[t] = [int(sess.tok[t, 0])]
        assert emitted[t] == want, t

    def run(k):
        for _ in range(k):
            act = sess.active()
            if not any(act):
                break
            draw = (sess.pos + 1).cpu()
            sess.step(1, use_graph=False)
            out = rec.check_step(rec.steps[-1])
            assert rec.steps[-1]["active"].tolist() == act
            ts = [t for t in range(4) if act[t]]
            want = choose(out[ts], ts, draw[ts])
            for t, w in zip(ts, want):
                emitted[t].append(int(sess.tok[t, 0]))
                assert emitted[t][-1] == w, (t, len(emitted[t]))
    sess.submit(0, PROMPTS[0], max_new_tokens=12, **par(0)); admitted(0, PROMPTS[0])
    run(2)
    sess.submit(1, PROMPTS[1], max_new_tokens=3, **par(1)); admitted(1, PROMPTS[1])
    run(3)
    sess.submit(2, PROMPTS[2], max_new_tokens=9, **par(2)); admitted(2, PROMPTS[2])
    run(40)
    assert not any(sess.active()) and [sess.result(t)[0].tolist() for t in range(3)] == [emitted[t] for t in range(3)]
    assert [len(emitted[t]) for t in range(4)] == [12, 3, 9, 0]
    assert 17 not in emitted[0]                                          # (banned)
    turn1 = list(emitted[1])
    new = _toks(6, 8)
    sess.extend(1, new, max_new_tokens=4, **par(1)); admitted(1, PROMPTS[1] + turn1 + new)
    run(40)
    assert sess.result(1)[0].tolist() == emitted[1] and len(emitted[1]) == 4 and len(rec.steps) <= 24
    # the histories after retirement: the context of the turn, and one count per token fed back (every emitted token but the last)
    assert _history_is(sess, 0, PROMPTS[0], emitted[0][:-1]) and _history_is(sess, 2, PROMPTS[2], emitted[2][:-1])
    assert _history_is(sess, 1, PROMPTS[1] + turn1 + new, emitted[1][:-1])
    assert not bool(sess.hist[3].any())


# ------------------------------------------------------------------------------------------------ 3. graph / eager, independence, one capture
def _request(sess, ts, use_graph=True, mx=10, params=PEN):
    for t in ts:
        sess.submit(t, PROMPTS[t], max_new_tokens=mx, **params[t])
    sess.run(use_graph=use_graph)
    return {t: (sess.result(t)[0].tolist(), sess.result(t)[1], sess.hist[t].cpu().clone()) for t in ts}


def _same(a, b):
    return a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2])


@pytest.mark.parametrize("sampling", [False, True], ids=["greedy", "sampling"])
def test_graph_equals_eager_and_tokens_do_not_depend_on_the_other_tenants(dec128, sampling):
    dec = dec128
    params = [dict(PEN[t], **SAMPLING[t]) for t in range(4)] if sampling else PEN
    sess = dec.session(sampling=sampling, penalties=True)
    eager = _request(sess, range(4), use_graph=False, params=params)
    graph = _request(sess, range(4), use_graph=True, params=params)
    again = _request(sess, range(4), use_graph=True, params=params)
    for t in range(4):
        assert _same(eager[t], graph[t]) and _same(graph[t], again[t]) and len(graph[t][0]) == 10 and graph[t][1] == 2, t
        assert _history_is(sess, t, PROMPTS[t], graph[t][0][:-1]), t       # counts = bincount(result tokens[:-1]), bit 15 = the prompt's tokens
    assert len(sess._graphs) == 1
    for t in range(4):                                                   # alone
        assert _same(_request(sess, [t], params=params)[t], graph[t]), t
    sess.submit(0, PROMPTS[0], max_new_tokens=10, **params[0])           # admitted while others are mid-generation, in another order
    sess.step(3)
    sess.submit(3, PROMPTS[3], max_new_tokens=10, **params[3])
    sess.step(2)
    sess.submit(2, PROMPTS[2], max_new_tokens=10, **params[2])
    sess.run()
    for t in (0, 2, 3):
        assert (sess.result(t)[0].tolist(), sess.result(t)[1]) == graph[t][:2] and torch.equal(sess.hist[t].cpu(), graph[t][2]), t
    assert len(sess._graphs) == 1
    assert 17 not in graph[0][0]


def test_parameters_change_between_requests_on_one_capture(dec128):
    dec = dec128
    sess, plain = dec.session(penalties=True), dec.session()
    base = _request(sess, [1], mx=16, params=[{}] * 4)[1][0]
    graphs = dict(sess._graphs)
    plain.submit(1, PROMPTS[1], max_new_tokens=16)
    plain.run()
    assert base == plain.result(1)[0].tolist()
    for p in (dict(repetition_penalty=1.5), dict(frequency_penalty=2.0, presence_penalty=1.0), dict(logit_bias={base[1]: -math.inf}),
              dict(repetition_penalty=0.5, logit_bias={base[0]: -math.inf, 9: 3.0})):
        toks = _request(sess, [1], mx=16, params=[p] * 4)[1][0]
        assert len(toks) == 16, p
        assert all(i not in toks for i, b in p.get("logit_bias", {}).items() if b == -math.inf), p      # so these differ from the neutral run
    assert _request(sess, [1], mx=16, params=[{}] * 4)[1][0] == base       # back to neutral: the plain tokens again
    assert dict(sess._graphs) == graphs and len(graphs) == 1             # new parameters, the same captured graph object
    with pytest.raises(ValueError):
        sess.submit(0, PROMPTS[0], repetition_penalty=0.0)
    with pytest.raises(ValueError):
        sess.submit(0, PROMPTS[0], logit_bias={V: 1.0})
    with pytest.raises(ValueError):
        sess.submit(0, PROMPTS[0], logit_bias={i: 1.0 for i in range(17)})           # more than session(max_logit_bias=16) holds
    with pytest.raises(ValueError):
        sess.submit(0, PROMPTS[0][:-1] + [V])                                          # a prompt token outside the vocabulary
    assert not any(sess.active()) and not bool(sess.hist[0].any())                   # refused before anything was touched
    s64 = dec.session(penalties=True, max_logit_bias=64)
    assert s64.bias_id.shape == (4, 64) and dec.session(penalties=True, max_logit_bias=0).bias_val.shape == (4, 0)
    with pytest.raises(ValueError):
        dec.session(penalties=True, max_logit_bias=65)


# ------------------------------------------------------------------------------------------------ 4. bans and forced tokens
def test_banned_tokens_stay_out_and_a_large_bias_forces_its_token(dec128, monkeypatch):
    dec = dec128
    plain = dec.session()
    plain.submit(0, PROMPTS[0], max_new_tokens=10)
    plain.run()
    emitted = plain.result(0)[0].tolist()
    sess = dec.session(penalties=True)
    sess.submit(0, PROMPTS[0], max_new_tokens=10, logit_bias={i: -math.inf for i in set(emitted)})
    sess.run()
    got = sess.result(0)[0].tolist()
    assert len(got) == 10 and not set(got) & set(emitted)
    # +100 on one token: the restatement's row has its maximum there whenever every raw logit is below 100 in magnitude -- checked per step on the
    # logits the launch was given, not assumed
    rec = Recorder(monkeypatch)
    sess.submit(2, PROMPTS[2], max_new_tokens=8, logit_bias={77: 100.0})
    sess.run(use_graph=False)
    rows = [rec.check_first(rec.first[-1])[0]] + [rec.check_step(r)[2] for r in rec.steps]
    raws = [rec.first[-1]["logits"][0]] + [r["logits"][2] for r in rec.steps]
    # (the 8th token is emitted by the 7th step: 1 admission + 7 steps)
    assert len(rows) == 8
    for row, raw in zip(rows, raws):
        assert float(raw.float().abs().max()) < 50.0                     # so l[77] + 100 > 50 > every other element, in fp16 too
        assert int(torch.argmax(row.float())) == 77
    assert sess.result(2)[0].tolist() == [77] * 8 and sess.result(2)[1] == 2


# ------------------------------------------------------------------------------------------------ 5. extend, load_tenant, log-probabilities
def test_extend_folds_the_history_and_load_tenant_clears_it(dec128):
    dec = dec128
    sess = dec.session(penalties=True)
    turn1 = _request(sess, [1, 2], mx=8)
    new = _toks(5, 9)
    sess.extend(1, new, max_new_tokens=6, **PEN[0])
    # right after the admission: bit 15 at the whole conversation so far (the last emitted token is part of the chunk), no counts yet
    assert _history_is(sess, 1, PROMPTS[1] + turn1[1][0] + new, [])
    sess.run()
    toks = sess.result(1)[0].tolist()
    assert len(toks) == 6 and _history_is(sess, 1, PROMPTS[1] + turn1[1][0] + new, toks[:-1])
    assert torch.equal(sess.hist[2].cpu(), turn1[2][2])                  # the other tenant keeps its own
    assert sess.pen[1].tolist() == pytest.approx([1.3, 1 / 1.3, 0.5, 0.25]) and sess.bias_id[1, :4].tolist() == [5, 17, 300, -1]
    assert sess.pen[1, 1].item() == torch.tensor(1.0 / 1.3, dtype=torch.float32).item()                  # the fp64 quotient, rounded once
    sess.load_tenant(1, {k: v for k, v in dec.tenant_state(1).items()})
    assert not bool(sess.hist[1].any()) and sess.pen[1].tolist() == [1.0, 1.0, 0.0, 0.0]
    assert bool((sess.bias_id[1] == -1).all()) and not bool(sess.bias_val[1].any())
    assert torch.equal(sess.hist[2].cpu(), turn1[2][2]) and sess.pen[2].tolist() != [1.0, 1.0, 0.0, 0.0]
    with pytest.raises(RuntimeError):
        sess.extend(1, new)                                              # nothing to extend any more
    again = _request(sess, [1], mx=8)[1]                                 # the same fine-tune, the same request: the first turn again
    assert _same(again, turn1[1])


def test_log_probabilities_are_the_raw_logits(dec128, monkeypatch):
    from bitdelta_amd import serving_ops as ops
    dec, K = dec128, 5
    plain = dec.session()
    plain.submit(0, PROMPTS[0], max_new_tokens=8)
    plain.run()
    ban = {i: -math.inf for i in set(plain.result(0)[0].tolist())}
    rec = Recorder(monkeypatch)
    sess = dec.session(logprobs=K, penalties=True)
    sess.submit(0, PROMPTS[0], max_new_tokens=8, repetition_penalty=1.2, logit_bias=ban)
    sess.run(use_graph=False)
    toks = sess.result(0)[0]
    raws = [rec.first[-1]["logits"][0]] + [r["logits"][0] for r in rec.steps]
    assert toks.numel() == 8 and len(raws) == 8                          # 1 admission + 7 steps
    lp, ids, lps = sess.result_logprobs(0)
    w_lp, w_ids, w_lps = ops.token_logprobs(torch.stack(raws).cuda(), toks.cuda(), K)
    assert torch.equal(lp.view(torch.int32), w_lp.cpu().view(torch.int32)) and torch.equal(ids, w_ids.cpu())
    assert torch.equal(lps.view(torch.int32), w_lps.cpu().view(torch.int32))
    # the lists are the model's own: they still hold banned tokens (the plain run's choices head them), which the request never emitted
    assert not set(toks.tolist()) & set(ban) and set(ids[:, 0].tolist()) & set(ban)
    graph = dec.session(logprobs=K, penalties=True)
    graph.submit(0, PROMPTS[0], max_new_tokens=8, repetition_penalty=1.2, logit_bias=ban)
    graph.run()
    assert torch.equal(graph.result(0)[0], toks) and all(torch.equal(a, b) for a, b in zip(graph.result_logprobs(0)[1:2], [ids]))
    assert torch.equal(graph.result_logprobs(0)[0].view(torch.int32), lp.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 6. retirement, and a plain session
def test_a_penalised_tenant_retires_for_the_right_reason(dec128):
    dec = dec128
    sess = dec.session(penalties=True)
    toks = _request(sess, [0], mx=12)[0]
    assert toks[1] == 2 and len(toks[0]) == 12                           # max_new_tokens
    stop = toks[0][4]
    cut = toks[0].index(stop) + 1
    sess.submit(0, PROMPTS[0], max_new_tokens=12, stop_token_ids=[stop], **PEN[0])
    sess.run()
    assert sess.result(0)[1] & 1 and sess.result(0)[0].tolist() == toks[0][:cut]        # its stop token, chosen under the penalties
    assert _history_is(sess, 0, PROMPTS[0], toks[0][:cut - 1])
    from bitdelta_amd.serving_loop import TenantDecoder
    small = TenantDecoder.synthetic("tiny128", 2, "cuda", dtype=torch.float16, seed=3, max_len=72)
    s2 = small.session(penalties=True)
    s2.submit(1, PROMPTS[0], max_new_tokens=50, **PEN[0])                # 64 padded rows + 8 more: the cache is full first
    s2.run()
    assert s2.result(1)[1] == 4 and s2.result(1)[0].numel() == 9 and int(s2.pos[1]) == 72
    assert not bool(s2.hist[0].any())                                    # the idle slot was not touched
    s2.submit(0, PROMPTS[2], max_new_tokens=1, **PEN[1])                 # retired by its first token: nothing was fed back
    assert not any(s2.active()) and s2.result(0)[1] == 2 and _history_is(s2, 0, PROMPTS[2], [])


def test_a_session_without_penalties_has_none_of_it(dec128):
    dec = dec128
    for plain in (dec.session(), dec.session(sampling=True), dec.session(logprobs=3)):
        assert plain.penalties is False
        assert not any(hasattr(plain, a) for a in ("hist", "pen", "bias_id", "bias_val", "plogits"))
        for bad in (dict(repetition_penalty=1.1), dict(presence_penalty=0.5), dict(frequency_penalty=-0.5), dict(logit_bias={3: 1.0})):
            with pytest.raises(ValueError, match="penalties=True"):
                plain.submit(0, PROMPTS[0], **bad)
            with pytest.raises(ValueError, match="penalties=True"):
                plain.submit_all(PROMPTS, **bad)
        with pytest.raises(ValueError):
            plain.submit(0, PROMPTS[0], repetition_penalty=-1.0)         # an invalid value is refused as such
        assert not any(plain.active())
    a, b = dec.session(), dec.session()
    a.submit_all(PROMPTS, max_new_tokens=8)
    b.submit_all(PROMPTS, max_new_tokens=8, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias={})       # neutral values pass
    a.run()
    b.run()
    assert _results(a) == _results(b) and len(a._graphs) == 1
