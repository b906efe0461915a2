"""GPU tests of per-token log-probabilities in a TenantSession (serving_loop.py, session(logprobs=k)) on the two-layer synthetic decoder tiny128:
the tokens are the plain session's; every reported entry is the restatement's (tests/logprobs_ref.py) on the logits of the step that emitted its
token; a greedy token heads its own list; graph replay, the other tenants and the order of admission do not change a tenant's entries; extend
restarts them, load_tenant clears them, a tenant that retires for any reason has its last token's entry; a plain session has none."""
import numpy as np
import pytest
import torch

import logprobs_ref as ref

pytestmark = pytest.mark.gpu

K = 5
PARAMS = [dict(temperature=1.0, top_k=0, top_p=1.0, seed=2 ** 63 + 17), dict(temperature=0.7, top_k=20, top_p=0.9, seed=11),
          dict(temperature=0.0, top_k=0, top_p=1.0, seed=0), dict(temperature=1.5, top_k=0, top_p=0.8, seed=2 ** 64 - 1)]


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


def _poison(sess):
    """entries nobody wrote are recognisable: NaN / -9"""
    sess.lp.fill_(float("nan"))
    sess.top_lp.fill_(float("nan"))
    sess.top_id.fill_(-9)


def _bits(t):
    return t.contiguous().view(torch.int32).numpy()


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) if x.dtype == torch.float32 else torch.equal(x, y) for x, y in zip(a, b))


def _complete(sess, t, k=K, greedy=True):
    """tenant t's entries cover exactly result(t)'s tokens, every one was written, and a greedy token heads its own list"""
    toks = sess.result(t)[0]
    lp, ids, lps = sess.result_logprobs(t)
    n = toks.numel()
    assert lp.shape == (n,) and ids.shape == (n, k) and lps.shape == (n, k) and lp.dtype == lps.dtype == torch.float32 and ids.dtype == torch.int32
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(lps).all()) and bool(((ids >= 0) & (ids < 512)).all()), t
    if k:
        assert bool((lps[:, :-1] >= lps[:, 1:]).all()) and bool((lp <= lps[:, 0]).all())
        if greedy:
            assert ids[:, 0].tolist() == toks.tolist() and np.array_equal(_bits(lps[:, 0]), _bits(lp)), t
    return lp, ids, lps


# ------------------------------------------------------------------------------------------------ 1. the tokens are unchanged
def test_a_logprob_session_emits_the_plain_sessions_tokens(dec128):
    dec = dec128
    runs = []
    for sess in (dec.session(), dec.session(logprobs=K), dec.session(logprobs=0)):
        sess.submit_all(PROMPTS, max_new_tokens=12, stop_token_ids=[[], [3], [], [5]])
        sess.run()
        first = _results(sess)
        for t in (2, 0):
            sess.submit(t, PROMPTS[t], max_new_tokens=5)
        sess.run()
        sess.extend(0, _toks(7, 3), max_new_tokens=4)
        sess.run()
        runs.append((first, _results(sess)))
        if sess.logprobs is not None:
            for t in range(4):
                _complete(sess, t, k=sess.logprobs)
    assert runs[0] == runs[1] == runs[2]
    greedy = runs[0][0]
    runs = []
    for sess in (dec.session(sampling=True), dec.session(sampling=True, logprobs=K)):
        sess.submit_all(PROMPTS, max_new_tokens=10, **{q: [P[q] for P in PARAMS] for q in PARAMS[0]})
        sess.run()
        runs.append(_results(sess))
    assert runs[0] == runs[1] and runs[0][0][0][:10] != greedy[0][0][:10]              # (tau = 1 on 512 near-flat logits: not the argmax path)
    for t in range(4):
        _complete(sess, t, greedy=t == 2)                                # tenant 2 samples at temperature 0


# ------------------------------------------------------------------------------------------------ 2. every entry against the restatement
@pytest.mark.parametrize("sampling", [False, True], ids=["greedy", "sampling"])
def test_every_entry_is_the_restatements(dec128, monkeypatch, sampling):
    """eager steps with step_logprobs and token_logprobs wrapped to keep the logits they were given: entry [t, j] is the restatement's answer on the
    logits of the step that emitted token j of tenant t -- the first token after submit and after extend from the prefill's logits"""
    from bitdelta_amd import serving_ops as ops
    dec = dec128
    first, steps = [], []
    orig_rows, orig_step = ops.token_logprobs, ops.step_logprobs

    def rows(logits, tokens, top_n, out=None):
        first.append((logits.clone(), tokens.tolist()))
        return orig_rows(logits, tokens, top_n, out)

    def step(logits, tok, n, lp_n, lp, top_id, top_lp):
        before = lp_n.tolist()
        orig_step(logits, tok, n, lp_n, lp, top_id, top_lp)
        assert lp_n.tolist() == n.tolist()
        steps.append((logits.clone(), before, n.tolist(), tok[:, 0].tolist()))
    monkeypatch.setattr(ops, "token_logprobs", rows)
    monkeypatch.setattr(ops, "step_logprobs", step)
    par = (lambda t: PARAMS[t]) if sampling else (lambda t: {})
    sess = dec.session(sampling=sampling, logprobs=K)
    _poison(sess)
    records = {t: [] for t in range(4)}                                  # tenant -> [(logits row bits, token)], one per emitted token of its current turn

    def admit(t):
        lg, toks = first[-1]
        assert len(toks) == 1
        records[t] = [(lg[0].cpu().view(torch.int16).numpy().view(np.uint16), toks[0])]

    def run(k):
        for _ in range(k):
            if not any(sess.active()):
                break
            sess.step(1, use_graph=False)
            lg, before, after, tok = steps[-1]
            for t in range(4):
                if after[t] != before[t]:
                    assert after[t] == before[t] + 1
                    records[t].append((lg[t].cpu().view(torch.int16).numpy().view(np.uint16), tok[t]))
    sess.submit(0, PROMPTS[0], max_new_tokens=12, **par(0)); admit(0)   # three tenants, three prompt lengths, admitted at different steps
    run(2)
    sess.submit(1, PROMPTS[1], max_new_tokens=3, **par(1)); admit(1)    # retires early
    run(3)
    sess.submit(2, PROMPTS[2], max_new_tokens=9, **par(2)); admit(2)
    run(40)
    assert not any(sess.active()) and [sess.result(t)[0].numel() for t in range(4)] == [12, 3, 9, 0]
    sess.extend(1, _toks(6, 8), max_new_tokens=4, **par(1)); admit(1)   # the entries restart with the turn
    run(40)
    assert sess.result(1)[0].numel() == 4 and len(steps) <= 24
    for t in range(3):
        toks = sess.result(t)[0].tolist()
        lp, ids, lps = _complete(sess, t, greedy=not sampling)
        assert [r[1] for r in records[t]] == toks, t
        for j, (bits, tok) in enumerate(records[t]):
            w_lp, w_ids, w_lps = ref.row_logprobs(ref.values(bits, "float16"), tok, K)
            assert ids[j].tolist() == w_ids.tolist(), (t, j)
            assert ref.within([float(lp[j])], [w_lp]).all() and ref.within(lps[j].numpy(), w_lps).all(), (t, j)
    # tenant 3 was never admitted: nothing of it was written; nor anything past a tenant's tokens in this turn or the longest one before it
    assert bool(torch.isnan(sess.lp[3]).all()) and bool((sess.top_id[3] == -9).all()) and bool(torch.isnan(sess.top_lp[3]).all()) and int(sess.lp_n[3]) == 0
    assert bool(torch.isnan(sess.lp[0, 12:]).all()) and bool((sess.top_id[1, 4:] == -9).all()) and bool(torch.isnan(sess.top_lp[2, 9:]).all())


# ------------------------------------------------------------------------------------------------ 3. graph / eager, independence
def _request(sess, ts, use_graph=True, mx=10, params=None):
    _poison(sess)
    for t in ts:
        sess.submit(t, PROMPTS[t], max_new_tokens=mx, **(params[t] if params else {}))
    sess.run(use_graph=use_graph)
    return {t: (sess.result(t)[0],) + sess.result_logprobs(t) for t in ts}


@pytest.mark.parametrize("sampling", [False, True], ids=["greedy", "sampling"])
def test_graph_equals_eager_and_entries_do_not_depend_on_the_other_tenants(dec128, sampling):
    dec = dec128
    params = PARAMS if sampling else None
    sess = dec.session(sampling=sampling, logprobs=K)
    eager = _request(sess, range(4), use_graph=False, params=params)
    graph = _request(sess, range(4), use_graph=True, params=params)
    again = _request(sess, range(4), use_graph=True, params=params)
    for t in range(4):
        assert _same(eager[t], graph[t]) and _same(graph[t], again[t]) and graph[t][0].numel() == 10, t
        _complete(sess, t, greedy=not sampling or t == 2)
    assert len(sess._graphs) == 1
    for t in range(4):                                                   # alone
        assert _same(_request(sess, [t], params=params)[t], graph[t]), t
    _poison(sess)                                                        # admitted while others are mid-generation
    p = params or [{}] * 4
    sess.submit(0, PROMPTS[0], max_new_tokens=10, **p[0])
    sess.step(3)
    sess.submit(3, PROMPTS[3], max_new_tokens=10, **p[3])
    sess.step(2)
    sess.submit(2, PROMPTS[2], max_new_tokens=10, **p[2])
    sess.run()
    for t in (0, 2, 3):
        assert _same((sess.result(t)[0],) + sess.result_logprobs(t), graph[t]), t
    assert len(sess._graphs) == 1
    # the count is part of the graph's key: a session with another count captures its own step and reports the same leading entries
    s20 = dec.session(sampling=sampling, logprobs=20)
    got = _request(s20, [1], params=params)[1]
    assert torch.equal(got[0], graph[1][0]) and np.array_equal(_bits(got[1]), _bits(graph[1][1]))
    assert torch.equal(got[2][:, :K], graph[1][2]) and np.array_equal(_bits(got[3][:, :K]), _bits(graph[1][3]))
    _complete(s20, 1, k=20, greedy=not sampling)


# ------------------------------------------------------------------------------------------------ 4. extend, load_tenant, retirement, refusals
def test_extend_restarts_and_load_tenant_clears_the_entries(dec128):
    dec = dec128
    sess = dec.session(logprobs=K)
    turn1 = _request(sess, [1, 2], mx=8)
    sess.extend(1, _toks(5, 9), max_new_tokens=3)
    sess.run()
    lp, ids, lps = _complete(sess, 1)
    assert lp.numel() == 3 and int(sess.lp_n[1]) == 3 and sess.result(1)[0].tolist() == ids[:, 0].tolist()
    assert _same((sess.result(2)[0],) + sess.result_logprobs(2), turn1[2])         # the other tenant keeps its own
    sess.load_tenant(1, {k: v for k, v in dec.tenant_state(1).items()})
    assert int(sess.lp_n[1]) == 0 and int(sess.n[1]) == 0
    assert [x.shape for x in sess.result_logprobs(1)] == [(0,), (0, K), (0, K)]
    assert _same((sess.result(2)[0],) + sess.result_logprobs(2), turn1[2])
    sess.submit(1, PROMPTS[1], max_new_tokens=8)                                   # the same fine-tune again: the first turn's entries
    sess.run()
    assert _same((sess.result(1)[0],) + sess.result_logprobs(1), turn1[1])


def test_a_retiring_tenant_has_its_last_tokens_entry(dec128):
    dec = dec128
    sess = dec.session(logprobs=K)
    got = _request(sess, [0], mx=12)[0]
    assert sess.result(0)[1] == 2 and got[0].numel() == 12                         # max_new_tokens
    _complete(sess, 0)
    stop = got[0].tolist()[4]
    cut = got[0].tolist().index(stop) + 1
    _poison(sess)
    sess.submit(0, PROMPTS[0], max_new_tokens=12, stop_token_ids=[stop])
    sess.run()
    assert sess.result(0)[1] & 1 and sess.result(0)[0].tolist() == got[0].tolist()[:cut]     # its stop token
    assert _same(_complete(sess, 0), [x[:cut] for x in got[1:]])
    from bitdelta_amd.serving_loop import TenantDecoder
    small = TenantDecoder.synthetic("tiny128", 2, "cuda", dtype=torch.float16, seed=3, max_len=72)
    s2 = small.session(logprobs=K)
    _poison(s2)
    s2.submit(1, PROMPTS[0], max_new_tokens=50)                                    # 64 padded rows + 8 more: the cache is full first
    s2.run()
    assert s2.result(1)[1] == 4 and s2.result(1)[0].numel() == 9 and int(s2.lp_n[1]) == 9
    _complete(s2, 1)
    assert bool(torch.isnan(s2.lp[0]).all()) and int(s2.lp_n[0]) == 0              # the idle slot was not touched
    s2.submit(0, PROMPTS[2], max_new_tokens=1)                                     # retired by its first token: the prefill's entry alone
    assert not any(s2.active()) and s2.result(0)[1] == 2
    assert _complete(s2, 0)[0].numel() == 1


def test_argument_and_a_plain_session(dec128):
    dec = dec128
    plain = dec.session()
    assert plain.logprobs is None and not hasattr(plain, "lp_n")
    with pytest.raises(ValueError, match="logprobs"):
        plain.result_logprobs(0)
    for bad in (-1, 21, True, 2.5):
        with pytest.raises(ValueError):
            dec.session(logprobs=bad)
    assert dec.session(logprobs=20).top_id.shape == (4, 256, 20) and dec.session(logprobs=0).top_lp.shape == (4, 256, 0)
