"""GPU tests of per-request sampling in a TenantSession (serving_loop.py, session(sampling=True)) on two-layer synthetic decoders: the sampling
session with greedy parameters is the plain session; step_end_sample is step_end_ragged's state transition with sample_rows' token; every emitted
token is the restatement's (tests/sampling_ref.py) for the logits the step saw; graph replay, the other tenants and the order of admission do not
change a tenant's tokens; parameters change between requests without a new capture; retirement reasons are unchanged."""
import numpy as np
import pytest
import torch

import sampling_ref as ref

pytestmark = pytest.mark.gpu

NAME = {torch.float16: "float16", torch.bfloat16: "bfloat16"}
BIG_SEED = 2 ** 63 + 2 ** 32 + 17


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


# ------------------------------------------------------------------------------------------------ 1. greedy parameters: the plain session
@pytest.mark.parametrize("name,T,dtype", [("tiny128", 4, torch.float16), ("tiny2048", 3, torch.bfloat16)])
def test_sampling_session_with_greedy_parameters_is_the_plain_session(name, T, dtype):
    from bitdelta_amd.serving_loop import TenantDecoder
    dec = TenantDecoder.synthetic(name, T, "cuda", dtype=dtype, seed=31, max_len=192, shared_heads=True)
    plain, samp = dec.session(), dec.session(sampling=True)
    for use_graph in (True, False):
        got = []
        for sess in (plain, samp):
            sess.submit_all(PROMPTS[:T], max_new_tokens=12, stop_token_ids=[[], [3], [], [5]][:T])
            sess.run(use_graph=use_graph)
            got.append(_results(sess))
        assert got[0] == got[1], use_graph
        assert all(len(toks) >= 1 and reason in (1, 2) for toks, reason in got[0])
    # one tenant at a time, another order, an extension: still the plain session's tokens
    got = []
    for sess in (plain, samp):
        for t in (2, 0):
            sess.submit(t, PROMPTS[t], max_new_tokens=5)
        sess.run()
        sess.extend(0, _toks(7, 3), max_new_tokens=4)
        sess.run()
        got.append(_results(sess))
    assert got[0] == got[1]


# ------------------------------------------------------------------------------------------------ 2. the step kernel
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_step_end_sample_is_step_end_ragged_with_the_sampled_token(dtype):
    from bitdelta_amd import serving_ops as ops
    dev, T, V, Lc, cap = "cuda", 8, 2056, 40, 6
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(T, V + 8, generator=g) * 3).to(dtype).to(dev)[:, :V]                 # a row stride > V
    STOP = int(torch.argmax(logits[1]))

    def state():
        return dict(tok=torch.full((T, 1), 9, dtype=torch.long, device=dev), out=torch.full((T, cap), -7, dtype=torch.long, device=dev),
                    n=torch.tensor([1, 2, 3, 1, 5, 7, 1, 2], device=dev), pos=torch.tensor([10, 11, Lc - 1, 13, 14, 15, 2 ** 33, 17], device=dev),
                    limit=torch.tensor([9, 9, 9, 2, 9, 9, 9, 9], device=dev), active=torch.tensor([1, 1, 1, 1, 0, 1, 1, 0], dtype=torch.bool, device=dev),
                    done=torch.zeros(T, dtype=torch.uint8, device=dev))
    stop_ids = torch.full((T, 2), -1, dtype=torch.long, device=dev)
    stop_ids[1, 1] = STOP
    z = lambda dt, v=0: torch.full((T,), v, dtype=dt, device=dev)
    a, b = state(), state()
    ops.step_end_ragged(logits, a["tok"], a["out"], a["n"], a["pos"], a["limit"], stop_ids, a["active"], a["done"], Lc)
    dbg = torch.full((T, 4), -77, dtype=torch.int32, device=dev)
    ops.step_end_sample(logits, b["tok"], b["out"], b["n"], b["pos"], b["limit"], stop_ids, b["active"], b["done"], Lc,
                        z(torch.float32), z(torch.int32, 5), z(torch.float32, 0.5), z(torch.long, 3), dbg)
    for k in a:
        assert torch.equal(a[k], b[k]), k                             # tau = 0: the same transition, inactive tenants (4, 7) untouched
    assert a["done"].tolist() == [0, 1, 4, 2, 0, 0, 4, 0] and a["active"].tolist() == [True, False, False, False, False, True, False, False]
    assert dbg[4].tolist() == [-77] * 4 and dbg[7].tolist() == [-77] * 4 and int(dbg[0, 3]) & 1
    # tau > 0: sample_rows' token with d = pos + 1, the same bookkeeping around it
    tau = torch.tensor([1.0, 0.25, 4.0, 1.0, 1.0, 0.0, 1.0, 1.0], device=dev)
    k_ = torch.tensor([0, 50, 0, 7, 0, 3, 2100, 0], dtype=torch.int32, device=dev)
    p_ = torch.tensor([1.0, 0.9, 0.5, 1.0, 1.0, 0.9, 0.9, 1.0], device=dev)
    seed = torch.tensor([1, 2 ** 40, -5, 7, 8, 9, 2 ** 62, 11], device=dev)
    c = state()
    dbg_rows = torch.zeros(T, 4, dtype=torch.int32, device=dev)
    want = ops.sample_rows(logits, tau, k_, p_, seed, c["pos"] + 1, dbg_rows)
    ops.step_end_sample(logits, c["tok"], c["out"], c["n"], c["pos"], c["limit"], stop_ids, c["active"], c["done"], Lc, tau, k_, p_, seed, dbg)
    s0 = state()
    for t in range(T):
        if not bool(s0["active"][t]):
            assert all(torch.equal(c[k][t], s0[k][t]) for k in c), t
            continue
        w = int(want[t])
        assert int(c["tok"][t, 0]) == w and dbg[t].tolist() == dbg_rows[t].tolist(), t
        n0 = int(s0["n"][t])
        assert c["out"][t].tolist() == [w if j == n0 else -7 for j in range(cap)], t
        assert int(c["n"][t]) == n0 + 1 and int(c["pos"][t]) == int(s0["pos"][t]) + 1
        reason = (1 if w in stop_ids[t].tolist() else 0) | (2 if n0 + 1 >= int(s0["limit"][t]) else 0) | (4 if int(s0["pos"][t]) + 1 >= Lc else 0)
        assert int(c["done"][t]) == reason and bool(c["active"][t]) == (reason == 0), t
    assert len({int(x) for x in want}) > 2                            # (not the argmax everywhere)


# ------------------------------------------------------------------------------------------------ 3. end to end against the restatement
PARAMS = [dict(temperature=1.0, top_k=0, top_p=1.0, seed=BIG_SEED), dict(temperature=0.7, top_k=20, top_p=0.9, seed=11),
          dict(temperature=0.0, top_k=0, top_p=1.0, seed=0), dict(temperature=1.5, top_k=0, top_p=0.8, seed=2 ** 64 - 1)]


def _i64(s):
    return s & (2 ** 64 - 1)


def _check_record(rec, dtype):
    """(bits [V], tau, k, p, seed, d, token): the token is the restatement's where the draw is decisive, one of its top two otherwise"""
    bits, tau, k, p, seed, d, tok = rec
    s = ref.sample(bits, NAME[dtype], tau, k, p, seed, d)
    if s["greedy"] or (s["filters_decisive"] and s["gap"] > s["delta"]):
        assert tok == s["token"], (tau, k, p, seed, d, tok, s["token"])
        return 0
    if s["filters_decisive"]:
        assert tok in (s["token"], s["second"]), (tau, k, p, seed, d, tok, s["token"], s["second"])
    return 1


def test_every_emitted_token_is_the_restatements(dec128, monkeypatch):
    """eager steps with step_end_sample and sample_rows wrapped to record the logits they were given: every recorded (logits, parameters, d) yields
    the emitted token -- the first token after submit (d = L) and after extend (d = P + n) included"""
    from bitdelta_amd import serving_ops as ops
    dec, dtype = dec128, torch.float16
    first, steps = [], []
    orig_rows, orig_step = ops.sample_rows, ops.step_end_sample

    def rows(logits, tau, k, p, seed, draw, dbg=None):
        tok = orig_rows(logits, tau, k, p, seed, draw, dbg)
        first.append((logits.clone(), tau.tolist(), k.tolist(), p.tolist(), seed.tolist(), draw.tolist(), tok.tolist()))
        return tok

    def step(logits, tok, out, n, pos, limit, stop_ids, active, done, Lc, tau, k, p, seed, dbg=None):
        before = (logits.clone(), active.tolist(), (pos + 1).tolist(), tau.tolist(), k.tolist(), p.tolist(), seed.tolist())
        orig_step(logits, tok, out, n, pos, limit, stop_ids, active, done, Lc, tau, k, p, seed, dbg)
        steps.append(before + (tok[:, 0].tolist(),))
    monkeypatch.setattr(ops, "sample_rows", rows)
    monkeypatch.setattr(ops, "step_end_sample", step)
    sess = dec.session(sampling=True)
    sess.submit_all(PROMPTS, max_new_tokens=8, **{q: [P[q] for P in PARAMS] for q in PARAMS[0]})
    assert first[-1][5] == [128] * 4                                  # d = L, the common padded length
    sess.run(use_graph=False)
    turn1 = _results(sess)
    sess.extend(1, _toks(6, 8), max_new_tokens=6, **PARAMS[3])
    assert first[-1][5] == [128 + 7 + 7]                              # d = P + n: 7 generated rows are cached, the chunk has 1 + 6 rows
    sess.submit(2, PROMPTS[0], max_new_tokens=6, **PARAMS[1])
    assert first[-1][5] == [64]
    sess.run(use_graph=False)
    recs, emitted = [], {t: [] for t in range(4)}
    for lg, tau, k, p, seed, d, tok in first:
        b = lg.cpu().view(torch.int16).numpy().view(np.uint16)
        recs += [(b[r], tau[r], k[r], p[r], _i64(seed[r]), d[r], tok[r]) for r in range(len(tok))]
    for lg, act, d, tau, k, p, seed, tok in steps:
        b = lg.cpu().view(torch.int16).numpy().view(np.uint16)
        recs += [(b[t], tau[t], k[t], p[t], _i64(seed[t]), d[t], tok[t]) for t in range(4) if act[t]]
    assert len(steps) <= 24 and len(recs) == sum(len(x[0]) for x in turn1) + sum(len(x[0]) for i, x in enumerate(_results(sess)) if i in (1, 2))
    soft = sum(_check_record(r, dtype) for r in recs)
    assert soft <= 0.05 * len(recs) + 1, (soft, len(recs))
    assert len({r[5] for r in recs if r[4] == _i64(PARAMS[3]["seed"])}) == 8 + 6          # tenant 3's seed: draws at 14 different rows, none reused


# ------------------------------------------------------------------------------------------------ 4. graph / eager, independence, seeds
def _run_request(sess, ts, use_graph=True, params=PARAMS, mx=10):
    for t in ts:
        sess.submit(t, PROMPTS[t], max_new_tokens=mx, **params[t])
    sess.run(use_graph=use_graph)
    return {t: sess.result(t) for t in ts}


def test_graph_equals_eager_and_tokens_do_not_depend_on_the_other_tenants(dec128):
    dec = dec128
    sess, plain = dec.session(sampling=True), dec.session()
    eager = _run_request(sess, range(4), use_graph=False)
    graph = _run_request(sess, range(4), use_graph=True)
    again = _run_request(sess, range(4), use_graph=True)
    for t in range(4):
        assert eager[t][0].tolist() == graph[t][0].tolist() == again[t][0].tolist() and eager[t][1] == graph[t][1] == 2, t
    assert len(sess._graphs) == 1
    # alone, and admitted while others are mid-generation: the same tokens
    for t in range(4):
        assert _run_request(sess, [t])[t][0].tolist() == graph[t][0].tolist(), t
    sess.submit(0, PROMPTS[0], max_new_tokens=10, **PARAMS[0])
    sess.step(3)
    sess.submit(3, PROMPTS[3], max_new_tokens=10, **PARAMS[3])
    sess.step(2)
    sess.submit(2, PROMPTS[2], max_new_tokens=10, **PARAMS[2])
    sess.run()
    for t in (0, 2, 3):
        assert sess.result(t)[0].tolist() == graph[t][0].tolist(), t
    # the greedy tenant (2) next to sampling tenants: its plain-session tokens
    assert _run_request(plain, [2], params=[{}] * 4)[2][0].tolist() == graph[2][0].tolist()
    assert graph[0][0].tolist() != _run_request(plain, [0], params=[{}] * 4)[0][0].tolist()      # (tau = 1 on 512 near-flat logits: not the argmax path)


def test_seeds_parameters_between_requests_and_load_tenant(dec128):
    dec = dec128
    sess = dec.session(sampling=True)
    one = dict(temperature=1.0, seed=5)
    a = _run_request(sess, [1], params=[one] * 4, mx=24)[1][0].tolist()
    graph = dict(sess._graphs)
    b = _run_request(sess, [1], params=[one] * 4, mx=24)[1][0].tolist()
    c = _run_request(sess, [1], params=[dict(temperature=1.0, seed=6)] * 4, mx=24)[1][0].tolist()
    d = _run_request(sess, [1], params=[dict(temperature=0.5, top_k=3, top_p=0.7, seed=2 ** 64 - 1)] * 4, mx=24)[1][0].tolist()
    e = _run_request(sess, [1], params=[{}] * 4, mx=24)[1][0].tolist()
    assert a == b and a != c and len(a) == 24                          # the same seed: the same tokens; two seeds differ within 24 tokens
    assert len(d) == 24 and e == _run_request(dec.session(), [1], params=[{}] * 4, mx=24)[1][0].tolist()
    assert dict(sess._graphs) == graph and len(graph) == 1             # new parameters, the same captured graph object
    assert sess.temperature.tolist() == [0.0, 0.0, 0.0, 0.0]
    # the device arrays hold what was submitted; load_tenant resets the slot to greedy
    sess.submit(1, PROMPTS[1], max_new_tokens=2, temperature=0.5, top_k=3, top_p=0.75, seed=2 ** 64 - 1)
    sess.run()
    assert (sess.temperature[1].item(), sess.top_k[1].item(), sess.top_p[1].item(), sess.seed[1].item()) == (0.5, 3, 0.75, -1)
    state = {k: v for k, v in dec.tenant_state(1).items()}
    sess.load_tenant(1, state)
    assert (sess.temperature[1].item(), sess.top_k[1].item(), sess.top_p[1].item(), sess.seed[1].item()) == (0.0, 0, 1.0, 0)
    # a plain session refuses the arguments before it touches anything
    plain = dec.session()
    with pytest.raises(ValueError, match="sampling=True"):
        plain.submit(0, PROMPTS[0], temperature=0.5)
    with pytest.raises(ValueError):
        sess.submit(0, PROMPTS[0], top_p=0.0)
    assert not any(plain.active()) and not any(sess.active())


def test_a_sampling_tenant_retires_for_the_right_reason(dec128):
    dec = dec128
    sess = dec.session(sampling=True)
    par = dict(temperature=1.0, top_k=0, top_p=1.0, seed=77)
    toks = _run_request(sess, [0], params=[par] * 4, mx=12)[0]
    assert toks[1] == 2 and toks[0].numel() == 12                      # max_new_tokens
    stop = toks[0].tolist()[4]
    cut = toks[0].tolist().index(stop) + 1
    sess.submit(0, PROMPTS[0], max_new_tokens=12, stop_token_ids=[stop], **par)
    sess.run()
    assert sess.result(0)[1] & 1 and sess.result(0)[0].tolist() == toks[0].tolist()[:cut]      # its stop token, sampled
    from bitdelta_amd.serving_loop import TenantDecoder
    small = TenantDecoder.synthetic("tiny128", 2, "cuda", dtype=torch.float16, seed=3, max_len=72)
    s2 = small.session(sampling=True)
    s2.submit(1, PROMPTS[0], max_new_tokens=50, **par)                 # 64 padded rows + 8 more: the cache is full first
    s2.run()
    assert s2.result(1)[1] == 4 and s2.result(1)[0].numel() == 9 and int(s2.pos[1]) == 72
