"""GPU tests of the tail truncation in a TenantSession (serving_loop.py, session(sampling=True, truncation=True)) on a two-layer synthetic
decoder, V = 512, 24-token turns.  The step's rows are taken where the launch sees them: serving_ops.step_truncate / truncate_rows are wrapped
to remember their input tensor (under graph replay the graph's own static buffer) and the session's tlogits holds the output, so after every
single step the test has, per tenant, the row the launch received and the row it wrote.  Each such pair is judged by the acceptance rule of
tests/truncation_ref.py, and the token the step emitted must be a kept element of the written row.  A FREE run in a session made without
the feature comes first.  The power of these tests: the rows are the model's, not crafted, so -- unlike the kernel tests, which assert it
for every row -- a test here cannot demand that the reference cuts EVERY row to more than one and fewer than all finite elements; each test
counts the steps on which it does and asserts a floor (8 of a tenant's 23 steps where three filters run side by side, 4 where one request
runs alone), and prints the counts."""
import numpy as np
import pytest
import torch

import truncation_ref as ref

pytestmark = pytest.mark.gpu

V = 512
N = 24                       # tokens of a turn
SAMPLING = [dict(temperature=1.0, top_k=0, top_p=1.0, seed=2 ** 63 + 17), dict(temperature=0.7, top_k=20, top_p=0.9, seed=11),
            dict(temperature=1.5, top_k=0, top_p=1.0, seed=5), dict(temperature=0.9, top_k=50, top_p=0.8, seed=2 ** 64 - 1)]
TRUNC = [dict(min_p=0.1), dict(typical_p=0.8), dict(epsilon_cutoff=3e-3, eta_cutoff=0.02), dict()]      # tenant 3 stays neutral
NAMES = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


def _prm(kw):
    d = dict(dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0), **kw)
    return tuple(d[k] for k in NAMES)


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


def _results(sess):
    return [(sess.result(t)[0].tolist(), sess.result(t)[1]) for t in range(sess.T)]


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def free(dec128):
    """greedy and sampled free runs in sessions made WITHOUT the feature, run once, never modified: {kind: [(tokens, reason)] * 4}"""
    res = {}
    for kind in ("greedy", "sampling"):
        sess = dec128.session(sampling=kind == "sampling", logprobs=5)
        for t in range(4):
            sess.submit(t, PROMPTS[t], max_new_tokens=N, **(SAMPLING[t] if kind == "sampling" else {}))
        sess.run()
        res[kind] = _results(sess)
        assert all(len(y) == N and r == 2 for y, r in res[kind])
    return res


class _Spy:
    """remembers the tensors the two truncation launches were given: .step = (logits, out) of the last step_truncate call -- under graph
    replay the captured call's, i.e. the graph's static buffers -- and .rows = [(logits, tau, params, out)] of every truncate_rows call"""

    def __init__(self, monkeypatch):
        from bitdelta_amd import serving_ops as ops
        self.step, self.rows = None, []
        step, rows = ops.step_truncate, ops.truncate_rows

        def step_truncate(logits, out, tau, params, active):
            self.step = (logits, out)
            return step(logits, out, tau, params, active)

        def truncate_rows(logits, tau, params, out=None):
            got = rows(logits, tau, params, out=out)
            self.rows.append((logits, tau, params, got))
            return got
        monkeypatch.setattr(ops, "step_truncate", step_truncate)
        monkeypatch.setattr(ops, "truncate_rows", truncate_rows)


def _judge_first(spy, sess, t, tau, prm):
    """the rows form at admission: the last truncate_rows call is tenant t's; its token is a kept element of an accepted row"""
    logits, tau_d, prm_d, out = spy.rows[-1]
    assert logits.shape == (1, V) and abs(float(tau_d[0]) - tau) < 1e-6 and prm_d.tolist() == [list(np.float32(prm).tolist())]
    exact = ref.check_row(_bits(logits)[0], "float16", tau, prm, _bits(out)[0])
    first = sess.result(t)[0].tolist()[0]
    assert _bits(out)[0][first] != ref.NINF["float16"], (t, first)
    return exact


def _run_judged(sess, spy, mode, reqs):
    """step until nobody is active, one step at a time, and judge every active tenant's row of every step.  reqs: {t: (tau, prm)}.
    Returns {t: [rows judged, rows exactly the reference's, rows on which the reference keeps more than one and fewer than all finite]}"""
    stats = {t: [0, 0, 0] for t in reqs}
    while True:
        act = sess.active()
        if not any(act):
            break
        n0 = sess.n.tolist()
        sess.step(1, use_graph=mode == "graph")
        torch.cuda.synchronize()
        logits, out = spy.step
        assert out.data_ptr() == sess.tlogits.data_ptr()
        ib, ob, n1 = _bits(logits), _bits(out), sess.n.tolist()
        for t, (tau, prm) in reqs.items():
            if not act[t]:
                assert n1[t] == n0[t]
                continue
            assert n1[t] == n0[t] + 1
            tok = int(sess.out[t, n0[t]])
            stats[t][1] += ref.check_row(ib[t], "float16", tau, prm, ob[t])
            stats[t][0] += 1
            stats[t][2] += ref.is_informative(ib[t], "float16", tau, prm)
            assert ob[t][tok] != ref.NINF["float16"], (t, n0[t], tok)    # the emitted token is a kept element
    return stats


# ------------------------------------------------------------------------------------------------ 1. every token obeys the rule
@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_every_token_lies_in_a_set_the_rule_accepts_and_the_neutral_tenant_notices_nothing(dec128, free, monkeypatch, mode):
    spy = _Spy(monkeypatch)
    sess = dec128.session(sampling=True, logprobs=5, truncation=True)
    reqs, first_exact = {}, 0
    for t in range(4):
        sess.submit(t, PROMPTS[t], max_new_tokens=N, **SAMPLING[t], **TRUNC[t])
        reqs[t] = (SAMPLING[t]["temperature"], _prm(TRUNC[t]))
        first_exact += _judge_first(spy, sess, t, *reqs[t])              # the first token at admission obeys the rule
        assert sess.trunc[t].tolist() == np.float32(reqs[t][1]).tolist()
    stats = _run_judged(sess, spy, mode, reqs)
    got = _results(sess)
    assert got[3] == free["sampling"][3]                                 # neutral parameters: the plain sampling session's tokens, bit for bit
    assert all(len(y) == N and r == 2 for y, r in got)
    for t in (0, 1, 2):
        assert stats[t][0] == N - 1 and stats[t][2] >= 8, (t, stats[t])  # the power of the test: the reference cuts most of these rows
    assert any(got[t] != free["sampling"][t] for t in (0, 1, 2))         # ... and the cut changes what is sampled
    print("%s: first tokens %d of 4 exact; per tenant [judged, exact, informative]: %s" % (mode, first_exact, stats))
    if mode == "graph":
        (key,) = sess._graphs
        assert key[-1] == "truncation" and len(key) == 11


def test_min_p_one_reproduces_the_greedy_session(dec128, free, monkeypatch):
    spy = _Spy(monkeypatch)
    sess = dec128.session(sampling=True, truncation=True)
    for t in range(4):
        sess.submit(t, PROMPTS[t], max_new_tokens=N, temperature=1.0, seed=1000 + t, min_p=1.0)
    rows = {t: [_bits(spy.rows[t][0])[0]] for t in range(4)}             # per tenant: the row each token was chosen from
    while any(sess.active()):
        sess.step(1)
        torch.cuda.synchronize()
        ib = _bits(spy.step[0])
        for t in range(4):
            if len(rows[t]) < int(sess.n[t]):
                rows[t].append(ib[t])
    compared = 0
    for t in range(4):
        y, want = sess.result(t)[0].tolist(), free["greedy"][t][0]
        assert len(y) == N == len(rows[t])
        for j in range(N):
            l = ref.values(rows[t][j], "float16")
            top = np.sort(l[np.isfinite(l)])[::-1]
            delta = 1e-4 * max(1.0, float(top[0] - top[-1]))             # tau = 1: x = l - m
            if not top[0] - top[1] > delta:                              # an undecided step: the trajectories may part here
                break
            assert y[j] == int(np.argmax(l)) == want[j], (t, j)
            compared += 1
    print("min_p = 1: %d of %d steps decided and equal to the greedy session's" % (compared, 4 * N))
    assert compared >= 3 * N


# ------------------------------------------------------------------------------------------------ 2. one capture, extend, load_tenant
def test_parameters_change_between_requests_on_one_capture(dec128, free, monkeypatch):
    spy = _Spy(monkeypatch)
    sess = dec128.session(sampling=True, truncation=True)
    seen = []
    for kw in (dict(min_p=0.2), dict(typical_p=0.5), dict(), dict(epsilon_cutoff=3e-3), dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=0.01)):
        sess.submit(2, PROMPTS[2], max_new_tokens=N, **SAMPLING[2], **kw)
        req = (SAMPLING[2]["temperature"], _prm(kw))
        _judge_first(spy, sess, 2, *req)
        st = _run_judged(sess, spy, "graph", {2: req})
        seen.append(_results(sess)[2])
        if not kw:
            assert seen[-1] == free["sampling"][2]
        else:
            assert st[2][2] >= 4, (kw, st)
        assert len(sess._graphs) == 1
    assert len({tuple(y) for y, _ in seen}) >= 3                         # the parameters matter
    # the refusals come before anything is touched
    names = ("trunc", "n", "done", "out", "temperature")
    before = [getattr(sess, k).clone() for k in names] + [c.clone() for c in sess.cache["k"] + sess.cache["v"]]
    for bad in (dict(min_p=1.5), dict(min_p=-0.1), dict(typical_p=0.0), dict(typical_p=float("nan")), dict(epsilon_cutoff=1.0), dict(eta_cutoff=-1e-3),
                dict(eta_cutoff=float("inf")), dict(min_p=True)):
        with pytest.raises(ValueError):
            sess.submit(2, PROMPTS[2], **bad)
        with pytest.raises(ValueError):
            sess.extend(2, [5], **bad)
    with pytest.raises(ValueError):
        sess.submit_all(PROMPTS, temperature=1.0, min_p=[0.0, 0.0, 1.5, 0.0])
    with pytest.raises(ValueError, match="for 4 tenants"):
        sess.submit_all(PROMPTS, temperature=1.0, typical_p=[0.5, 0.5])
    after = [getattr(sess, k) for k in names] + sess.cache["k"] + sess.cache["v"]
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and not any(sess.active())
    # submit_all: one value for all or one per tenant
    sess.submit_all(PROMPTS, max_new_tokens=4, temperature=1.0, seed=3, min_p=[0.0, 0.1, 0.0, 1.0], typical_p=0.9, eta_cutoff=[0.0, 0.0, 0.01, 0.0])
    assert sess.trunc.tolist() == np.float32([[0.0, 0.9, 0.0, 0.0], [0.1, 0.9, 0.0, 0.0], [0.0, 0.9, 0.0, 0.01], [1.0, 0.9, 0.0, 0.0]]).tolist()
    assert spy.rows[-1][0].shape == (4, V) and torch.equal(spy.rows[-1][2], sess.trunc)
    sess.run()
    assert len(sess._graphs) == 1


def test_extend_takes_the_turns_own_parameters_and_load_tenant_clears(dec128, monkeypatch):
    spy = _Spy(monkeypatch)
    dec, t = dec128, 1
    sess = dec.session(sampling=True, truncation=True)
    sess.submit(t, PROMPTS[t], max_new_tokens=12, **SAMPLING[t], min_p=0.3)
    sess.submit(2, PROMPTS[2], max_new_tokens=N, **SAMPLING[2], typical_p=0.7)
    sess.run()
    other = _results(sess)[2]
    assert sess.trunc[t].tolist() == np.float32([0.3, 1.0, 0.0, 0.0]).tolist()
    sess.extend(t, [7, 8, 9], max_new_tokens=12, **SAMPLING[t], typical_p=0.6, eta_cutoff=0.01)      # they replace the turn before's
    req = (SAMPLING[t]["temperature"], (0.0, 0.6, 0.0, 0.01))
    assert sess.trunc[t].tolist() == np.float32(req[1]).tolist() and sess.trunc[2].tolist() == np.float32([0.0, 0.7, 0.0, 0.0]).tolist()
    _judge_first(spy, sess, t, *req)
    st = _run_judged(sess, spy, "graph", {t: req})
    assert st[t][0] == 11 and st[t][2] >= 4 and _results(sess)[2] == other
    sess.extend(t, [], max_new_tokens=4, **SAMPLING[t])                   # a turn without them: neutral again
    assert sess.trunc[t].tolist() == list(ref.NEUTRAL)
    sess.run()
    # load_tenant clears the slot; the same fine-tune and request give the same turn again
    sess.submit(t, PROMPTS[t], max_new_tokens=N, **SAMPLING[t], min_p=0.2, typical_p=0.9)
    sess.run()
    first = _results(sess)[t]
    sess.load_tenant(t, {k: v for k, v in dec.tenant_state(t).items()})
    assert sess.trunc[t].tolist() == list(ref.NEUTRAL) and sess.trunc[2].tolist() == np.float32([0.0, 0.7, 0.0, 0.0]).tolist()
    sess.submit(t, PROMPTS[t], max_new_tokens=N, **SAMPLING[t], min_p=0.2, typical_p=0.9)
    sess.run()
    assert _results(sess)[t] == first


# ------------------------------------------------------------------------------------------------ 3. next to every other feature
def test_with_every_other_feature_the_launch_reads_the_banned_row_and_logprobs_stay_raw(dec128, monkeypatch):
    from bitdelta_amd.constraint import TokenAutomaton as TA
    spy = _Spy(monkeypatch)
    dec = dec128
    allowed_ids = list(range(64, 192, 3))
    allowed = TA.allowed_set(allowed_ids)
    kw = dict(sampling=True, logprobs=5, penalties=True, constraints=True, stop_sequences=True, bans=True)
    par = dict(SAMPLING[1], repetition_penalty=1.3, presence_penalty=0.5, logit_bias={70: 2.0}, constraint=allowed, stop_sequences=[[400, 401]])
    plain = dec.session(**kw)
    plain.submit(1, PROMPTS[1], max_new_tokens=16, **par)
    plain.run()
    y0 = _results(plain)[1][0]
    assert len(y0) == 16 and set(y0) <= set(allowed_ids)
    sess = dec.session(truncation=True, **kw)
    sess.submit(1, PROMPTS[1], max_new_tokens=16, bad_words=[[y0[0]]], min_p=0.05, typical_p=0.95, **par)
    logits, _, _, out = spy.rows[-1]                                     # admission: the rows form reads the banned row
    assert _bits(logits)[0][y0[0]] == ref.NINF["float16"] and _bits(out)[0][y0[0]] == ref.NINF["float16"]
    req = (SAMPLING[1]["temperature"], (0.05, 0.95, 0.0, 0.0))
    _judge_first(spy, sess, 1, *req)
    st = _run_judged(sess, spy, "graph", {1: req})
    assert spy.step[0].data_ptr() == sess.blogits.data_ptr()             # the step form reads the ban launch's output ...
    ib = _bits(spy.step[0])[1]
    assert ib[y0[0]] == ref.NINF["float16"] and int((ib != ref.NINF["float16"]).sum()) <= len(allowed_ids) - 1      # ... banned, constrained
    y = _results(sess)[1][0]
    assert set(y) <= set(allowed_ids) and y0[0] not in y and st[1][0] == len(y) - 1 and len(sess._graphs) == 1
    lp, ids, _ = sess.result_logprobs(1)                                 # the log-probabilities still describe the RAW row
    assert lp.shape == (len(y),) and torch.equal(ids[0], plain.result_logprobs(1)[1][0])
    assert any(int(i) not in allowed_ids for i in ids[0].tolist())       # (a masked row could not list them)
    (key,) = sess._graphs
    assert key[-1] == "truncation" and key[-4:-1] == ("bans", 16, 8)


# ------------------------------------------------------------------------------------------------ 4. a session made without the feature
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
    plain = dec.session(sampling=True, logprobs=5)
    assert plain.truncation is False and not any(hasattr(plain, n) for n in ("trunc", "tlogits"))
    for bad in (dict(min_p=0.05), dict(typical_p=0.9), dict(epsilon_cutoff=3e-4), dict(eta_cutoff=3e-4)):
        with pytest.raises(ValueError, match="truncation=True"):
            plain.submit(0, PROMPTS[0], temperature=1.0, **bad)
        with pytest.raises(ValueError, match="truncation=True"):
            plain.submit_all(PROMPTS, temperature=1.0, **bad)
    with pytest.raises(ValueError, match="truncation=True"):
        plain.submit_all(PROMPTS, temperature=1.0, min_p=[0.0, 0.0, 0.05, 0.0])
    assert not any(plain.active())
    del calls[:]
    for t in range(4):
        plain.submit(t, PROMPTS[t], max_new_tokens=N, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, **SAMPLING[t])   # neutral values are no request
    plain.step(1, use_graph=False)
    before = list(calls)
    assert "step_truncate" not in before
    plain.run()
    assert _results(plain) == free["sampling"]
    (key,) = plain._graphs
    assert len(key) == 10                                                # the key it had
    with_flag = dec.session(sampling=True, logprobs=5, truncation=True)
    assert with_flag.trunc.shape == (4, 4) and with_flag.tlogits.shape == (4, V)
    del calls[:]
    for t in range(4):
        with_flag.submit(t, PROMPTS[t], max_new_tokens=N, **SAMPLING[t])
    with_flag.step(1, use_graph=False)
    assert calls == ["step_begin_ragged", "step_truncate"] + before[1:]  # the same launches in the same order, and one more in front of the step end
    with_flag.run()
    assert _results(with_flag) == free["sampling"]                       # nothing cut: the free run bit for bit
    greedy = dec.session(logprobs=5)                                     # a greedy session takes neutral values only, and the flag not at all
    with pytest.raises(ValueError, match="truncation=True"):
        greedy.submit(0, PROMPTS[0], min_p=0.05)
    with pytest.raises(ValueError, match="sampling=True"):
        dec.session(truncation=True)
    with pytest.raises(ValueError, match="sampling=True"):
        dec.session(truncation=True, logprobs=5, bans=True)
