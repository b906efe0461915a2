"""GPU tests of the order in which a TenantSession (serving_loop.py) runs its per-feature stages, on a two-layer synthetic decoder, V = 512.
Every serving_ops launch a session can make is wrapped to record its name and its arguments, and the sequences below are what a session with
every feature on, and one with none, launched before the stages became one list: admission order, step order, which buffer each mask reads,
the graph key, the tensors a trial step puts back, what one admission leaves in the per-request arrays, and what load_tenant clears."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 512
ALL_ON = dict(sampling=True, logprobs=3, penalties=True, constraints=True, stop_sequences=True, bans=True, truncation=True)
ROWS = ("penalize_rows", "constrain_rows", "ban_rows", "truncate_rows", "sample_rows", "token_logprobs")
ADMISSION = ["penalize_rows", "constrain_rows", "ban_rows", "truncate_rows", "sample_rows", "token_logprobs"]
STEP = ["step_begin_ragged", "step_penalize", "step_constrain", "step_ban", "step_truncate", "step_end_sample", "step_logprobs",
        "step_constrain_advance", "step_stop_sequences"]
BASE_STATE = ("tok", "pos", "n", "limit", "active_flags", "done", "stop_ids", "out")      # then cache["valid"]
# every per-request array of an all-on session (the names are attributes of the session)
ARRAYS = ("stop_ids", "temperature", "top_k", "top_p", "seed", "lp_n", "hist", "pen", "bias_id", "bias_val", "c_state", "c_n", "ss_tok", "ss_len",
          "ss_n", "hit", "hold", "ctx_len", "ban_ngram", "ban_tok", "ban_len", "ban_min", "trunc", "n", "done", "out")


@pytest.fixture(scope="module")
def dec128():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib
    from bitdelta_amd.serving_loop import TenantDecoder
    _lib.lib()
    return TenantDecoder.synthetic("tiny128", 4, "cuda", dtype=torch.float16, max_len=256)


def _distinct(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randperm(499, generator=g)[:n] + 1).tolist()


PROMPTS = [_distinct(n, 80 + n) for n in (9, 64, 33, 70)]


@pytest.fixture
def calls(monkeypatch):
    """[(name, positional arguments, result)] of every step_* and rows launch, in call order"""
    from bitdelta_amd import serving_ops as ops
    seen = []
    for name in [n for n in dir(ops) if n.startswith("step_")] + list(ROWS):
        def wrap(fn, name):
            def f(*a, **k):
                got = fn(*a, **k)
                seen.append((name, a, got))
                return got
            return f
        monkeypatch.setattr(ops, name, wrap(getattr(ops, name), name))
    return seen


def _names(calls):
    return [c[0] for c in calls]


def _results(sess):
    return [(sess.result(t)[0].tolist(), sess.result(t)[1]) for t in range(sess.T)]


# ------------------------------------------------------------------------------------------------ 1. every feature on: order and buffers
def test_an_all_on_session_launches_its_stages_in_order_each_mask_on_the_one_before(dec128, calls):
    sess = dec128.session(**ALL_ON)
    sess.submit_all(PROMPTS, max_new_tokens=8, temperature=1.0, seed=[1, 2, 3, 4])
    assert _names(calls) == ADMISSION
    rows = {n: (a, got) for n, a, got in calls}
    prefill = rows["penalize_rows"][0][0]                                # the prefill's logits: what the first mask reads
    for before, after in zip(ADMISSION, ADMISSION[1:4]):                 # each mask reads the row the one before it returned
        assert rows[after][0][0].data_ptr() == rows[before][1].data_ptr(), after
    assert torch.equal(rows["sample_rows"][0][0], rows["truncate_rows"][1])
    assert rows["token_logprobs"][0][0].data_ptr() == prefill.data_ptr()     # the log-probabilities are the raw rows'
    del calls[:]
    sess.step(1, use_graph=False)
    assert _names(calls) == STEP
    step = {n: a for n, a, _ in calls}
    bufs = [sess.plogits, sess.clogits, sess.blogits, sess.tlogits]
    for name, buf in zip(STEP[1:5], bufs):                               # every mask writes its own buffer ...
        assert step[name][1].data_ptr() == buf.data_ptr(), name
    for name, buf in zip(STEP[2:6], bufs):                               # ... and the next launch reads it; the step end reads the last
        assert step[name][0].data_ptr() == buf.data_ptr(), name
    raw = step["step_penalize"][0]
    assert raw.data_ptr() not in [b.data_ptr() for b in bufs] and raw.shape == (4, V)
    assert step["step_logprobs"][0].data_ptr() == raw.data_ptr()         # the lm_head row, not a masked one


# ------------------------------------------------------------------------------------------------ 2. no feature on
def test_a_plain_session_launches_the_two_ragged_step_kernels_and_nothing_else(dec128, calls):
    sess = dec128.session()
    sess.submit_all(PROMPTS, max_new_tokens=8)
    assert _names(calls) == []                                           # greedy admission: argmax, no rows launch
    sess.step(1, use_graph=False)
    assert _names(calls) == ["step_begin_ragged", "step_end_ragged"]
    assert [getattr(sess, n).data_ptr() for n in BASE_STATE] + [sess.cache["valid"].data_ptr()] == [v.data_ptr() for v in sess._state()]
    sess.step(1)
    (key,) = sess._graphs
    assert len(key) == 10 and key[6:] == (False, None, False, False)


# ------------------------------------------------------------------------------------------------ 3. every feature on: graph key and state
def test_the_all_on_sessions_graph_key_and_state(dec128):
    from bitdelta_amd.serving_loop import FusedDeltaLinear
    dec = dec128
    sess = dec.session(**ALL_ON)
    sess.submit_all(PROMPTS, max_new_tokens=8, temperature=1.0, seed=[1, 2, 3, 4])
    sess.step(2)
    sess.step(2)
    (key,) = sess._graphs                                                # one capture, whatever is replayed
    assert key == (dec.fuse_glue, dec.fuse_qkv_norm, dec.fuse_gateup_norm, dec.norm_handoff, FusedDeltaLinear.use_tiled, sess.out.data_ptr(),
                   True, 3, True, True, True, 4, 8, "bans", 16, 8, "truncation")
    names = BASE_STATE + ("lp_n", "hist", "c_state", "c_n", "ss_n", "hit", "hold")
    want = [getattr(sess, n) for n in names]
    want.insert(len(BASE_STATE), sess.cache["valid"])
    assert [v.data_ptr() for v in sess._state()] == [v.data_ptr() for v in want]


# ------------------------------------------------------------------------------------------------ 4. graph and no-graph; the single write
def _request(stop_sequence):
    from bitdelta_amd.constraint import TokenAutomaton as TA
    return dict(max_new_tokens=14, stop_token_ids=[[3], [5, 4], [], [9, 7, 8]], temperature=[1.0, 0.7, 1.3, 0.9], top_k=[40, 20, 2 ** 40, 50],
                top_p=[0.9, 1.0, 0.95, 0.8], seed=[2 ** 63 + 17, 11, 5, 2 ** 64 - 1], repetition_penalty=1.3, logit_bias={70: 2.0},
                constraint=[None, TA.allowed_set(range(64, 192, 3)), None, None], stop_sequences=[stop_sequence],
                no_repeat_ngram_size=2, min_p=0.05)


def _run(dec, stop_sequence, use_graph):
    sess = dec.session(**ALL_ON)
    sess.submit_all(PROMPTS, **_request(stop_sequence))
    sess.run(use_graph=use_graph)
    return sess


@pytest.fixture(scope="module")
def runs(dec128):
    """(graph, no graph): the same all-on request on two sessions.  The stop sequence is tokens 5 and 6 of tenant 0's free turn (a first run
    with a sequence nobody emits finds them), so tenant 0 retires on it"""
    probe = _run(dec128, [V - 2, V - 1], False)
    y = _results(probe)[0][0]
    assert len(y) == 14
    seq = y[5:7]
    return _run(dec128, seq, True), _run(dec128, seq, False), seq


def test_graph_and_no_graph_agree_on_a_request_that_uses_every_feature(runs):
    a, b, seq = runs
    assert len(a._graphs) == 1 and len(b._graphs) == 0
    assert _results(a) == _results(b)
    y, reason = _results(a)[0]
    assert reason == 16 and y[-2:] == seq and a.stop_match(0) == (0, 2)
    assert set(_results(a)[1][0]) <= set(range(64, 192, 3)) | {4, 5}
    for name in ("hist", "c_state", "hit", "hold"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.hit.tolist() == [0, -1, -1, -1] and a.c_state.tolist() == [-1, 0, -1, -1]


def test_one_admission_leaves_exactly_the_requests_values_in_the_arrays(runs):
    a, _, seq = runs
    f32 = lambda v: np.float32(v).tolist()
    assert a.stop_ids.tolist() == [[3] + [-1] * 7, [4, 5] + [-1] * 6, [-1] * 8, [7, 8, 9] + [-1] * 5]
    assert a.temperature.tolist() == f32([1.0, 0.7, 1.3, 0.9]) and a.top_p.tolist() == f32([0.9, 1.0, 0.95, 0.8])
    assert a.top_k.tolist() == [40, 20, 2 ** 31 - 1, 50] and a.seed.tolist() == [17 - 2 ** 63, 11, 5, -1]
    assert a.pen.tolist() == [f32([1.3, 1.0 / 1.3, 0.0, 0.0])] * 4
    assert a.bias_id.tolist() == [[70] + [-1] * 15] * 4 and a.bias_val.tolist() == [[2.0] + [0.0] * 15] * 4
    assert a.trunc.tolist() == [f32([0.05, 1.0, 0.0, 0.0])] * 4
    assert a.ss_tok.tolist() == [[seq + [-1] * 6] + [[-1] * 8] * 3] * 4 and a.ss_len.tolist() == [[2, 0, 0, 0]] * 4
    assert a.ban_ngram.tolist() == [2] * 4 and a.ban_min.tolist() == [0] * 4
    assert a.ban_len.tolist() == [[0] * 16] * 4 and bool((a.ban_tok == -1).all())
    assert a.ctx_len.tolist() == [len(p) for p in PROMPTS]
    for t, p in enumerate(PROMPTS):
        assert a.ctx[t, :len(p)].tolist() == p
    ids = list(range(64, 192, 3))
    assert a.c_off[1, :2].tolist() == [0, len(ids)] and a.c_tok[1, :len(ids)].tolist() == ids and a.c_next[1, :len(ids)].tolist() == [0] * len(ids)
    assert a.c_acc[1, 0].item() == 1
    n = a.n.tolist()
    assert a.lp_n.tolist() == n and a.c_n.tolist() == n and a.ss_n.tolist() == n


# ------------------------------------------------------------------------------------------------ 5. load_tenant
def test_load_tenant_clears_the_slots_arrays_of_every_feature_and_nobody_elses(runs, dec128):
    a, _, _ = runs
    assert not any(a.active())
    before = {n: getattr(a, n).clone() for n in ARRAYS}
    a.load_tenant(1, dict(dec128.tenant_state(1)))
    got = {n: getattr(a, n) for n in ARRAYS}
    for n in ARRAYS:
        for t in (0, 2, 3):
            assert torch.equal(got[n][t], before[n][t]), (n, t)
    f32 = lambda v: np.float32(v).tolist()
    zero = ("lp_n", "c_n", "ss_n", "hold", "ctx_len", "ban_ngram", "ban_min", "n", "done", "temperature", "top_k", "seed", "ss_len", "ban_len",
            "bias_val", "hist", "out")
    for n in zero:
        assert not bool(got[n][1].any()), n
    for n in ("stop_ids", "bias_id", "ss_tok", "ban_tok", "c_state", "hit"):
        assert bool((got[n][1] == -1).all()), n
    assert got["top_p"][1].item() == 1.0 and got["pen"][1].tolist() == f32([1.0, 1.0, 0.0, 0.0]) and got["trunc"][1].tolist() == f32([0.0, 1.0, 0.0, 0.0])
    assert not bool(a.cache["valid"][1].any()) and bool(a.cache["valid"][2].any())
