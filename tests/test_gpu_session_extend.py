"""TenantSession.extend: the next turn of a tenant's conversation from its cached keys (serving_loop.py), on the GPU.

1. Two turns against the dense twin: submit a 9-token prompt, run, extend by 20 tokens, run -- the second turn's tokens pass the teacher-forced
   rule of tests/test_gpu_ragged_decode.py (argmax of tenant t's dense fp32 model where its top-2 margin is above 0.05, within 0.1 of the top
   otherwise) on pads + prompt + turn-1 tokens + new tokens + turn-2 tokens.  Once per arm: bd_srv_prefill_attention_cached, and the stock ops
   (hip_prefill_attention = False); the test counts the kernel's calls, so each arm is known to have run.
2. Independence: a tenant extended while two others generate produces what it produces alone, the others' tokens are unchanged, and the extension
   itself leaves their pos / valid / cache rows as they were.
3. Lifecycle: every refusal leaves state and cache unchanged (clones compared); extend after load_tenant; admission at the end of the cache;
   tokens = [] (a one-row chunk); an int8 base; one full-width Mistral-7B layer with 6 tenants.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bd():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import bitdelta_amd
    from bitdelta_amd import _lib
    _lib.lib()
    return bitdelta_amd


def _toks(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, 500, (n,), generator=g).tolist()


def _truth(bd, dec, t, npad, history, toks):
    """the teacher-forced rule against tenant t's dense fp32 model: `history` (every token of the conversation so far, behind npad left pads),
    then each of `toks` in turn"""
    from test_gpu_serving import _dense_reference_logits
    seq = torch.tensor([0] * npad + list(history), dtype=torch.long, device="cuda")
    msk = torch.tensor([False] * npad + [True] * len(history), device="cuda")
    for s_, tok in enumerate(toks.tolist()):
        ref = _dense_reference_logits(bd, dec, t, seq, msk)
        top2 = ref.topk(2).values
        if (top2[0] - top2[1]).item() > 0.05:
            assert tok == int(ref.argmax()), (t, s_)
        else:
            assert ref[tok] >= top2[0] - 0.1, (t, s_)
        seq = torch.cat([seq, torch.tensor([tok], device="cuda")])
        msk = torch.cat([msk, torch.tensor([True], device="cuda")])


def _clone_state(state):
    """a deep copy of TenantDecoder.tenant_state(t) (views of the decoder's storage)"""
    if isinstance(state, dict):
        return {k: _clone_state(v) for k, v in state.items()}
    if isinstance(state, (tuple, list)):
        return type(state)(_clone_state(v) for v in state)
    return state.clone()


def _snapshot(sess):
    return [v.clone() for v in sess._state()] + [c.clone() for c in sess.cache["k"] + sess.cache["v"]]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture
def count_cached(monkeypatch):
    from bitdelta_amd import serving_ops as ops
    calls = []
    orig = ops.prefill_attention_cached

    def counted(q, *a, **kw):
        calls.append(tuple(q.shape))
        return orig(q, *a, **kw)
    monkeypatch.setattr(ops, "prefill_attention_cached", counted)
    return calls


@pytest.fixture(scope="module")
def dec128(bd):
    from bitdelta_amd.serving_loop import TenantDecoder
    return TenantDecoder.synthetic("tiny128", 4, "cuda", dtype=torch.float16, seed=31, max_len=256)


# ------------------------------------------------------------------------------------------------ 1. two turns against the dense twin
@pytest.mark.parametrize("hip", [True, False], ids=["hip", "stock"])
def test_two_turns_agree_with_the_dense_model(bd, dec128, count_cached, hip):
    dec, t = dec128, 1
    prompt, more = _toks(9, 11), _toks(20, 12)
    dec.hip_prefill_attention = hip
    try:
        sess = dec.session()
        sess.submit(t, prompt, max_new_tokens=6)
        sess.run()
        turn1, r1 = sess.result(t)
        assert r1 == 2 and turn1.numel() == 6 and int(sess.pos[t]) == 64 + 5 and not count_cached
        sess.extend(t, more, max_new_tokens=6)
        assert sess.active()[t] and int(sess.pos[t]) == 64 + 5 + 21 and int(sess.n[t]) == 1
        assert count_cached == ([(1, 21, 4, 128)] * len(dec.layers) if hip else [])
        sess.run()
    finally:
        dec.hip_prefill_attention = True
    turn2, r2 = sess.result(t)
    assert r2 == 2 and turn2.numel() == 6 and int(sess.pos[t]) == 64 + 5 + 21 + 5
    valid = sess.cache["valid"][t]
    assert not bool(valid[:55].any()) and bool(valid[55:95].all()) and not bool(valid[95:].any())
    _truth(bd, dec, t, 55, prompt + turn1.tolist() + more, turn2)


# ------------------------------------------------------------------------------------------------ 2. independence
def _two_turns_alone(dec, t, prompt, more, mx1, mx2):
    sess = dec.session()
    sess.submit(t, prompt, max_new_tokens=mx1)
    sess.run()
    first = sess.result(t)[0]
    sess.extend(t, more, max_new_tokens=mx2)
    sess.run()
    return first, sess.result(t)[0]


def _independence(dec):
    prompts = {0: _toks(33, 1), 1: _toks(9, 2), 2: _toks(70, 3)}
    more = _toks(20, 4)
    alone1 = _two_turns_alone(dec, 1, prompts[1], more, 5, 6)
    alone = {}
    for t, mx in ((0, 12), (2, 10)):
        s_ = dec.session()
        s_.submit(t, prompts[t], max_new_tokens=mx)
        s_.run()
        alone[t] = s_.result(t)[0]
    sess = dec.session()
    sess.submit(1, prompts[1], max_new_tokens=5)
    sess.run()
    assert torch.equal(sess.result(1)[0], alone1[0])
    sess.submit(0, prompts[0], max_new_tokens=12)
    sess.submit(2, prompts[2], max_new_tokens=10)
    sess.step(3)
    others = lambda: [x[[0, 2, 3]].clone() for x in (sess.pos, sess.n, sess.tok, sess.done, sess.active_flags, sess.out, sess.cache["valid"])] + \
        [c[[0, 2, 3]].clone() for c in sess.cache["k"] + sess.cache["v"]]
    before = others()
    sess.extend(1, more, max_new_tokens=6)
    assert _same(before, others()), "the extension of tenant 1 touched another tenant's state or cache rows"
    assert sess.active() == [True, True, True, False]
    sess.run()
    assert torch.equal(sess.result(1)[0], alone1[1]), (sess.result(1)[0], alone1[1])
    for t in (0, 2):
        assert torch.equal(sess.result(t)[0], alone[t]) and sess.result(t)[1] == 2
    assert not bool(sess.cache["valid"][3].any())


def test_a_tenant_extended_next_to_others_generates_what_it_generates_alone(bd, dec128):
    _independence(dec128)


def test_extension_on_an_int8_base(bd):
    from bitdelta_amd.serving_loop import TenantDecoder
    _independence(TenantDecoder.synthetic("tiny128", 4, "cuda", dtype=torch.float16, seed=31, max_len=256, base_int8=True))


# ------------------------------------------------------------------------------------------------ 3. lifecycle
def test_refusals_leave_state_and_cache_unchanged(bd, dec128):
    from bitdelta_amd.serving_loop import TenantDecoder
    dec = dec128
    sess = dec.session()
    sess.submit(0, _toks(9, 5), max_new_tokens=4)
    sess.run()
    sess.submit(1, _toks(12, 6), max_new_tokens=30)
    sess.step(2)
    snap = _snapshot(sess)
    with pytest.raises(RuntimeError):
        sess.extend(1, [5, 6, 7])                               # still generating
    with pytest.raises(RuntimeError):
        sess.extend(3, [5, 6, 7])                               # never submitted
    with pytest.raises(ValueError):
        sess.extend(0, list(range(1, 200)))                     # 67 + 200 rows > 256
    with pytest.raises(ValueError):
        sess.extend(0, [5], stop_token_ids=list(range(9)))      # more stop ids than the session holds
    with pytest.raises(IndexError):
        sess.extend(4, [5])
    assert _same(snap, _snapshot(sess))
    # a fine-tune replaced since: the rows in the cache are another model's
    own = _clone_state(dec.tenant_state(0))
    sess.load_tenant(0, _clone_state(dec.tenant_state(2)))
    snap = _snapshot(sess)
    with pytest.raises(RuntimeError):
        sess.extend(0, [5, 6, 7])
    assert _same(snap, _snapshot(sess))
    sess.run()
    sess.load_tenant(0, own)                                    # (the decoder is shared by the module: tenant 0 gets its fine-tune back)
    # the conversation's real length beyond MAX_PROMPT (a cache that would hold it)
    big = TenantDecoder.synthetic("tiny128", 2, "cuda", dtype=torch.float16, seed=3, max_len=1200, shared_heads=True)
    s2 = big.session()
    s2.submit(1, _toks(9, 7), max_new_tokens=3)
    s2.run()
    snap = _snapshot(s2)
    with pytest.raises(ValueError, match="reduce the input length"):
        s2.extend(1, _toks(1020, 8))
    assert _same(snap, _snapshot(s2))
    s2.extend(1, _toks(30, 8), max_new_tokens=2)                # ... and a turn that fits is taken
    s2.run()
    assert s2.result(1)[1] == 2 and s2.result(1)[0].numel() == 2


def test_admission_at_the_end_of_the_cache(bd):
    from bitdelta_amd.serving_loop import TenantDecoder
    dec = TenantDecoder.synthetic("tiny128", 4, "cuda", dtype=torch.float16, seed=33, max_len=96, shared_heads=True)
    sess = dec.session()
    for t in (0, 2):
        sess.submit(t, _toks(9, 20 + t), max_new_tokens=3)
    sess.run()
    assert int(sess.pos[0]) == 66 and int(sess.pos[2]) == 66
    # tenant 0: the chunk ends one row before the end -- admitted, one step fills the last row, reason 4 after two tokens
    sess.extend(0, _toks(28, 30), max_new_tokens=5)
    assert sess.active()[0] and int(sess.pos[0]) == 95
    sess.run()
    toks, reason = sess.result(0)
    assert reason == 4 and toks.numel() == 2 and int(sess.pos[0]) == 96
    # tenant 2: the chunk ends at the last row -- its first token is all there is room for
    sess.extend(2, _toks(29, 31), max_new_tokens=5)
    assert not sess.active()[2] and sess.result(2)[1] == 4 and sess.result(2)[0].numel() == 1 and int(sess.pos[2]) == 96
    assert bool(sess.cache["valid"][2, 55:96].all())
    snap = _snapshot(sess)
    for t in (0, 2):
        with pytest.raises(RuntimeError):
            sess.extend(t, [])                                  # the cache is full
    assert _same(snap, _snapshot(sess))
    for t in (1, 3):
        assert not bool(sess.cache["valid"][t].any()) and int(sess.cache["k"][0][t].abs().max()) == 0


@pytest.mark.parametrize("hip", [True, False], ids=["hip", "stock"])
def test_extend_without_new_tokens_is_a_one_row_chunk(bd, dec128, count_cached, hip):
    """tokens = []: the chunk is the last emitted token alone (Sq = 1) and the turn continues the generation"""
    dec, t = dec128, 2
    prompt = _toks(40, 41)
    dec.hip_prefill_attention = hip
    try:
        sess = dec.session()
        sess.submit(t, prompt, max_new_tokens=4, stop_token_ids=[100000])
        sess.run()
        turn1 = sess.result(t)[0]
        sess.extend(t, [], max_new_tokens=4)
        assert count_cached == ([(1, 1, 4, 128)] * len(dec.layers) if hip else [])
        sess.run()
    finally:
        dec.hip_prefill_attention = True
    turn2, r2 = sess.result(t)
    assert r2 == 2 and turn2.numel() == 4 and int(sess.pos[t]) == 64 + 3 + 1 + 3
    assert int((sess.stop_ids[t] >= 0).sum()) == 0              # the second turn's (empty) stop list replaced the first's
    _truth(bd, dec, t, 24, prompt + turn1.tolist(), turn2)


def test_full_width_layer_second_turn_agrees_with_dense_models(bd):
    """one Mistral-7B layer (32 / 8 heads), 6 tenants: tenant 3 takes a second turn while tenant 0 generates"""
    from bitdelta_amd.serving_loop import TenantDecoder
    dec = TenantDecoder.synthetic("mistral-1layer", 6, "cuda", dtype=torch.float16, seed=21, max_len=192)
    prompt, more, other = _toks(33, 51), _toks(20, 52), _toks(9, 53)
    sess = dec.session()
    sess.submit(3, prompt, max_new_tokens=3)
    sess.run()
    turn1 = sess.result(3)[0]
    sess.submit(0, other, max_new_tokens=8)
    sess.step(2)
    sess.extend(3, more, max_new_tokens=3)
    sess.run()
    turn2, r2 = sess.result(3)
    assert r2 == 2 and turn2.numel() == 3 and sess.result(0)[0].numel() == 8
    _truth(bd, dec, 3, 31, prompt + turn1.tolist() + more, turn2)
    _truth(bd, dec, 0, 55, other, sess.result(0)[0][:2])
    for t in (1, 2, 4, 5):
        assert not bool(sess.cache["valid"][t].any())
