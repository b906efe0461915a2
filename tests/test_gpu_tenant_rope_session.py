"""Per-tenant rotary tables through the decoder and the session (GPU): TenantDecoder(rope=[spec per tenant]) against dense per-tenant models that
build their OWN fp64 table from the spec's frequencies (they never read dec.cos), against a shared-table decoder where every tenant has the
same spec, across the launch forms (staggered admission, graph replay, stock-op glue), through extend, load_tenant(rope=) on a live session,
and score().  Three specs: neutral, linear factor 4 (vicuna-16k's), rope_theta 1e6."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = (40, 64, 33)
BOUND = 3e-3                 # tests/test_gpu_serving.py: prefill logits of a two-layer fp16 model against its dense twin


@pytest.fixture(scope="module")
def bd():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import bitdelta_amd
    from bitdelta_amd import _lib
    _lib.lib()
    return bitdelta_amd


def _specs():
    from bitdelta_amd.serving_loop import rope_spec
    return [rope_spec(), rope_spec(scaling={"rope_type": "linear", "factor": 4.0}), rope_spec(1e6)]


def _toks(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, 500, (n,), generator=g).tolist()


PROMPTS = [_toks(n, 300 + i) for i, n in enumerate(LENS)]


def _make(rope, seed=51, T=3):
    from bitdelta_amd.serving_loop import TenantDecoder
    return TenantDecoder.synthetic("tiny128", T, "cuda", dtype=torch.float16, seed=seed, max_len=256, rope=rope)


@pytest.fixture(scope="module")
def dec(bd):
    return _make(_specs())


def relerr(a, ref):
    a, ref = a.double(), ref.double()
    return ((a - ref).norm() / ref.norm()).item()


def _dense(bd, dec, t, ids, am, spec, all_rows=False):
    """test_gpu_serving._dense_reference_logits' model -- tenant t as ONE dense network (W + alpha * S^T), no KV cache, raw positions, causal mask,
    left pads masked as keys -- in float64 and with its own rotary table: cos / sin of position * inv_freq in float64, from the SPEC's
    frequencies, never rounded to 16 bits and never read from the decoder.  ids / am: 1-D tensors (the padded sequence so far)."""
    import torch.nn.functional as F
    from bitdelta_amd.serving_loop import rope_inv_freq
    hid, inter, nl, heads, kvh, vocab = dec.cfg
    hd = dec.hd
    L = ids.shape[0]

    def merged(fl):
        S = (bd.unpack(fl.mask[t]).double() * 2 - 1).T
        return fl.weight.double() + fl.column_alpha(t).double()[:, None] * S

    def rms(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + dec.eps) * w.double()

    def rope(x, cos, sin):
        return x * cos + torch.cat([x[..., hd // 2:], x[..., :hd // 2]], -1) * sin

    ang = torch.outer(torch.arange(L, dtype=torch.float64), rope_inv_freq(spec, hd).double()).to(ids.device)
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1), torch.cat([-ang.sin(), ang.sin()], -1)
    x = dec.embed[t][ids].double()
    keymask = am[None, :] & torch.ones(L, L, dtype=torch.bool, device=ids.device).tril()
    keymask = keymask | torch.eye(L, dtype=torch.bool, device=ids.device)
    for layer in dec.layers:
        q, k, v = layer.qkv.split(rms(x, layer.norm1[t]) @ merged(layer.qkv).T)
        q = rope(q.view(L, heads, hd).transpose(0, 1), cos, sin)
        k = rope(k.view(L, kvh, hd).transpose(0, 1), cos, sin)
        v = v.view(L, kvh, hd).transpose(0, 1)
        k, v = k.repeat_interleave(heads // kvh, 0), v.repeat_interleave(heads // kvh, 0)
        s = ((q @ k.transpose(1, 2)) / hd ** 0.5).masked_fill(~keymask[None], float("-inf"))
        x = x + (s.softmax(-1) @ v).transpose(0, 1).reshape(L, heads * hd) @ merged(layer.o).T
        g, u = layer.gate_up.split(rms(x, layer.norm2[t]) @ merged(layer.gate_up).T)
        x = x + (F.silu(g) * u) @ merged(layer.down).T
    return rms(x if all_rows else x[-1], dec.final_norm[t]) @ dec.lm_head[t].double().T


def _truth(bd, dec, t, spec, npad, history, toks):
    """the teacher-forced rule: the argmax of tenant t's dense model where its top-2 margin is above 0.05, within 0.1 of the top otherwise"""
    seq = torch.tensor([0] * npad + list(history), dtype=torch.long, device="cuda")
    msk = torch.tensor([False] * npad + [True] * len(history), device="cuda")
    for s_, tok in enumerate(torch.as_tensor(toks).tolist()):
        ref = _dense(bd, dec, t, seq, msk, spec)
        top2 = ref.topk(2).values
        if (top2[0] - top2[1]).item() > 0.05:
            assert tok == int(ref.argmax()), (t, s_)
        else:
            assert ref[tok] >= top2[0] - 0.1, (t, s_)
        seq = torch.cat([seq, torch.tensor([tok], device="cuda")])
        msk = torch.cat([msk, torch.tensor([True], device="cuda")])


def _session_tokens(d, prompts=PROMPTS, n=6, use_graph=True, **kw):
    sess = d.session(**kw)
    for t, p in enumerate(prompts):
        sess.submit(t, p, max_new_tokens=n)
    sess.run(use_graph=use_graph)
    return [sess.result(t)[0] for t in range(len(prompts))]


# ------------------------------------------------------------------------------------------------ 1. against dense models
def test_prefill_logits_and_greedy_tokens_follow_each_tenants_table(bd, dec):
    specs = _specs()
    assert dec.rope_per_tenant and dec.cos.shape == (3, 256, 128) and [dec.tenant_rope(t) for t in range(3)] == specs
    ids, am = dec.prepare(PROMPTS)
    assert ids.shape == (3, 64)
    lg = dec.prefill(ids, am, dec.new_cache())
    refs = [_dense(bd, dec, t, ids[t], am[t], specs[t]) for t in range(3)]
    # the same weights with one shared neutral table against the unchanged fp32 reference of tests/test_gpu_serving.py: what the bound is used to
    from test_gpu_serving import _dense_reference_logits
    plain = _make(None)
    lg0 = plain.prefill(ids, am, plain.new_cache())
    for t in range(3):
        e, e0 = relerr(lg[t], refs[t]), relerr(lg0[t], _dense_reference_logits(bd, plain, t, ids[t], am[t]))
        print("TENANT-ROPE prefill tenant %d: relerr against its dense fp64 model %.3e (rope=None decoder against the fp32 reference: %.3e)" % (t, e, e0))
        assert e <= BOUND, (t, e)
    assert torch.equal(lg[0], lg0[0])                                       # the neutral slot is the decoder of before, bit for bit
    # a wrong table cannot pass: for the two scaled tenants the dense model with the NEUTRAL table is >= 10 x the bound away from the right one
    for t in (1, 2):
        wrong = _dense(bd, dec, t, ids[t], am[t], specs[0])
        gap = relerr(wrong, refs[t])
        print("TENANT-ROPE tenant %d: dense model with the neutral table against the right one: relerr %.3e" % (t, gap))
        assert gap >= 10 * BOUND, (t, gap)
        assert relerr(lg[t], wrong) > BOUND and relerr(lg0[t], refs[t]) > BOUND
    steps = 6
    toks, n = dec.generate(PROMPTS, max_new_tokens=steps, use_graph=True)
    toks_e, _ = dec.generate(PROMPTS, max_new_tokens=steps, use_graph=False)
    assert n == steps and torch.equal(toks, toks_e)
    for t in range(3):
        _truth(bd, dec, t, specs[t], 64 - LENS[t], PROMPTS[t], toks[t])


# ------------------------------------------------------------------------------------------------ 2. the same rope everywhere
def test_one_spec_for_every_tenant_equals_the_shared_table(bd):
    lin4 = _specs()[1]
    listed, shared = _make([lin4] * 3), _make(lin4)
    assert listed.cos.shape == (3, 256, 128) and shared.cos.shape == (256, 128) and torch.equal(listed.cos[2], shared.cos)
    ids, am = listed.prepare(PROMPTS)
    assert torch.equal(listed.prefill(ids, am, listed.new_cache()), shared.prefill(ids, am, shared.new_cache()))
    a, na = listed.generate(PROMPTS, max_new_tokens=6)
    b, nb = shared.generate(PROMPTS, max_new_tokens=6)
    assert na == nb == 6 and torch.equal(a, b)
    for x, y in zip(_session_tokens(listed), _session_tokens(shared)):
        assert x.numel() == 6 and torch.equal(x, y)
    # ... and it is not the neutral decoder
    assert not torch.equal(listed.prefill(ids, am, listed.new_cache()), _make(None).prefill(ids, am, shared.new_cache()))


# ------------------------------------------------------------------------------------------------ 3. launch forms
def test_session_tokens_do_not_depend_on_the_launch_form(bd, dec):
    alone = []
    for t in range(3):
        sess = dec.session()
        sess.submit(t, PROMPTS[t], max_new_tokens=8)
        sess.run()
        alone.append(sess.result(t)[0])
    sess = dec.session()                                                    # staggered admission: every tenant at its own position
    sess.submit(0, PROMPTS[0], max_new_tokens=8)
    sess.step(2)
    sess.submit(1, PROMPTS[1], max_new_tokens=8)
    sess.step(3)
    sess.submit(2, PROMPTS[2], max_new_tokens=8)
    sess.run()
    assert len(sess._graphs) >= 1
    for t in range(3):
        assert alone[t].numel() == 8 and torch.equal(sess.result(t)[0], alone[t]), t
    for x, y in zip(_session_tokens(dec, n=8, use_graph=False), _session_tokens(dec, n=8, use_graph=True)):
        assert torch.equal(x, y)                                            # eager == graph replay
    # the stock-op arm follows the same tables: prefill logits of both arms, each within the dense bound of the same model
    ids, am = dec.prepare(PROMPTS)
    hip = dec.prefill(ids, am, dec.new_cache())
    dec.fast_glue = False
    try:
        stock = dec.prefill(ids, am, dec.new_cache())
    finally:
        dec.fast_glue = True
    for t in range(3):
        e = relerr(stock[t], hip[t])
        print("TENANT-ROPE stock-op prefill against HIP prefill, tenant %d: relerr %.3e" % (t, e))
        assert e <= BOUND, (t, e)
        # tests/test_gpu_serving.py's stock-versus-HIP rule is the same prefill token through either arm; beyond fp16 noise it must agree
        top2 = hip[t].float().topk(2).values
        assert (top2[0] - top2[1]).item() <= 0.05 or int(stock[t].argmax()) == int(hip[t].argmax()), t


# ------------------------------------------------------------------------------------------------ 4. extend
def test_extend_continues_a_scaled_tenants_conversation(bd, dec):
    t, spec = 1, _specs()[1]
    prompt, more = _toks(9, 11), _toks(20, 12)
    sess = dec.session()
    sess.submit(t, prompt, max_new_tokens=6)
    sess.run()
    turn1 = sess.result(t)[0]
    sess.extend(t, more, max_new_tokens=6)
    sess.run()
    turn2, reason = sess.result(t)
    assert reason == 2 and turn2.numel() == 6 and int(sess.pos[t]) == 64 + 5 + 21 + 5
    whole = prompt + turn1.tolist() + more
    _truth(bd, dec, t, spec, 55, whole, turn2)
    # a submit of the whole conversation (35 tokens behind 29 pads: other absolute positions, the same differences) obeys the same rule
    again = dec.session()
    again.submit(t, whole, max_new_tokens=6)
    again.run()
    _truth(bd, dec, t, spec, 64 - len(whole), whole, again.result(t)[0])


# ------------------------------------------------------------------------------------------------ 5. load_tenant(rope=) on a live session
def _clone_state(state):
    if isinstance(state, dict):
        return {k: _clone_state(v) for k, v in state.items()}
    if isinstance(state, (tuple, list)):
        return type(state)(_clone_state(v) for v in state)
    return state.clone()


def test_load_tenant_with_a_rope_spec_on_a_live_session(bd):
    from bitdelta_amd.serving_loop import ROPE_DEFAULT, rope_spec, rope_tables
    specs = _specs()
    new = rope_spec(5e5, {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                          "original_max_position_embeddings": 64})
    d = _clone_state(_make(None, seed=77).tenant_state(2))                   # another fine-tune (signs, scales, dense rows) for slot 0
    X, U = _make(specs), _make(specs)
    Y = _make([new] + specs[1:])                                             # built with the spec in slot 0, then given the fine-tune
    assert Y.load_tenant(0, d, rope=new) is False
    Z = _make(specs)
    Z.load_tenant(0, d)
    sx, su = X.session(), U.session()
    for s in (sx, su):
        s.submit(1, PROMPTS[1], max_new_tokens=12)
        s.submit(2, PROMPTS[2], max_new_tokens=9)
        s.step(3)
    graphs = dict(sx._graphs)
    assert len(graphs) == 1
    ptrs = (X.cos.data_ptr(), X.sin.data_ptr())
    before = (X.cos.clone(), X.sin.clone())
    view = X.tenant_view(0)
    with pytest.raises(ValueError):
        sx.load_tenant(0, d, rope=rope_spec(scaling={"rope_type": "linear", "factor": 2.0})[:3])      # not a spec record: refused before any write
    with pytest.raises(ValueError):
        sx.load_tenant(0, d, rope=rope_spec(inv_freq=[1.0] * 32))
    assert X.tenant_rope(0) == specs[0] and torch.equal(X.cos, before[0])
    assert sx.load_tenant(0, d, rope=new) is False
    assert sx._graphs == graphs                                              # the table rewrite alone drops no captured graph
    assert X.tenant_rope(0) == new and [X.tenant_rope(t) for t in (1, 2)] == specs[1:]
    assert (X.cos.data_ptr(), X.sin.data_ptr()) == ptrs and X.cos.shape == (3, 256, 128)
    c, s = rope_tables(256, 128, "cuda", torch.float16, new)
    assert torch.equal(X.cos[0], c) and torch.equal(X.sin[0], s) and not torch.equal(c, before[0][0])
    assert torch.equal(X.cos[1:], before[0][1:]) and torch.equal(X.sin[1:], before[1][1:])
    assert torch.equal(view.cos, c) and X.tenant_view(0).cos.data_ptr() == ptrs[0]           # a view slices the rewritten storage
    with pytest.raises(RuntimeError):
        sx.extend(0, [5, 6])                                                 # nothing of the fine-tune that left is extended
    sx.submit(0, PROMPTS[0], max_new_tokens=8)
    sx.run()
    su.run()
    assert sx._graphs == graphs
    for t in (1, 2):
        assert torch.equal(sx.result(t)[0], su.result(t)[0]), t             # the other tenants: exactly the tokens of the untouched decoder
    assert len(sx.result(1)[0]) == 12 and len(sx.result(2)[0]) == 9
    sy = Y.session()
    sy.submit(0, PROMPTS[0], max_new_tokens=8)
    sy.run()
    assert torch.equal(sx.result(0)[0], sy.result(0)[0]) and len(sx.result(0)[0]) == 8
    # rope=None puts the decoder's default back
    assert sx.load_tenant(0, d) is False
    assert X.tenant_rope(0) == ROPE_DEFAULT and torch.equal(X.cos, before[0]) and torch.equal(X.sin, before[1]) and sx._graphs == graphs
    sx.submit(0, PROMPTS[0], max_new_tokens=8)
    sx.run()
    sz = Z.session()
    sz.submit(0, PROMPTS[0], max_new_tokens=8)
    sz.run()
    assert torch.equal(sx.result(0)[0], sz.result(0)[0])


# ------------------------------------------------------------------------------------------------ 6. a refused load
def test_shared_table_decoder_refuses_another_spec(bd):
    specs = _specs()
    S = _make(specs[2])
    d = _clone_state(_make(None, seed=77).tenant_state(2))
    assert not S.rope_per_tenant and S.cos.shape == (256, 128)
    sess = S.session()
    sess.load_tenant(0, _clone_state(S.tenant_state(0)), tag="a")
    sess.submit(0, PROMPTS[0], max_new_tokens=6)
    sess.run()
    want = sess.result(0)[0]
    kept = _clone_state(S.tenant_state(0))
    table = (S.cos.clone(), S.sin.clone())
    for bad in (specs[1], specs[0]):
        with pytest.raises(ValueError):
            sess.load_tenant(0, d, tag="b", rope=bad)
        with pytest.raises(ValueError):
            S.load_tenant(0, d, tag="b", rope=bad)
    assert S.tenant_tag(0) == "a" and S.tenant_rope(0) == specs[2]
    assert torch.equal(S.cos, table[0]) and torch.equal(S.sin, table[1])

    def same(a, b):
        if isinstance(a, dict):
            return all(same(a[k], b[k]) for k in a)
        if isinstance(a, (tuple, list)):
            return all(same(x, y) for x, y in zip(a, b))
        return torch.equal(a, b)
    assert same(S.tenant_state(0), kept)
    assert int(sess.n[0]) == 6 and torch.equal(sess.result(0)[0], want)      # the refused load cleared nothing
    sess.submit(0, PROMPTS[0], max_new_tokens=6)
    sess.run()
    assert torch.equal(sess.result(0)[0], want)
    # the decoder's own spec, spelled or by default, is a load like any other
    sess.load_tenant(0, d, tag="b", rope=specs[2])
    assert S.tenant_tag(0) == "b" and S.tenant_rope(0) == specs[2] and torch.equal(S.cos, table[0])
    sess.load_tenant(0, kept, tag="a")
    sess.submit(0, PROMPTS[0], max_new_tokens=6)
    sess.run()
    assert torch.equal(sess.result(0)[0], want)


# ------------------------------------------------------------------------------------------------ 7. score
def test_score_follows_each_tenants_table(bd, dec):
    """tests/test_gpu_score.py's band: e = the largest |prefill's last-row logit - the dense model's| over the tenants, 4 e + the kernel's bound"""
    KERNEL = 2.0 ** -19
    specs = _specs()
    seqs = [_toks(n, 70 + i) for i, n in enumerate((33, 70, 128))]
    ids, am = dec.prepare(seqs)
    assert ids.shape == (3, 128)
    last = dec.prefill(ids, am, dec.new_cache(128))
    got = dec.score(seqs)
    e, dense = 0.0, []
    for t in range(3):
        dense.append(_dense(bd, dec, t, ids[t], am[t], specs[t], all_rows=True))
        e = max(e, float((last[t].double() - dense[t][-1]).abs().max()))
    print("TENANT-ROPE score: e = largest |prefill last-row logit - dense fp64 model| over the tenants: %.3e" % e)
    for t in range(3):
        s, pad = seqs[t], 128 - len(seqs[t])
        logp = torch.log_softmax(dense[t], dim=-1)
        ref = torch.zeros(len(s), dtype=torch.float64, device="cuda")
        for i in range(1, len(s)):
            ref[i] = -logp[pad + i - 1, s[i]]
        worst = float((got[t].double() - ref).abs().max())
        print("TENANT-ROPE score tenant %d: largest |d| = %.3e (band 4 e = %.3e)" % (t, worst, 4 * e))
        assert bool(((got[t].double() - ref).abs() <= 4 * e + KERNEL * (1.0 + ref.abs())).all()), (t, worst, e)
        if t:                                                               # the neutral table's losses do not fit the band of a scaled tenant
            wrong = torch.log_softmax(_dense(bd, dec, t, ids[t], am[t], specs[0], all_rows=True), dim=-1)
            refw = torch.zeros_like(ref)
            for i in range(1, len(s)):
                refw[i] = -wrong[pad + i - 1, s[i]]
            assert not bool(((got[t].double() - refw).abs() <= 4 * e + KERNEL * (1.0 + refw.abs())).all()), t
