"""GPU tests of per-tenant positions in decode: the ragged forms of the decode attention and of the two step kernels, and
serving_loop.TenantSession on top of them.  The ragged attention is held to the scalar kernel bit for bit (a tenant at position p must see
exactly what a lockstep launch at p shows it); the step kernels to a torch restatement of their rules; the session to `generate` (lockstep),
to itself (a tenant's tokens do not depend on who else is running) and to dense fp32 per-tenant models."""
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


# ------------------------------------------------------------------------------------------------ 1. attention
def _ragged_attention(qkv, cos, sin, kc, vc, valid, pos, active, heads, kvh):
    """bd_srv_decode_attention_ragged through the C entry, into an output pre-filled with a NaN pattern (a row the kernel must zero cannot be
    zero by accident).  Returns (out, last attention form)."""
    from bitdelta_amd._lib import DTYPE_CODE, check, lib, ptr, stream_ptr, workspace
    L = lib()
    T, Lc = qkv.shape[0], kc.shape[2]
    out = torch.full((T, 1, heads * 128), float("nan"), device=qkv.device, dtype=qkv.dtype)
    need = L.bd_srv_decode_attention_workspace_bytes(T, heads, kvh, 128, Lc)
    ws, need = workspace(need, qkv.device, zeroed=True) if need > 0 else (None, 0)
    check(L.bd_srv_decode_attention_ragged(ptr(qkv), ptr(cos), ptr(sin), ptr(kc), ptr(vc), ptr(valid), ptr(pos), ptr(active), ptr(out), T, heads, kvh,
                                           128, Lc, qkv.stride(0), out.stride(0), DTYPE_CODE[qkv.dtype], ptr(ws), need, stream_ptr()), "ragged")
    torch.cuda.synchronize()
    return out, L.bd_last_attention_form(), ws


ATTN_CASES = [(dt, 4, h, k, Lc) for dt in (torch.float16, torch.bfloat16) for h, k in ((8, 2), (4, 4), (8, 1)) for Lc in (96, 320, 640)]
ATTN_CASES += [(torch.float16, 12, 8, 2, 320), (torch.bfloat16, 12, 8, 2, 640)]       # 24 (tenant, kv head) pairs: the rule keeps 4 splits


@pytest.mark.parametrize("dtype,T,heads,kvh,Lc", ATTN_CASES)
def test_ragged_attention_rows_equal_the_scalar_kernel(bd, dtype, T, heads, kvh, Lc):
    """Row t of a ragged launch == row t of the scalar launch at p = pos[t], bit for bit: output, cache rows, validity bytes.  Lc 96 runs unsplit,
    320 and 640 split (T = 4: 8 or 16 splits, the MAXS = 16 merge; T = 12: 4 splits, the MAXS = 4 merge).  Then tenants that must stay out."""
    from bitdelta_amd import serving_ops as ops
    from bitdelta_amd.serving_loop import _rope_tables
    g = torch.Generator(device="cuda").manual_seed(heads * 1000 + kvh * 100 + Lc)
    cos, sin = _rope_tables(Lc, 128, "cuda", dtype)
    qkv = torch.randn(T, 1, (heads + 2 * kvh) * 128, device="cuda", generator=g).to(dtype)
    kc0 = torch.randn(T, kvh, Lc, 128, device="cuda", generator=g).to(dtype)
    vc0 = torch.randn(T, kvh, Lc, 128, device="cuda", generator=g).to(dtype)
    mid = Lc // 2 + 5                                            # inside a middle split, not on an iteration boundary
    pads = [0, 3, 17, 30]
    act_all = torch.ones(T, dtype=torch.bool, device="cuda")
    scalar = {}                                                  # position -> (out, kc, vc, valid, form) of the lockstep launch there

    def base_valid(pos_l):
        v = torch.zeros(T, Lc, dtype=torch.bool, device="cuda")
        for t, p in enumerate(pos_l):
            if 0 < p <= Lc:
                v[t, min(pads[t % 4], p - 1):min(p, Lc)] = True  # a different left padding per tenant; nothing at or beyond its position
        return v

    live_results = {}
    for pos_l in ([0, 33, mid, Lc - 1], [31, 32, Lc - 1, mid]):
        pos_l = (pos_l * 3)[:T]
        valid0 = base_valid(pos_l)
        for p in set(pos_l):
            k_, v_, vl_ = kc0.clone(), vc0.clone(), valid0.clone()
            o_ = ops.decode_attention(qkv, cos, sin, k_, v_, vl_, torch.tensor([p], device="cuda"), heads, kvh)
            scalar[p] = (o_, k_, v_, vl_, bd._lib.lib().bd_last_attention_form())
        kc, vc, valid = kc0.clone(), vc0.clone(), valid0.clone()
        out, form, ws = _ragged_attention(qkv, cos, sin, kc, vc, valid, torch.tensor(pos_l, device="cuda"), act_all, heads, kvh)
        for t, p in enumerate(pos_l):
            o_, k_, v_, vl_, form_s = scalar[p]
            assert form == form_s, (hex(form), hex(form_s))      # the same instantiation and split count
            assert torch.equal(out[t], o_[t]), (t, p)
            assert torch.equal(kc[t], k_[t]) and torch.equal(vc[t], v_[t]) and torch.equal(valid[t], vl_[t]), (t, p)
            assert bool(valid[t, p]) and torch.equal(kc[t, :, :p], kc0[t, :, :p]) and torch.equal(kc[t, :, p + 1:], kc0[t, :, p + 1:])
        if ws is not None:
            assert int(ws[:16384].max()) == 0                    # tickets back at zero
        live_results[tuple(pos_l)] = (out, kc, vc, valid, valid0)
        nsplit, maxs = form & 0xff, (form >> 16) & 0xff
        assert (nsplit == 1) == (Lc < 256), hex(form)
        assert Lc < 256 or ((nsplit, maxs) == (4, 4) if T == 12 else (nsplit > 4 and maxs == 16)), hex(form)

    # tenants that stay out: tenant 1 inactive, tenant 2 at pos == Lc; then also tenant 0 at pos == -1.  Rows 0 / 3 (then 3) are as before.
    pos_l = ([0, 33, mid, Lc - 1] * 3)[:T]
    out_a, kc_a, vc_a, valid_a, valid0 = live_results[tuple(pos_l)]
    for extra in (False, True):
        pos2, act2 = list(pos_l), [True] * T
        act2[1], pos2[2] = False, Lc
        if extra:
            pos2[0] = -1
        dead = {1, 2} | ({0} if extra else set())
        kc, vc, valid = kc0.clone(), vc0.clone(), valid0.clone()
        out, _, ws = _ragged_attention(qkv, cos, sin, kc, vc, valid, torch.tensor(pos2, device="cuda"), torch.tensor(act2, device="cuda"), heads, kvh)
        for t in range(T):
            if t in dead:
                assert int(out[t].view(torch.int16).abs().max()) == 0, t                    # exactly zero (+0.0 bits)
                assert torch.equal(kc[t], kc0[t]) and torch.equal(vc[t], vc0[t]) and torch.equal(valid[t], valid0[t]), t
            else:
                assert torch.equal(out[t], out_a[t]) and torch.equal(kc[t], kc_a[t]) and torch.equal(vc[t], vc_a[t]), t
                assert torch.equal(valid[t], valid_a[t]), t
        if ws is not None:
            assert int(ws[:16384].max()) == 0


# ------------------------------------------------------------------------------------------------ 2. step kernels
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("T,V,H", [(1, 512, 64), (4, 1000, 256), (12, 512, 64)])
def test_ragged_step_kernels_follow_their_rules(bd, dtype, T, V, H):
    """bd_srv_step_begin_ragged / bd_srv_step_end_ragged against the rules of include/bitdelta_hip.h restated in torch, over several steps in a row:
    ties and NaNs in the logits, active and inactive tenants, a stop hit (tenants 0, 4, 8), n reaching limit (1, 5, 9), pos reaching Lc (2, 6, 10),
    tenants inactive from the start with garbage state (3, 7, 11), n beyond out_cap, tok outside the table.  Every buffer is compared exactly."""
    from bitdelta_amd import serving_ops as ops
    g = torch.Generator(device="cuda").manual_seed(T + V + H)
    embed = torch.randn(T, V, H, device="cuda", generator=g).to(dtype)
    Lc, ns, cap, STOP = 40, 3, 3, 123
    kind = [t % 4 for t in range(T)]
    st = dict(tok=torch.randint(0, V, (T, 1), device="cuda", generator=g),
              pos=torch.tensor([Lc - 3 if k == 2 else (Lc + 7 if k == 3 else 5 + t) for t, k in enumerate(kind)], device="cuda"),
              n=torch.ones(T, dtype=torch.long, device="cuda"),
              limit=torch.tensor([4 if k == 1 else 100 for k in kind], device="cuda"),
              active=torch.tensor([k != 3 for k in kind], device="cuda"),
              done=torch.zeros(T, dtype=torch.uint8, device="cuda"),
              out=torch.full((T, cap + 2), -7, dtype=torch.long, device="cuda"),
              valid=torch.zeros(T, Lc, dtype=torch.bool, device="cuda"))
    st["valid"][:, :5] = True
    stop_ids = torch.full((T, ns), -1, dtype=torch.long, device="cuda")
    stop_ids[[t for t in range(T) if kind[t] == 0], 1] = STOP
    out_view = st["out"][:, 1:1 + cap]                           # out_cap = 3 inside rows of 5: the margins must keep their -7
    ref = {k: v.clone() for k, v in st.items()}
    seen = set()
    for it in range(7):
        if it == 0:
            st["tok"][0, 0] = ref["tok"][0, 0] = V + 5            # device data outside the table: clamped
        if it == 3:
            st["tok"][0, 0] = ref["tok"][0, 0] = -3
        x = ops.step_begin_ragged(embed, st["tok"], st["valid"], st["pos"], st["active"])
        for t in range(T):
            p = int(ref["pos"][t])
            if bool(ref["active"][t]) and 0 <= p < Lc:
                assert torch.equal(x[t, 0], embed[t, min(max(int(ref["tok"][t, 0]), 0), V - 1)]), (it, t)
                ref["valid"][t, p] = True
            else:
                assert int(x[t].view(torch.int16).abs().max()) == 0, (it, t)
        assert torch.equal(st["valid"], ref["valid"]), it
        logits = torch.randn(T, V, device="cuda", generator=g).to(dtype)
        if it == 1:                                              # ties: the first maximum wins
            logits[:, [7, 3, V - 1]] = 100.0
        if it == 2:                                              # NaN beats everything, the first NaN wins
            logits[:, [V - 5, 11]] = float("nan")
        if it == 4:                                              # the winner is the stop token of tenants 0, 4, 8
            logits[:, STOP] = 50.0
        ops.step_end_ragged(logits, st["tok"], out_view, st["n"], st["pos"], st["limit"], stop_ids, st["active"], st["done"], Lc)
        nxt = torch.argmax(logits, dim=-1).tolist()
        for t in range(T):
            if not bool(ref["active"][t]):
                continue
            ref["tok"][t, 0] = nxt[t]
            n0 = int(ref["n"][t])
            if n0 < cap:
                ref["out"][t, 1 + n0] = nxt[t]
            else:
                seen.add("cap")
            ref["n"][t] += 1
            ref["pos"][t] += 1
            reason = (1 if nxt[t] in stop_ids[t].tolist() else 0) | (2 if int(ref["n"][t]) >= int(ref["limit"][t]) else 0) | \
                (4 if int(ref["pos"][t]) >= Lc else 0)
            if reason:
                ref["active"][t] = False
                ref["done"][t] = reason
                seen.add(reason)
        for k in st:
            assert torch.equal(st[k], ref[k]), (it, k, st[k], ref[k])
    assert not bool(st["active"].any()) and "cap" in seen and 1 in seen and (T == 1 or {2, 4} <= seen)
    assert int(st["done"][0]) == 1 and (T == 1 or (int(st["done"][1]) == 2 and int(st["done"][2]) == 4 and int(st["done"][3]) == 0))
    # the range guard of step_begin on its own: an ACTIVE tenant whose position left the cache gets a zero row and no mark
    for p_out in (Lc, -1):
        st["active"][0], st["pos"][0] = True, p_out
        x = ops.step_begin_ragged(embed, st["tok"], st["valid"], st["pos"], st["active"])
        assert int(x[0].view(torch.int16).abs().max()) == 0 and torch.equal(st["valid"], ref["valid"])


# ------------------------------------------------------------------------------------------------ 3. lockstep equivalence
@pytest.mark.parametrize("name,T,dtype", [("tiny128", 4, torch.float16), ("tiny2048", 3, torch.bfloat16)])
def test_session_in_lockstep_generates_what_generate_does(bd, name, T, dtype):
    """submit_all + run == generate, token for token, by graph replay and eagerly (tiny2048: the RMSNorm hand-off is on)"""
    from bitdelta_amd.serving_loop import TenantDecoder
    dec = TenantDecoder.synthetic(name, T, "cuda", dtype=dtype, seed=31, max_len=192, shared_heads=True)
    g = torch.Generator().manual_seed(9)
    prompts = [torch.randint(1, 500, (n,), generator=g).tolist() for n in (9, 64, 33, 70)[:T]]
    ref, n_ref = dec.generate(prompts, max_new_tokens=12, use_graph=True)
    assert n_ref == 12
    sess = dec.session()
    for use_graph in (True, False):
        sess.submit_all(prompts, max_new_tokens=12)
        assert sess.active() == [True] * T
        sess.run(use_graph=use_graph)
        for t in range(T):
            toks, reason = sess.result(t)
            assert reason == 2 and torch.equal(toks, ref[t]), (use_graph, t, toks, ref[t])
    ref2, _ = dec.generate(prompts, max_new_tokens=12, use_graph=True)        # ... and the lockstep path is as it was next to a session
    assert torch.equal(ref2, ref)


# ------------------------------------------------------------------------------------------------ 4. / 5. staggered admission
PLAN = [(0, 9, 10, 3), (2, 70, 8, 2), (1, 33, 6, None)]          # (tenant, prompt length, max_new_tokens, steps before the next admission)


def _prompts(lengths, seed=5):
    g = torch.Generator().manual_seed(seed)
    return {t: torch.randint(1, 500, (n,), generator=g).tolist() for t, n in lengths}


def _staggered(dec, plan, prompts):
    """the admissions of `plan` on one session; returns {tenant: (tokens, reason)}"""
    sess = dec.session()
    for t, _, mx, steps in plan:
        sess.submit(t, prompts[t], max_new_tokens=mx)
        if steps is None:
            sess.run()
        else:
            sess.step(steps)
    return sess, {t: sess.result(t) for t in range(dec.T)}


def _alone(dec, plan, prompts):
    res = {}
    for t, _, mx, _ in plan:
        sess = dec.session()                                     # a fresh session on the same decoder (and its one KV cache)
        sess.submit(t, prompts[t], max_new_tokens=mx)
        sess.run()
        assert sess.active() == [False] * dec.T
        res[t] = sess.result(t)
    return res


def _teacher_forced_truth(bd, dec, t, prompt, toks):
    """tests/test_gpu_serving.py's rule against tenant t's dense fp32 model, on the tenant's OWN padded ids and mask"""
    from test_gpu_serving import _dense_reference_logits
    from bitdelta_amd.serving_loop import padded_length
    L = padded_length(len(prompt))
    seq = torch.zeros(L, dtype=torch.long, device="cuda")
    msk = torch.zeros(L, dtype=torch.bool, device="cuda")
    seq[L - len(prompt):] = torch.tensor(prompt, device="cuda")
    msk[L - len(prompt):] = True
    for s_, tok in enumerate(toks.tolist()):
        ref = _dense_reference_logits(bd, dec, t, seq, msk)
        top2 = ref.topk(2).values
        if (top2[0] - top2[1]).item() > 0.05:
            assert tok == int(ref.argmax()), (t, s_)
        else:
            assert ref[tok] >= top2[0] - 0.1, (t, s_)
        seq = torch.cat([seq, torch.tensor([tok], device="cuda")])
        msk = torch.cat([msk, torch.tensor([True], device="cuda")])


@pytest.fixture(scope="module")
def staggered128(bd):
    from bitdelta_amd.serving_loop import TenantDecoder
    dec = TenantDecoder.synthetic("tiny128", 4, "cuda", dtype=torch.float16, seed=31, max_len=256)
    prompts = _prompts([(t, n) for t, n, _, _ in PLAN])
    sess, res = _staggered(dec, PLAN, prompts)
    return dec, prompts, sess, res


def _check_independence(dec, prompts, sess, res):
    alone = _alone(dec, PLAN, prompts)
    for t, _, mx, _ in PLAN:
        assert res[t][1] == 2 and alone[t][1] == 2 and res[t][0].numel() == mx
        assert torch.equal(res[t][0], alone[t][0]), (t, res[t][0], alone[t][0])
    assert res[3][0].numel() == 0 and res[3][1] == 0              # tenant 3 never submitted


def test_staggered_tenants_generate_what_they_generate_alone(bd, staggered128):
    dec, prompts, sess, res = staggered128
    assert not bool(sess.cache["valid"][3].any()) and int(sess.cache["k"][0][3].abs().max()) == 0     # tenant 3's rows: never touched
    assert int(sess.pos[0]) == 64 + 9 and int(sess.pos[2]) == 128 + 7 and int(sess.pos[1]) == 64 + 5
    _check_independence(dec, prompts, sess, res)


def test_staggered_tenants_on_an_int8_base(bd):
    from bitdelta_amd.serving_loop import TenantDecoder
    dec = TenantDecoder.synthetic("tiny128", 4, "cuda", dtype=torch.float16, seed=31, max_len=256, base_int8=True)
    prompts = _prompts([(t, n) for t, n, _, _ in PLAN])
    sess, res = _staggered(dec, PLAN, prompts)
    _check_independence(dec, prompts, sess, res)


def test_one_tenant_prefill_views_share_storage(bd, staggered128):
    """tenant_view(t) / cache_view(cache, t): the parent's storage offset by the tenant, no copy of a weight, a mask or a cache"""
    dec, _, sess, _ = staggered128
    t = 2
    v, cv = dec.tenant_view(t), dec.cache_view(sess.cache, t)
    assert v.T == 1 and len(v.layers) == len(dec.layers)

    def at(view, parent, rows=t):
        return view.data_ptr() == parent.data_ptr() + rows * parent.stride(0) * parent.element_size() and view.shape[1:] == parent.shape[1:] and \
            view.shape[0] == 1
    for lv, lp in zip(v.layers, dec.layers):
        for name in ("qkv", "o", "gate_up", "down"):
            fv, fp = getattr(lv, name), getattr(lp, name)
            assert fv.weight.data_ptr() == fp.weight.data_ptr() and fv.weight.shape == fp.weight.shape
            assert at(fv.mask, fp.mask) and at(fv.alpha, fp.alpha)
            assert (fv.alpha_pair is None) == (fp.alpha_pair is None) and (fp.alpha_pair is None or at(fv.alpha_pair, fp.alpha_pair))
            assert fv.mask_packed is None and fv.weight_tiled is None
        assert at(lv.norm1, lp.norm1) and at(lv.norm2, lp.norm2)
    assert at(v.embed, dec.embed) and at(v.final_norm, dec.final_norm) and at(v.lm_head, dec.lm_head)
    assert v.cos.data_ptr() == dec.cos.data_ptr() and v.sin.data_ptr() == dec.sin.data_ptr()
    for li in range(len(dec.layers)):
        assert at(cv["k"][li], sess.cache["k"][li]) and at(cv["v"][li], sess.cache["v"][li])
    assert at(cv["valid"], sess.cache["valid"])
    assert dec.tenant_view(t) is v                               # made once


def test_staggered_tokens_agree_with_dense_models(bd, staggered128):
    dec, prompts, _, res = staggered128
    for t, _, _, _ in PLAN:
        _teacher_forced_truth(bd, dec, t, prompts[t], res[t][0])


def test_staggered_full_width_layer_agrees_with_dense_models(bd):
    """one Mistral-7B layer, 6 tenants: three tenants admitted two steps apart, three steps each (the first token comes from the prefill)"""
    from bitdelta_amd.serving_loop import TenantDecoder
    dec = TenantDecoder.synthetic("mistral-1layer", 6, "cuda", dtype=torch.float16, seed=21, max_len=192)
    plan = [(0, 9, 4, 2), (3, 64, 4, 2), (5, 33, 4, None)]
    prompts = _prompts([(t, n) for t, n, _, _ in plan], seed=2)
    sess, res = _staggered(dec, plan, prompts)
    for t, _, mx, _ in plan:
        assert res[t][1] == 2 and res[t][0].numel() == mx
        _teacher_forced_truth(bd, dec, t, prompts[t], res[t][0])
    for t in (1, 2, 4):
        assert res[t][0].numel() == 0 and not bool(sess.cache["valid"][t].any())


# ------------------------------------------------------------------------------------------------ 6. lifecycle
def test_session_lifecycle(bd):
    from bitdelta_amd.serving_loop import TenantDecoder
    T = 4
    dec = TenantDecoder.synthetic("tiny128", T, "cuda", dtype=torch.float16, seed=33, max_len=192, shared_heads=True)
    prompts = _prompts([(0, 12), (1, 40), (2, 7)], seed=4)
    sess = dec.session()
    for t in range(3):
        sess.submit(t, prompts[t], max_new_tokens=8)
    with pytest.raises(RuntimeError):
        sess.submit(1, prompts[1])                               # still generating
    sess.run()
    base = [sess.result(t) for t in range(3)]
    assert all(r == 2 and tk.numel() == 8 for tk, r in base)     # max_new_tokens ends with reason 2
    # a stop id ends ITS tenant at that token, the others go on
    stop = int(base[0][0][3])
    first = base[0][0].tolist().index(stop)
    for t in range(3):
        sess.submit(t, prompts[t], max_new_tokens=8, stop_token_ids=[stop, 100000] if t == 0 else ())      # (re-submission to finished tenants)
    sess.run()
    toks0, r0 = sess.result(0)
    assert torch.equal(toks0, base[0][0][:first + 1]) and r0 == (1 | (2 if first + 1 >= 8 else 0)) and first + 1 < 8
    for t in (1, 2):
        assert torch.equal(sess.result(t)[0], base[t][0]) and sess.result(t)[1] == 2
    # a first token that already stops the tenant; max_new_tokens == 1
    sess.submit(1, prompts[1], max_new_tokens=8, stop_token_ids=[int(base[1][0][0])])
    sess.submit(2, prompts[2], max_new_tokens=1)
    assert sess.active() == [False] * T
    assert sess.result(1)[1] == 1 and sess.result(1)[0].tolist() == base[1][0][:1].tolist()
    assert sess.result(2)[1] == 2 and sess.result(2)[0].tolist() == base[2][0][:1].tolist()
    sess.run()                                                   # nothing to do
    # re-submitting to a finished tenant reproduces its first run
    sess.submit(0, prompts[0], max_new_tokens=8)
    sess.run()
    assert torch.equal(sess.result(0)[0], base[0][0]) and sess.result(0)[1] == 2
    with pytest.raises(ValueError):
        sess.submit(0, list(range(1, 1100)))                     # the reference's refusal, per tenant
    with pytest.raises(ValueError):
        sess.submit(0, prompts[0], stop_token_ids=list(range(9)))


def test_session_ends_a_tenant_at_the_end_of_its_cache(bd):
    """max_len = 66, a prompt padded to 64: the first token comes from the prefill, two steps fill rows 64 and 65, reason 4 -- and nothing is written
    beyond the tenant's cache rows or beyond `out` (a poisoned margin around it)"""
    from bitdelta_amd.serving_loop import TenantDecoder
    T, POISON = 4, 0x7F7F7F7F7F7F7F7F
    dec = TenantDecoder.synthetic("tiny128", T, "cuda", dtype=torch.float16, seed=33, max_len=66, shared_heads=True)
    sess = dec.session()
    cap = sess.out.shape[1]
    big = torch.full((T + 2, cap + 16), POISON, dtype=torch.long, device="cuda")
    sess.out = big[1:T + 1, 8:8 + cap]                           # before the first step: the captured graph holds this view's address
    sess.out.zero_()
    prompt = _prompts([(2, 50)], seed=6)[2]
    sess.submit(2, prompt, max_new_tokens=50)
    sess.run()
    toks, reason = sess.result(2)
    assert reason == 4 and toks.numel() == 3 and int(sess.pos[2]) == 66 and int(sess.n[2]) == 3
    assert sess.active() == [False] * T
    snap = [sess.cache["k"][0].clone(), sess.cache["v"][0].clone(), sess.cache["valid"].clone(), big.clone()]
    sess.step(2)                                                 # nobody is active: nothing moves
    sess.step(1, use_graph=False)
    for a, b in zip(snap, [sess.cache["k"][0], sess.cache["v"][0], sess.cache["valid"], big]):
        assert torch.equal(a, b)
    assert int(sess.pos[2]) == 66
    for t in (0, 1, 3):                                          # a write past row 65 of tenant 2 would land in tenant 3's rows
        for li in range(len(dec.layers)):
            assert int(sess.cache["k"][li][t].abs().max()) == 0 and int(sess.cache["v"][li][t].abs().max()) == 0
        assert not bool(sess.cache["valid"][t].any())
    assert bool(sess.cache["valid"][2, 64:66].all())
    keep = sess.out.clone()
    sess.out.fill_(POISON)
    assert bool((big == POISON).all())                           # no store outside [T, cap]
    sess.out.copy_(keep)


def test_session_refuses_what_it_cannot_run(bd):
    from bitdelta_amd.serving_loop import TenantDecoder
    dec = TenantDecoder.synthetic("tiny", 2, "cuda", dtype=torch.float16, seed=1, max_len=128)          # head_dim 64: no HIP decode attention
    with pytest.raises(ValueError):
        dec.session()
    dec = TenantDecoder.synthetic("tiny128", 2, "cuda", dtype=torch.float16, seed=1, max_len=128, shared_heads=True)
    for switch, val in (("fast_glue", False), ("step_kernels", False), ("prefetch_o", True)):
        old = getattr(dec, switch)
        setattr(dec, switch, val)
        with pytest.raises(ValueError):
            dec.session()
        setattr(dec, switch, old)
    assert dec.session(max_stop_ids=4).stop_ids.shape == (2, 4)
