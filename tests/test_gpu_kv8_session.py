"""TenantDecoder(kv_cache="fp8") through a session: submit, 6 steps, retire, extend by 5 tokens, 3 more steps -- a one-layer decoder (hidden 256, 2
heads of 128, 3 tenants, random per-tenant cache scales).  After every step each tenant's logits are compared with a dense fp64 twin of that tenant that computes everything itself except K / V: those are
the session's own cache bytes after the step, dequantised with the tenant's scales (rounding flips at e4m3 boundaries stay out of the comparison;
tests/test_gpu_kv8_kernels.py pins the bytes).  Bound: relerr <= 3e-3, the one-layer bound of tests/test_gpu_serving.py.  A scale applied to the
wrong tenant, head, layer or side is an error of tens of percent."""
import pytest
import torch

pytestmark = pytest.mark.gpu
CFG, T = (256, 512, 1, 2, 2, 512), 3          # (hidden, intermediate, layers, heads, kv heads, vocabulary), tenants


def scales(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return tuple(0.25 + 3.75 * torch.rand(*shape, generator=g) for _ in range(2))


def twin_logits(dec, cache, t, tok, pos):
    """tenant t's one-layer model in fp64 on token `tok` at cache row `pos`, attending over the cache bytes as they stand (valid rows <= pos)"""
    import bitdelta_amd as bd
    import torch.nn.functional as F
    from bitdelta_amd.serving_loop import _rope
    hid, inter, _, heads, kvh, _ = dec.cfg
    layer, f64 = dec.layers[0], torch.float64

    def merged(fl):                                       # the delta merged into the base weight: W + alpha * S^T
        return fl.weight.to(f64) + fl.column_alpha(t).to(f64)[:, None] * (bd.unpack(fl.mask[t]).to(f64) * 2 - 1).T

    def rms(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + dec.eps) * w.to(f64)

    lut = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(f64).to(dec.dev)
    K = lut[cache["k"][0][t].view(torch.uint8).long()] * cache["k_scale"][0][t].to(f64)[:, None, None]       # [kvh, Lc, 128]
    V = lut[cache["v"][0][t].view(torch.uint8).long()] * cache["v_scale"][0][t].to(f64)[:, None, None]
    x = dec.embed[t][tok].to(f64)
    q = layer.qkv.split(rms(x, layer.norm1[t]) @ merged(layer.qkv).T)[0]
    cos, sin = (dec.cos[t], dec.sin[t]) if dec.rope_per_tenant else (dec.cos, dec.sin)
    q = _rope(q.view(1, 1, heads, 128).transpose(1, 2), cos[pos:pos + 1].to(f64), sin[pos:pos + 1].to(f64))[0, :, 0]      # [heads, 128]
    rep = heads // kvh
    s = torch.einsum("hd,hld->hl", q, K.repeat_interleave(rep, 0)) / 128 ** 0.5
    ok = cache["valid"][t] & (torch.arange(s.shape[1], device=dec.dev) <= pos)
    a = torch.einsum("hl,hld->hd", s.masked_fill(~ok[None], float("-inf")).softmax(-1), V.repeat_interleave(rep, 0)).reshape(-1)
    x = x + a @ merged(layer.o).T
    g, u = layer.gate_up.split(rms(x, layer.norm2[t]) @ merged(layer.gate_up).T)
    x = x + (F.silu(g) * u) @ merged(layer.down).T
    return rms(x, dec.final_norm[t]) @ dec.lm_head[t].to(f64).T


def test_session_logits_follow_the_fp64_twin_over_its_own_bytes(monkeypatch):
    from test_gpu_serving import relerr
    from bitdelta_amd import serving_ops as ops
    from bitdelta_amd.serving_loop import TenantDecoder
    ks, vs = scales(5, 1, T, 2)
    dec = TenantDecoder.synthetic(CFG, T, "cuda", dtype=torch.float16, seed=41, max_len=128, kv_cache="fp8", kv_scales=(ks, vs))
    seen, orig = [], ops.step_end_ragged
    monkeypatch.setattr(ops, "step_end_ragged", lambda logits, *a, **kw: (seen.append(logits.clone()), orig(logits, *a, **kw))[1])
    sess = dec.session()
    cache = sess.cache
    assert cache["k"][0].dtype == torch.float8_e4m3fn and cache["k"][0].shape == (T, 2, 128, 128)
    assert torch.equal(cache["k_scale"][0].cpu(), ks[0]) and torch.equal(cache["v_inv"][0].cpu(), 1.0 / vs[0])
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(1, 500, (n,), generator=g).tolist() for n in (9, 30, 64)]

    def stepped(n):
        for _ in range(n):
            tok, pos, act = sess.tok[:, 0].tolist(), sess.pos.tolist(), sess.active_flags.tolist()
            sess.step(1, use_graph=False)
            for t in range(T):
                if act[t]:
                    err = relerr(seen[-1][t], twin_logits(dec, cache, t, tok[t], pos[t]))
                    print(f"KV8 session tenant {t} pos {pos[t]}: relerr {err:.2e}")
                    assert err <= 3e-3, (t, pos[t], err)

    for t in range(T):
        sess.submit(t, prompts[t], max_new_tokens=7)
    stepped(6)
    assert not any(sess.active()) and len(seen) == 6
    more = torch.randint(1, 500, (5,), generator=g).tolist()
    P = int(sess.pos[1])
    sess.extend(1, more, max_new_tokens=4)
    # the chunk's last row: its logits chose the turn's first token; the twin sees the history through the bytes (the kernel through one more rounding)
    ref = twin_logits(dec, cache, 1, more[-1], P + 5)
    top2 = ref.topk(2).values
    assert int(sess.tok[1, 0]) == int(ref.argmax()) if float(top2[0] - top2[1]) > 0.05 else float(ref[int(sess.tok[1, 0])]) >= float(top2[0]) - 0.1
    stepped(3)
    assert len(seen) == 9 and not any(sess.active())


def test_one_captured_graph_serves_a_scale_reload_and_refusals():
    from bitdelta_amd.serving_loop import TenantDecoder, kv_scales_from_cache
    dec = TenantDecoder.synthetic(CFG, T, "cuda", dtype=torch.float16, seed=42, max_len=128, kv_cache="fp8")
    prompt = list(range(1, 20))

    def turn(sess, use_graph):
        sess.submit(0, prompt, max_new_tokens=5)
        sess.run(use_graph=use_graph)
        return sess.result(0)[0].clone()
    sess = dec.session()
    turn(sess, True)
    graphs = dict(sess._graphs)
    assert len(graphs) == 1 and "fp8" in next(iter(graphs))
    k2, v2 = scales(9, 1, 2)
    from test_gpu_session_extend import _clone_state
    sess.load_tenant(0, _clone_state(dec.tenant_state(0)), kv_scales=(k2, v2))
    assert torch.equal(sess.cache["k_scale"][0][0].cpu(), k2[0]) and torch.equal(sess.cache["v_inv"][0][0].cpu(), 1.0 / v2[0]) and bool((sess.cache["k_scale"][0][1:] == 1).all())
    replayed = turn(sess, True)
    assert sess._graphs == graphs and torch.equal(replayed, turn(sess, False)), "the graph captured before the reload reads the new scales"
    # a default decoder is what it was; calibration gives scales of the cache's shape
    d16 = TenantDecoder.synthetic(CFG, T, "cuda", dtype=torch.float16, seed=42, max_len=128)
    c16 = d16.new_cache()
    assert c16["k"][0].dtype == torch.float16 and "k_scale" not in c16 and dec.new_cache(kv_cache=None)["k"][0].dtype == torch.float16
    ids, am = d16.prepare([prompt] * T)
    d16.prefill(ids, am, c16)
    kc, vc = kv_scales_from_cache(c16)
    assert kc.shape == (1, T, 2) and torch.allclose(kc[0, 0], c16["k"][0][0, :, 45:64].float().abs().amax(dim=(1, 2)).cpu() / 448)
    for refused in (lambda: TenantDecoder.synthetic(CFG, T, "cuda", dtype=torch.float16, kv_cache="int4"),
                    lambda: TenantDecoder.synthetic("tiny", T, "cuda", dtype=torch.float16, kv_cache="fp8"),          # head_dim 64
                    lambda: d16.load_tenant(0, _clone_state(d16.tenant_state(0)), kv_scales=(k2, v2))):
        with pytest.raises(ValueError):
            refused()
    dec.prefetch_o = True
    with pytest.raises(ValueError):
        dec.session()
    dec.prefetch_o, dec.hip_prefill_attention = False, False
    with pytest.raises(RuntimeError):
        dec.prefill(ids, am, dec.new_cache())
