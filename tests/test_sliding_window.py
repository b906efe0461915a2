"""Sliding-window attention (include/bitdelta_hip.h): the query at position i sees key j iff j <= i, i - j < W, j >= kv_start (prefill) and valid[j]
(decode).  Reference: plain fp64 attention with a boolean mask built from that sentence.  Acceptance rules (tests/test_gpu_attention_exact.py derives
them): uniform weights (Q = 0, K large noise, V = 0 / 1 codes of the key index) give an exact count quotient, gate 1 ulp of the output dtype; randn
inputs are held per element to |got - ref| <= c * 2u * (P_ref . |V|) + tiny, c = 1 (that module's RANGE_C, measured against stock SDPA; not re-fitted)."""
import math

import pytest
import torch

gpu = pytest.mark.gpu
HD, DEV = 128, "cuda"
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
U_TINY = {torch.float16: (2.0 ** -11, 2.0 ** -24), torch.bfloat16: (2.0 ** -8, 2.0 ** -133)}      # unit roundoff u, smallest subnormal
CHUNKS = [(70, 1), (70, 17), (200, 130)]                     # (q0, Sq) of the cached form, Lc = 330
bits = lambda x: x.contiguous().view(torch.int16)


def ulps(a, b):
    mono = lambda x: torch.where((i := bits(x).to(torch.int32)) < 0, -(i & 0x7FFF), i)
    return (mono(a) - mono(b)).abs()


def codes(n, dtype):                                         # [n, 128] of 0 / 1: dims 0..63 one-hot of key % 64, dims 64..127 of (key // 64) % 64
    key, v = torch.arange(n, device=DEV), torch.zeros(n, HD, device=DEV)
    v[key, key % 64] = 1
    v[key, 64 + (key // 64) % 64] = 1
    return v.to(dtype)


def ref(q, k, v, qpos, W, ok):
    """fp64 attention of q [B, heads, R, 128] at positions qpos [R] or [B, R] over k / v [B, kv heads, N, 128]; ok [B, 1, 1, N]: keys that are valid /
    not below kv_start.  Rows that see nothing -> 0.  Returns (P . V, P . |V|) as [B, R, heads * 128]."""
    j, qp = torch.arange(k.shape[2], device=DEV), qpos[..., None]
    ok = ok & ((j <= qp) & (qp - j < W)).view(-1, 1, qp.shape[-2], k.shape[2])
    kd, vd = (x.double().repeat_interleave(q.shape[1] // k.shape[1], dim=1) for x in (k, v))
    p = torch.softmax((q.double() @ kd.transpose(2, 3) / math.sqrt(HD)).masked_fill(~ok, float("-inf")), dim=-1).nan_to_num(0.0)
    return tuple((p @ x).transpose(1, 2).flatten(2) for x in (vd, vd.abs()))


def run_prefill(dtype, uniform, form, W, S=256, Lc=330, H=4):
    """B = 2, kv_start = [0, 37], G = 4.  form None: the whole prompt; (q0, Sq): that chunk over caches [B, 1, Lc, 128] whose rows at and past
    q0 + Sq are NaN.  Returns (out, fp64 reference, P . |V|, rows that are no pads [B, R, 1])."""
    from bitdelta_amd import serving_ops as ops
    g = torch.Generator(device=DEV).manual_seed(1)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    kst = torch.tensor([0, 37], dtype=torch.int32, device=DEV)
    q0, Sq = form or (0, S)
    qpos, n = torch.arange(q0, q0 + Sq, device=DEV), q0 + Sq       # n keys exist; every form takes the first rows of the same 384-row draw
    q = (torch.zeros(2, 384, H, HD, device=DEV, dtype=dtype) if uniform else rn(2, 384, H, HD).to(dtype))[:, :n]
    k = (rn(2, 384, 1, HD) * (50 if uniform else 1)).to(dtype)[:, :n]
    v = (codes(384, dtype)[None, :, None].expand(2, 384, 1, HD).contiguous() if uniform else rn(2, 384, 1, HD).to(dtype))[:, :n]
    if form is None:
        out = ops.prefill_attention(q, k, v, kv_start=kst, window=W)
    else:
        kc, vc = (torch.cat([x.transpose(1, 2), torch.full((2, 1, Lc - n, HD), float("nan"), device=DEV, dtype=dtype)], 2) for x in (k, v))
        out = ops.prefill_attention_cached(q[:, qpos], kc, vc, q0, kv_start=kst, window=W)
    ok = (torch.arange(n, device=DEV) >= kst[:, None].long())[:, None, None]
    return (out,) + ref(q[:, qpos].transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), qpos, W or n, ok) + ((qpos >= kst[:, None].long())[..., None],)


@gpu
@DTYPES
@pytest.mark.parametrize("form,W", [(None, W) for W in (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 256, 300)] +
                         [(c, W) for c in CHUNKS for W in (1, 33, 64, 129, 300)], ids=str)
def test_prefill_rows_see_their_window(form, W, dtype):
    """class 1, both prefill forms: finite and count_in_bin / count_visible within 1 ulp; only the pad rows i < kv_start[b] are left out"""
    out, want, _, keep = run_prefill(dtype, True, form, W)
    d = ulps(out, want.to(dtype)) * keep
    assert bool(torch.isfinite(out).all()) and int(d.max()) <= 1, f"row {int(d.amax((0, 2)).argmax())} of the launch"


def run_decode(dtype, uniform, T, G, Lc, pos, active, W, valid):
    """kv heads = 1.  pos: an int (lockstep form, active None) or one per tenant (ragged).  The windowed launch and the existing entry run on clones
    of the same caches and must leave the same cache and valid bits.  Returns (out, the existing entry's out, fp64 reference, P . |V|)."""
    from bitdelta_amd import serving_ops as ops
    from bitdelta_amd.serving_loop import _rope, _rope_tables
    g = torch.Generator(device=DEV).manual_seed(Lc + G)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    cos, sin = _rope_tables(Lc, HD, DEV, dtype)
    pt = torch.tensor(pos, device=DEV).reshape(-1)
    pe = pt.expand(T)
    qkv = (rn(T, 1, (G + 2) * HD) * (50 if uniform else 1)).to(dtype)
    kc, vc = (rn(T, 1, Lc, HD) * (50 if uniform else 1)).to(dtype), rn(T, 1, Lc, HD).to(dtype)
    if uniform:                                               # q = 0 (RoPE of 0 is 0); every cache row and the new token's v carry their index code
        qkv[..., :G * HD] = 0
        vc = codes(Lc, dtype)[None, None].expand(T, 1, Lc, HD).contiguous()
        qkv[:, 0, (G + 1) * HD:] = vc[0, 0, pe]
    act = None if active is None else torch.tensor(active, device=DEV)
    def launch(w, c):
        return (ops.decode_attention(qkv, cos, sin, *c, pt, G, 1, window=w) if act is None else
                ops.decode_attention_ragged(qkv, cos, sin, *c, pt, act, G, 1, window=w),) + c
    # (the windowed launch last: bd_last_attention_form() is then its form)
    (out0, k0, v0, m0), (out, k1, v1, m1) = (launch(w, (kc.clone(), vc.clone(), valid.clone())) for w in (None, W))
    assert torch.equal(bits(k1), bits(k0)) and torch.equal(bits(v1), bits(v0)) and torch.equal(m1, m0), "cache append / valid mark"
    qr = _rope(qkv[..., :G * HD].view(T, 1, G, HD).transpose(1, 2), cos[pe][:, None, None], sin[pe][:, None, None])
    ok = m1[:, None, None, :] if act is None else m1[:, None, None, :] & act.view(T, 1, 1, 1)
    return (out, out0) + ref(qr, k1, v1, pe[:, None], W, ok)


@gpu
@DTYPES
@pytest.mark.parametrize("form", ["ragged", "inactive", "lockstep", "long"])
@pytest.mark.parametrize("G", [1, 4, 8])
def test_decode_rows_see_their_window(G, form, dtype):
    """class 1, decode.  T = 2, Lc = 320: left pads and holes in valid inside and outside every window, splits that come out empty, an inactive
    tenant (zeros out, no append).  long: T = 1, Lc = 2304, where W > 2048 runs the DEPTH-4, 16-split form over a window that starts at row 204."""
    from bitdelta_amd import _lib
    T, Lc, pos, active = {"ragged": (2, 320, [300, 45], [True, True]), "inactive": (2, 320, [300, 45], [True, False]),
                          "lockstep": (2, 320, 300, None), "long": (1, 2304, 2303, None)}[form]
    l = torch.arange(Lc, device=DEV)
    valid = ((l >= 5) & (l % 7 != 3) & (l != 299) & (l != 44))[None] & (l[None] < torch.tensor(pos, device=DEV).reshape(-1, 1).expand(T, 1))
    for W in ([100, 2100, 4096] if form == "long" else [1, 2, 31, 32, 33, 64, 100, 257, 320, 1000]):
        out, _, want, _ = run_decode(dtype, True, T, G, Lc, pos, active, W, valid)
        f = _lib.lib().bd_last_attention_form()
        assert f >> 16 & 0xff == 16 and (form != "long" or f & 0xffff == (1 | 2 << 8 if W == 100 else 16 | 4 << 8)), f"W={W}: form {f:#x}"
        assert int(ulps(out, want.to(dtype)).max()) <= 1, f"W={W}"


@gpu
@DTYPES
def test_wide_windows_chunks_and_rows_that_start_masked(dtype):
    """class 2: W >= the key range is the existing entry bit for bit; the cached windowed form is the whole-prompt windowed form row for row.
    class 3, randn, W = 100 (S = 256, a chunk, decode at pos = 300): rows whose first tiles / ring rows are masked, per element within 2u P|V| + tiny"""
    pf = lambda form, W, **kw: run_prefill(dtype, False, form, W, **kw)
    whole, full = pf(None, 100, S=384)[0], pf(None, None)[0]
    assert torch.equal(bits(pf(None, 256)[0]), bits(full))
    for c in CHUNKS:
        assert torch.equal(bits(pf(c, 100)[0]), bits(whole[:, c[0]:sum(c)])) and torch.equal(bits(pf(c, 330)[0]), bits(pf(c, None)[0]))
    valid = torch.arange(320, device=DEV)[None] < torch.tensor([[300], [45]], device=DEV)
    for pos, active in (([300, 45], [True, True]), (45, None)):
        out, out0, _, _ = run_decode(dtype, False, 2, 4, 320, pos, active, 320, valid)
        assert torch.equal(bits(out), bits(out0))
    d = run_decode(dtype, False, 2, 4, 320, 300, None, 100, valid[:1].expand(2, 320).contiguous())
    for out, want, absv in (pf(None, 100)[:3], pf((200, 56), 100)[:3], (d[0], d[2], d[3])):
        assert bool(((out.double() - want).abs() <= 2 * U_TINY[dtype][0] * absv + U_TINY[dtype][1]).all())


@gpu
def test_a_windowed_decoder_forgets_what_left_its_window():
    """class 4: one layer, W = 48: position i depends on tokens i - 47 .. i only, through prefill, 8 session steps and an extend of 20 tokens"""
    from bitdelta_amd.serving_loop import TenantDecoder
    g = torch.Generator().manual_seed(7)
    a, ext = torch.randint(1, 512, (200,), generator=g).tolist(), torch.randint(1, 512, (20,), generator=g).tolist()
    far = [(t + 1) % 511 + 1 for t in a[:100]] + a[100:]           # differs from a in each of its first 100 tokens
    edge = a[:152] + [a[152] % 511 + 1] + a[153:]                  # differs in the token 47 back from the last one
    turn = lambda s, admit, tokens, n: (admit(0, tokens, max_new_tokens=n), s.run(), s.result(0)[0].tolist())[2]

    def run(dec, s, prompt):                                       # (first-token logits, the 9 tokens of the turn + the 4 after the extend)
        logits = dec.prefill(*dec.prepare([prompt]), dec.new_cache()).clone()
        return logits, turn(s, s.submit, prompt, 9) + turn(s, s.extend, ext, 4)
    dec, full = (TenantDecoder.synthetic((1024, 2048, 1, 8, 2, 512), 1, DEV, max_len=320, sliding_window=w) for w in (48, None))
    s, sf = dec.session(), full.session()
    (la, ta), (lf, tf), (le, _) = run(dec, s, a), run(dec, s, far), run(dec, s, edge)
    assert torch.equal(la, lf) and ta == tf and len(ta) == 13 and not torch.equal(la, le)
    assert not torch.equal(run(full, sf, a)[0], run(full, sf, far)[0])


def test_the_entries_refuse_a_window_below_one_and_what_they_do_not_cover():
    """class 5, host only: an empty call (T = 0 / B = 0) is BD_OK with a window and BD_E_BAD_SHAPE (-5) with one < 1; fp8 and causal=False take none"""
    from bitdelta_amd import _lib, serving_ops as ops
    from bitdelta_amd.serving_loop import TenantDecoder
    L, n = _lib.lib(), None
    for w, code in ((0, -5), (-4096, -5), (1, 0)):
        assert L.bd_srv_decode_attention_window(n, n, n, 0, n, n, n, n, n, n, 0, 4, 1, 128, 64, 768, 512, 0, w, n, 0, n) == code
        assert L.bd_srv_prefill_attention_window(n, n, n, n, 0, 64, 4, 1, 128, 8, 8, 8, 8, 8, 8, 8, 8, n, 1.0, w, 0, n) == code
        assert L.bd_srv_prefill_attention_cached_window(n, n, n, n, 0, 1, 4, 1, 128, 0, 64, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, n, 1.0, w, 0, n) == code
    with pytest.raises(ValueError, match="bd_srv_decode_attention_kv8"):
        TenantDecoder((1024, 2048, 1, 8, 2, 512), 1, "cpu", torch.float16, kv_cache="fp8", sliding_window=48)
    x = torch.zeros(1, 64, 1, 128, dtype=torch.float16)
    with pytest.raises(ValueError, match="causal"):
        ops.prefill_attention(x, x, x, causal=False, window=8)
