"""ctypes wrappers of the decode-step glue kernels (csrc/bd_serving.h): per-tenant RMSNorm, SwiGLU on the fused gate|up output,
and single-token attention with RoPE + KV-cache append.  Callers of the hot path, used by serving_loop.TenantDecoder at decode;
each has a stock-torch equivalent in that module (used at prefill and as the test reference)."""
import torch

from ._lib import DTYPE_CODE, check, lib, ptr, require_gpu, stream_ptr, workspace


def rmsnorm_tenant(x, w, eps):
    """x [T, M, H], w [T, H] -> w[t] * round(x * rsqrt(mean(x^2) + eps))   (HF RMSNorm, tenant t's weight for row block t)"""
    require_gpu(x, w)
    T, M, H = x.shape
    assert w.shape == (T, H) and w.dtype == x.dtype and x.stride(2) == 1 and w.stride(1) == 1
    assert T == 1 or x.stride(0) == M * x.stride(1), "rows must be evenly strided"
    y = torch.empty((T, M, H), device=x.device, dtype=x.dtype)
    with torch.cuda.device(x.device):
        check(lib().bd_srv_rmsnorm(ptr(x), ptr(w), ptr(y), T * M, H, x.stride(1), H, w.stride(0), M, float(eps),
                                   DTYPE_CODE[x.dtype], stream_ptr()), "srv_rmsnorm")
    return y


def add_rmsnorm(resid, y32, w, eps):
    """(x, h) with x = resid + y32.to(resid.dtype) and h = rmsnorm_tenant(x, w, eps), in ONE launch and with exactly those ops' roundings.
    resid [T, M, H] 16-bit, y32 [T, M, H] fp32 (a row-parallel Linear's reduced partial sums), w [T, H]."""
    require_gpu(resid, y32, w)
    T, M, H = resid.shape
    assert y32.shape == resid.shape and y32.dtype == torch.float32 and w.shape == (T, H) and w.dtype == resid.dtype
    assert resid.stride(2) == 1 and y32.stride(2) == 1 and w.stride(1) == 1 and H % 8 == 0 and H <= 8192
    assert T == 1 or (resid.stride(0) == M * resid.stride(1) and y32.stride(0) == M * y32.stride(1)), "rows must be evenly strided"
    x = torch.empty((T, M, H), device=resid.device, dtype=resid.dtype)
    h = torch.empty((T, M, H), device=resid.device, dtype=resid.dtype)
    with torch.cuda.device(resid.device):
        check(lib().bd_srv_add_rmsnorm(ptr(resid), ptr(y32), ptr(w), ptr(x), ptr(h), T * M, H, resid.stride(1), y32.stride(1), H, H, w.stride(0), M,
                                       float(eps), DTYPE_CODE[resid.dtype], stream_ptr()), "srv_add_rmsnorm")
    return x, h


def swiglu(gu, inter):
    """gu [T, M, 2*inter] (gate columns, then up columns) -> round(silu(gate)) * up, [T, M, inter]"""
    assert gu.shape[2] == 2 * inter
    return swiglu2(gu[..., :inter], gu[..., inter:])


def swiglu2(g, u):
    """g, u [B, S, I] (views allowed: last dim contiguous, rows evenly strided) -> round(silu(g)) * u as a new [B, S, I] tensor"""
    require_gpu(g, u)
    B, S, I = g.shape
    assert u.shape == g.shape and u.dtype == g.dtype and g.stride(2) == 1 and u.stride(2) == 1
    assert B == 1 or (g.stride(0) == S * g.stride(1) and u.stride(0) == S * u.stride(1))
    y = torch.empty((B, S, I), device=g.device, dtype=g.dtype)
    with torch.cuda.device(g.device):
        check(lib().bd_srv_swiglu(ptr(g), ptr(u), ptr(y), B * S, I, g.stride(1), u.stride(1), I, 0, DTYPE_CODE[g.dtype], stream_ptr()),
              "srv_swiglu")
    return y


def swiglu_interleaved8(gu):
    """gu [B, S, 2*I]: the output of a gate|up projection whose rows are interleaved in blocks of 8 ([g0..7 | u0..7 | g8..15 | ...],
    FusedDeltaLinear(interleave8=True)) -> round(silu(gate)) * up, [B, S, I]"""
    require_gpu(gu)
    B, S, I2 = gu.shape
    I = I2 // 2
    assert I2 % 16 == 0 and gu.stride(2) == 1 and (B == 1 or gu.stride(0) == S * gu.stride(1))
    y = torch.empty((B, S, I), device=gu.device, dtype=gu.dtype)
    with torch.cuda.device(gu.device):
        check(lib().bd_srv_swiglu(ptr(gu), ptr(gu), ptr(y), B * S, I, gu.stride(1), gu.stride(1), I, 1, DTYPE_CODE[gu.dtype],
                                  stream_ptr()), "srv_swiglu")
    return y


def table_stride(cos, sin, tenants):
    """The tenant stride (elements) of a pair of rotary tables as the *_tab entries take it: 0 for one shared [Lmax, 128] pair, Lmax * 128 for a
    contiguous per-tenant [T, Lmax, 128] pair (serving_loop.rope_tables per tenant, stacked).  A per-tenant pair whose leading dimension is
    not the launch's tenant count is a ValueError: tenant t would rotate with another tenant's rows, or read past the end.  Host only."""
    if cos.dim() not in (2, 3) or cos.shape != sin.shape:
        raise ValueError("rotary tables: cos %s and sin %s where [Lmax, 128] or [T, Lmax, 128] pairs are taken" % (tuple(cos.shape), tuple(sin.shape)))
    if cos.dim() == 2:
        return 0
    if cos.shape[0] != tenants:
        raise ValueError("rotary tables for %d tenants in a launch of %d" % (cos.shape[0], tenants))
    return cos.shape[1] * cos.shape[2]


def decode_attention(qkv, cos, sin, kcache, vcache, valid, pos, heads, kv_heads):
    """One new token per tenant.  qkv [T, 1, (heads + 2 kv_heads) * 128]; cos / sin [Lmax, 128], or contiguous [T, Lmax, 128]: tenant t's own
    tables (bd_srv_decode_attention_tab); caches [T, kv_heads, Lc, 128];
    valid [T, Lc] bool; pos: int64 device tensor with one element.  Returns [T, 1, heads * 128]; the caches and valid[:, pos] are
    updated in place."""
    T = qkv.shape[0]
    s_tab = table_stride(cos, sin, T)
    require_gpu(qkv, cos, sin, kcache, vcache, valid, pos)
    hd = kcache.shape[3]
    assert qkv.shape[1] == 1 and qkv.shape[2] == (heads + 2 * kv_heads) * hd and qkv.stride(2) == 1
    assert kcache.is_contiguous() and vcache.is_contiguous() and valid.is_contiguous() and valid.dtype == torch.bool
    assert cos.is_contiguous() and sin.is_contiguous() and cos.dtype == qkv.dtype and pos.dtype == torch.int64
    out = torch.empty((T, 1, heads * hd), device=qkv.device, dtype=qkv.dtype)
    L = lib()
    need = L.bd_srv_decode_attention_workspace_bytes(T, heads, kv_heads, hd, kcache.shape[2])
    # persistent per-stream scratch, zero-filled once: the kernel's arrival counters must be zero at launch and it restores them
    ws, need = workspace(need, qkv.device, zeroed=True) if need > 0 else (None, 0)
    with torch.cuda.device(qkv.device):
        if cos.dim() == 3:
            check(L.bd_srv_decode_attention_tab(ptr(qkv), ptr(cos), ptr(sin), s_tab, ptr(kcache), ptr(vcache), ptr(valid), ptr(pos), ptr(out),
                                                T, heads, kv_heads, hd, kcache.shape[2], qkv.stride(0), out.stride(0),
                                                DTYPE_CODE[qkv.dtype], ptr(ws), need, stream_ptr()), "srv_decode_attention_tab")
            return out
        check(L.bd_srv_decode_attention(ptr(qkv), ptr(cos), ptr(sin), ptr(kcache), ptr(vcache), ptr(valid), ptr(pos), ptr(out),
                                        T, heads, kv_heads, hd, kcache.shape[2], qkv.stride(0), out.stride(0),
                                        DTYPE_CODE[qkv.dtype], ptr(ws), need, stream_ptr()), "srv_decode_attention")
    return out


def decode_attention_ragged(qkv, cos, sin, kcache, vcache, valid, pos, active, heads, kv_heads):
    """decode_attention with one position per tenant: pos int64 [T], active bool [T] on the device.  Tenant t attends over its valid keys
    0 .. pos[t] and appends at pos[t]; a tenant that is inactive or whose position lies outside the cache gets a zero output row and its cache
    and valid rows stay as they are.  cos / sin [Lmax, 128] or per tenant [T, Lmax, 128], as in decode_attention."""
    T = qkv.shape[0]
    s_tab = table_stride(cos, sin, T)
    require_gpu(qkv, cos, sin, kcache, vcache, valid, pos, active)
    hd = kcache.shape[3]
    assert qkv.shape[1] == 1 and qkv.shape[2] == (heads + 2 * kv_heads) * hd and qkv.stride(2) == 1
    assert kcache.is_contiguous() and vcache.is_contiguous() and valid.is_contiguous() and valid.dtype == torch.bool
    assert cos.is_contiguous() and sin.is_contiguous() and cos.dtype == qkv.dtype and pos.dtype == torch.int64
    assert pos.numel() == T and pos.is_contiguous() and active.dtype == torch.bool and active.numel() == T and active.is_contiguous()
    out = torch.empty((T, 1, heads * hd), device=qkv.device, dtype=qkv.dtype)
    L = lib()
    need = L.bd_srv_decode_attention_workspace_bytes(T, heads, kv_heads, hd, kcache.shape[2])
    ws, need = workspace(need, qkv.device, zeroed=True) if need > 0 else (None, 0)          # (the scalar form's persistent scratch, same contract)
    with torch.cuda.device(qkv.device):
        if cos.dim() == 3:
            check(L.bd_srv_decode_attention_ragged_tab(ptr(qkv), ptr(cos), ptr(sin), s_tab, ptr(kcache), ptr(vcache), ptr(valid), ptr(pos),
                                                       ptr(active), ptr(out), T, heads, kv_heads, hd, kcache.shape[2], qkv.stride(0), out.stride(0),
                                                       DTYPE_CODE[qkv.dtype], ptr(ws), need, stream_ptr()), "srv_decode_attention_ragged_tab")
            return out
        check(L.bd_srv_decode_attention_ragged(ptr(qkv), ptr(cos), ptr(sin), ptr(kcache), ptr(vcache), ptr(valid), ptr(pos), ptr(active), ptr(out),
                                               T, heads, kv_heads, hd, kcache.shape[2], qkv.stride(0), out.stride(0),
                                               DTYPE_CODE[qkv.dtype], ptr(ws), need, stream_ptr()), "srv_decode_attention_ragged")
    return out


def prefill_attention_supported(q, k, v):
    """the shapes bd_srv_prefill_attention takes: [B, S, heads, 128] views (any batch / sequence strides that are multiples of 8 elements,
    heads contiguous), S a multiple of 64"""
    if q.dim() != 4 or q.shape[3] != 128 or q.dtype not in DTYPE_CODE or q.shape[1] % 64 or q.shape[2] % k.shape[2]:
        return False
    for t in (q, k, v):
        if t.stride(3) != 1 or t.stride(2) != 128 or t.stride(1) % 8 or t.stride(0) % 8 or t.data_ptr() % 16:
            return False
    return k.shape == v.shape and k.shape[:2] == q.shape[:2] and k.dtype == q.dtype == v.dtype


def prefill_attention(q, k, v, kv_start=None, causal=True, scale=None):
    """Flash-style attention of a whole prompt.  q [B, S, heads, 128], k / v [B, S, kv_heads, 128] -- views into a fused q|k|v projection
    output are fine (after RoPE); kv_start: optional int32 [B] device tensor, first valid key of each sequence (left padding).
    Returns [B, S, heads * 128] (what the o projection consumes)."""
    require_gpu(q, k, v)
    assert prefill_attention_supported(q, k, v), "prefill_attention: unsupported geometry"
    B, S, H, hd = q.shape
    out = torch.empty((B, S, H * hd), device=q.device, dtype=q.dtype)
    if kv_start is not None:
        assert kv_start.dtype == torch.int32 and kv_start.is_cuda and kv_start.numel() == B and kv_start.is_contiguous()
    with torch.cuda.device(q.device):
        check(lib().bd_srv_prefill_attention(ptr(q), ptr(k), ptr(v), ptr(out), B, S, H, k.shape[2], hd, q.stride(0), q.stride(1),
                                             k.stride(0), k.stride(1), v.stride(0), v.stride(1), out.stride(0), out.stride(1),
                                             ptr(kv_start) if kv_start is not None else None,
                                             float(scale if scale is not None else hd ** -0.5), int(bool(causal)),
                                             DTYPE_CODE[q.dtype], stream_ptr()), "srv_prefill_attention")
    return out


def prefill_attention_cached_supported(q, kcache, vcache, q0=0):
    """the shapes bd_srv_prefill_attention_cached takes: q a [B, Sq, heads, 128] view (batch / sequence strides multiples of 8 elements, heads
    contiguous, Sq >= 1), the caches [B, kv_heads, Lc, 128] (any batch / head / key strides that are multiples of 8), 0 <= q0 and q0 + Sq <= Lc"""
    if q.dim() != 4 or kcache.dim() != 4 or q.shape[3] != 128 or q.dtype not in DTYPE_CODE or q.shape[1] < 1 or q.shape[2] % kcache.shape[1]:
        return False
    if q.stride(3) != 1 or q.stride(2) != 128 or q.stride(1) % 8 or q.stride(0) % 8 or q.data_ptr() % 16:
        return False
    for t in (kcache, vcache):
        if t.stride(3) != 1 or t.stride(2) % 8 or t.stride(1) % 8 or t.stride(0) % 8 or t.data_ptr() % 16:
            return False
    return (kcache.shape == vcache.shape and kcache.shape[0] == q.shape[0] and kcache.shape[3] == 128 and kcache.dtype == q.dtype == vcache.dtype
            and 0 <= q0 and q0 + q.shape[1] <= kcache.shape[2])


def prefill_attention_cached(q, kcache, vcache, q0, kv_start=None, scale=None):
    """Causal flash-style attention of a chunk of queries at positions q0 .. q0 + Sq - 1 over the keys in the KV caches (the chunk's own rows
    already appended: rope_kv_append_(..., pos0=q0)).  q [B, Sq, heads, 128] -- the q slice of a fused q|k|v projection output is fine;
    kcache / vcache [B, kv_heads, Lc, 128]; kv_start: optional int32 [B] device tensor, first valid key of each sequence (left padding).
    Cache rows at or past q0 + Sq are not trusted.  Returns [B, Sq, heads * 128] (what the o projection consumes)."""
    require_gpu(q, kcache, vcache)
    q0 = int(q0)
    assert prefill_attention_cached_supported(q, kcache, vcache, q0), "prefill_attention_cached: unsupported geometry"
    B, Sq, H, hd = q.shape
    out = torch.empty((B, Sq, H * hd), device=q.device, dtype=q.dtype)
    if kv_start is not None:
        assert kv_start.dtype == torch.int32 and kv_start.is_cuda and kv_start.numel() == B and kv_start.is_contiguous()
    with torch.cuda.device(q.device):
        check(lib().bd_srv_prefill_attention_cached(ptr(q), ptr(kcache), ptr(vcache), ptr(out), B, Sq, H, kcache.shape[1], hd, q0, kcache.shape[2],
                                                    q.stride(0), q.stride(1), kcache.stride(0), kcache.stride(1), kcache.stride(2),
                                                    vcache.stride(0), vcache.stride(1), vcache.stride(2), out.stride(0), out.stride(1),
                                                    ptr(kv_start) if kv_start is not None else None,
                                                    float(scale if scale is not None else hd ** -0.5), DTYPE_CODE[q.dtype], stream_ptr()),
              "srv_prefill_attention_cached")
    return out


def cache_warm(a, b=None, blocks=0):
    """Read tensor a (and b) and discard the values on the CURRENT stream: the weight-prefetch node of a hipGraph side branch
    (serving_loop.TenantDecoder.prefetch_o).  Contiguous device tensors; whole 16-byte chunks are touched."""
    require_gpu(a)
    assert a.is_contiguous() and (b is None or (b.is_cuda and b.is_contiguous()))
    with torch.cuda.device(a.device):
        check(lib().bd_srv_cache_warm(ptr(a), a.numel() * a.element_size(), ptr(b) if b is not None else None,
                                      b.numel() * b.element_size() if b is not None else 0, int(blocks), stream_ptr()), "srv_cache_warm")


def decode_attention_supported(heads, kv_heads, head_dim):
    return head_dim == 128 and heads % kv_heads == 0 and heads // kv_heads in (1, 4, 8)


def rope_(x, cos, sin, heads, seq, pos0=0):
    """In-place rotary embedding of x [B, S, heads * 128] (a q / k projection output, before the head transpose); row r sits at position
    pos0 + r % seq.  cos / sin [Lmax, 128] in x.dtype with the rotate-half sign folded into sin, or contiguous [B, Lmax, 128]: batch row b is
    tenant b and rotates with its own tables (bd_srv_rope_tab; seq is then x.shape[1]).  Returns x."""
    s_tab = table_stride(cos, sin, x.shape[0])
    require_gpu(x, cos, sin)
    assert x.dim() == 3 and x.shape[2] == heads * 128 and x.stride(2) == 1
    assert x.shape[0] == 1 or x.stride(0) == x.shape[1] * x.stride(1)
    assert cos.is_contiguous() and sin.is_contiguous() and cos.dtype == x.dtype and cos.shape[-2] >= pos0 + seq
    with torch.cuda.device(x.device):
        if cos.dim() == 3:
            assert seq == x.shape[1], "per-tenant tables: the tenant of row r is r // seq, so seq is the rows per tenant"
            check(lib().bd_srv_rope_tab(ptr(x), ptr(cos), ptr(sin), s_tab, x.shape[0] * x.shape[1], heads, 128, x.stride(1), seq, pos0,
                                        DTYPE_CODE[x.dtype], stream_ptr()), "srv_rope_tab")
            return x
        check(lib().bd_srv_rope(ptr(x), ptr(cos), ptr(sin), x.shape[0] * x.shape[1], heads, 128, x.stride(1), seq, pos0,
                                DTYPE_CODE[x.dtype], stream_ptr()), "srv_rope")
    return x


def step_begin(embed, tok, valid, pos):
    """First launch of a greedy decode step: x[t] = embed[t, tok[t]] -> [T, 1, H], and valid[t, pos] = True (what `valid.index_fill_(1, pos, True)`
    and the per-tenant embedding gather do).  embed [T, V, H] (or [V, H]: one shared table), tok [T, 1] long, valid [T, Lc] bool, pos [1] long."""
    require_gpu(embed, tok, valid, pos)
    shared = embed.dim() == 2
    V, H = embed.shape[-2], embed.shape[-1]
    T = tok.shape[0]
    assert tok.dtype == torch.long and tok.is_contiguous() and tok.numel() == T and pos.dtype == torch.long and pos.numel() == 1
    assert valid.dtype == torch.bool and valid.is_contiguous() and valid.shape[0] == T and (shared or embed.shape[0] == T)
    assert embed.stride(-1) == 1 and H % 8 == 0
    x = torch.empty((T, 1, H), device=embed.device, dtype=embed.dtype)
    with torch.cuda.device(embed.device):
        check(lib().bd_srv_step_begin(ptr(embed), 0 if shared else embed.stride(0), embed.stride(-2), ptr(tok), ptr(x), H, ptr(valid), valid.shape[1],
                                      ptr(pos), T, V, H, stream_ptr()), "srv_step_begin")
    return x


def step_end(logits, tok, out, step, pos, stop_ids, stopped, ticket):
    """Last launch of a greedy decode step: nxt = argmax(logits, -1) (torch's order); tok[:, 0] = nxt; out[:, step] = nxt; stopped |= (nxt[:, None] ==
    stop_ids).any(1); pos += 1; step += 1 -- the five stock ops of the loop in one launch.  logits [T, V] 16-bit, ticket: a zeroed int32 word."""
    require_gpu(logits, tok, out, step, pos, stop_ids, stopped, ticket)
    T, V = logits.shape
    assert logits.stride(1) == 1 and V % 8 == 0 and tok.dtype == torch.long and tok.is_contiguous() and tok.numel() == T
    assert out.dtype == torch.long and out.shape[0] == T and out.stride(1) == 1 and stop_ids.dtype == torch.long and stop_ids.is_contiguous()
    assert stop_ids.shape[0] == T and stopped.dtype == torch.bool and stopped.is_contiguous() and stopped.numel() == T
    assert step.dtype == torch.long and pos.dtype == torch.long and step.numel() == 1 and pos.numel() == 1
    assert ticket.dtype == torch.int32 and ticket.numel() == 1
    with torch.cuda.device(logits.device):
        check(lib().bd_srv_step_end(ptr(logits), logits.stride(0), V, ptr(tok), ptr(out), out.stride(0), out.shape[1], ptr(stop_ids), stop_ids.shape[1],
                                    ptr(stopped), ptr(pos), ptr(step), ptr(ticket), T, DTYPE_CODE[logits.dtype], stream_ptr()), "srv_step_end")


def step_begin_ragged(embed, tok, valid, pos, active):
    """step_begin with per-tenant state: x[t] = embed[t, tok[t]] and valid[t, pos[t]] = True for an active tenant whose position lies in the cache;
    a zero row and no mark otherwise.  pos [T] long, active [T] bool."""
    require_gpu(embed, tok, valid, pos, active)
    shared = embed.dim() == 2
    V, H = embed.shape[-2], embed.shape[-1]
    T = tok.shape[0]
    assert tok.dtype == torch.long and tok.is_contiguous() and tok.numel() == T and pos.dtype == torch.long and pos.numel() == T and pos.is_contiguous()
    assert valid.dtype == torch.bool and valid.is_contiguous() and valid.shape[0] == T and (shared or embed.shape[0] == T)
    assert embed.stride(-1) == 1 and H % 8 == 0 and active.dtype == torch.bool and active.numel() == T and active.is_contiguous()
    x = torch.empty((T, 1, H), device=embed.device, dtype=embed.dtype)
    with torch.cuda.device(embed.device):
        check(lib().bd_srv_step_begin_ragged(ptr(embed), 0 if shared else embed.stride(0), embed.stride(-2), ptr(tok), ptr(x), H, ptr(valid),
                                             valid.shape[1], ptr(pos), ptr(active), T, V, H, stream_ptr()), "srv_step_begin_ragged")
    return x


def step_end_ragged(logits, tok, out, n, pos, limit, stop_ids, active, done, cache_len):
    """Last launch of a ragged step, per ACTIVE tenant: nxt = argmax(logits[t]); tok[t] = nxt; out[t, n[t]] = nxt; n[t] += 1; pos[t] += 1; and the
    tenant retires (active[t] = False, done[t] = reason) when nxt is one of its stop ids (1), n[t] reached limit[t] (2) or pos[t] reached
    cache_len (4).  logits [T, V] 16-bit; n / pos / limit [T] long; active [T] bool; done [T] uint8."""
    require_gpu(logits, tok, out, n, pos, limit, stop_ids, active, done)
    T, V = logits.shape
    assert logits.stride(1) == 1 and V % 8 == 0 and tok.dtype == torch.long and tok.is_contiguous() and tok.numel() == T
    assert out.dtype == torch.long and out.shape[0] == T and out.stride(1) == 1 and stop_ids.dtype == torch.long and stop_ids.is_contiguous()
    assert stop_ids.shape[0] == T and active.dtype == torch.bool and active.is_contiguous() and active.numel() == T
    assert done.dtype == torch.uint8 and done.is_contiguous() and done.numel() == T
    for v in (n, pos, limit):
        assert v.dtype == torch.long and v.numel() == T and v.is_contiguous()
    with torch.cuda.device(logits.device):
        check(lib().bd_srv_step_end_ragged(ptr(logits), logits.stride(0), V, ptr(tok), ptr(out), out.stride(0), out.shape[1], ptr(stop_ids),
                                           stop_ids.shape[1], ptr(pos), ptr(n), ptr(limit), ptr(active), ptr(done), int(cache_len), T,
                                           DTYPE_CODE[logits.dtype], stream_ptr()), "srv_step_end_ragged")


def _sampling_arrays(R, temperature, top_k, top_p, seed, dbg):
    assert temperature.dtype == torch.float32 and top_p.dtype == torch.float32 and top_k.dtype == torch.int32 and seed.dtype == torch.long
    for v in (temperature, top_k, top_p, seed):
        assert v.numel() == R and v.is_contiguous()
    assert dbg is None or (dbg.dtype == torch.int32 and dbg.shape == (R, 4) and dbg.is_contiguous())


def sample_rows(logits, temperature, top_k, top_p, seed, draw, dbg=None):
    """One token per row of logits [R, V] (16-bit), each row with its own temperature / top_p (float32 [R]), top_k (int32 [R]), seed (int64 [R]:
    the seed's 64 bits) and draw index `draw` (int64 [R]); include/bitdelta_hip.h (bd_srv_sample_rows) is the definition.  Returns tok, int64
    [R].  dbg: an int32 [R, 4] tensor that receives kept count / smallest kept logit's bits / the token's Philox word / flags."""
    require_gpu(logits, temperature, top_k, top_p, seed, draw, dbg)
    R, V = logits.shape
    assert logits.stride(1) == 1 and V % 8 == 0 and draw.dtype == torch.long and draw.numel() == R and draw.is_contiguous()
    _sampling_arrays(R, temperature, top_k, top_p, seed, dbg)
    tok = torch.empty(R, dtype=torch.long, device=logits.device)
    with torch.cuda.device(logits.device):
        check(lib().bd_srv_sample_rows(ptr(logits), logits.stride(0), V, ptr(temperature), ptr(top_k), ptr(top_p), ptr(seed), ptr(draw), ptr(tok),
                                       ptr(dbg), R, DTYPE_CODE[logits.dtype], stream_ptr()), "srv_sample_rows")
    return tok


def token_nll(logits, labels, lse=False):
    """nll[r] = -log softmax(logits[r])[labels[r]] for logits [R, V] (16-bit) and labels int64 [R]; include/bitdelta_hip.h (bd_srv_token_nll) is
    the definition.  A label outside [0, V) is ignored: exactly 0.  Returns nll, float32 [R] -- or (nll, lse) with lse=True, lse the rows'
    log-sum-exp.  Rows whose layout the entry point does not take (last dimension strided, a row stride that is no multiple of 8 -- a [R, 32001]
    tensor --, a misaligned start) are copied into rows of V rounded up to 8 elements; the padding is never read into a result."""
    require_gpu(logits, labels)
    assert logits.dim() == 2 and labels.dtype == torch.long and labels.numel() == logits.shape[0]
    R, V = logits.shape
    V8 = (V + 7) // 8 * 8                                   # the kernel reads whole 16-byte vectors: a row occupies V8 elements
    sl = logits.stride(0) if R > 1 else V8
    last = logits.storage_offset() + (R - 1) * sl + V8      # ... and the last row's must lie inside the tensor's storage
    if (logits.stride(1) != 1 or sl % 8 or sl < V or logits.data_ptr() % 16
            or last * logits.element_size() > logits.untyped_storage().nbytes()):
        padded = torch.empty((R, V8), device=logits.device, dtype=logits.dtype)
        padded[:, :V].copy_(logits)
        logits, sl = padded, V8
    labels = labels.contiguous()
    nll = torch.empty(R, dtype=torch.float32, device=logits.device)
    row_lse = torch.empty(R, dtype=torch.float32, device=logits.device) if lse else None
    with torch.cuda.device(logits.device):
        check(lib().bd_srv_token_nll(ptr(logits), sl, V, ptr(labels), ptr(nll), ptr(row_lse), R, DTYPE_CODE[logits.dtype], stream_ptr()),
              "srv_token_nll")
    return (nll, row_lse) if lse else nll


LOGPROBS_MAX = 20          # include/bitdelta_hip.h (bd_srv_token_logprobs): top_n is 0 .. 20


def token_logprobs(logits, tokens, top_n, out=None):
    """(lp, top_id, top_lp) for logits [R, V] (16-bit, V % 8 == 0), tokens int64 [R] and 0 <= top_n <= 20: lp[r] = log softmax(logits[r])[tokens[r]]
    (float32 [R]), top_id int32 / top_lp float32 [R, top_n] the top_n most probable tokens of each row and their log-probabilities, in descending
    order, ties by ascending index; include/bitdelta_hip.h (bd_srv_token_logprobs) is the definition.  The distribution is the row's softmax at
    temperature 1, before any filter.  Rows whose layout the entry point does not take (last dimension strided, a row stride that is no multiple
    of 8, a misaligned start) are copied first; the elements V .. stride - 1 of a row are never read into a result.  out: (lp, top_id, top_lp)
    to write into instead of new tensors (contiguous, of those shapes and dtypes)."""
    require_gpu(logits, tokens)
    assert logits.dim() == 2 and tokens.dtype == torch.long and tokens.numel() == logits.shape[0]
    R, V = logits.shape
    top_n = int(top_n)
    assert V % 8 == 0 and 0 <= top_n <= min(LOGPROBS_MAX, V)
    sl = logits.stride(0) if R > 1 else V
    if logits.stride(1) != 1 or sl % 8 or sl < V or logits.data_ptr() % 16:
        logits, sl = logits.contiguous(), V
    tokens = tokens.contiguous()
    if out is None:
        out = (torch.empty(R, dtype=torch.float32, device=logits.device), torch.empty((R, top_n), dtype=torch.int32, device=logits.device),
               torch.empty((R, top_n), dtype=torch.float32, device=logits.device))
    lp, top_id, top_lp = out
    require_gpu(lp, top_id, top_lp)
    assert lp.dtype == torch.float32 and lp.shape == (R,) and lp.is_contiguous()
    assert top_id.dtype == torch.int32 and top_id.shape == (R, top_n) and top_id.is_contiguous()
    assert top_lp.dtype == torch.float32 and top_lp.shape == (R, top_n) and top_lp.is_contiguous()
    with torch.cuda.device(logits.device):
        check(lib().bd_srv_token_logprobs(ptr(logits), sl, V, ptr(tokens), ptr(lp), ptr(top_id) if top_n else None, ptr(top_lp) if top_n else None,
                                          top_n, R, DTYPE_CODE[logits.dtype], stream_ptr()), "srv_token_logprobs")
    return lp, top_id, top_lp


def step_logprobs(logits, tok, n, lp_n, lp, top_id, top_lp):
    """Behind step_end_ragged / step_end_sample in the same step, per tenant whose count n[t] moved past lp_n[t]: entry [t, n[t] - 1] of lp
    [T, cap] float32, top_id [T, cap, k] int32 and top_lp [T, cap, k] float32 from row t of logits [T, V] and tok[t] (token_logprobs' rule), and
    lp_n[t] = n[t].  A tenant that emitted nothing in the step is not touched.  n / lp_n [T] long; k = top_id.shape[2], 0 .. 20."""
    require_gpu(logits, tok, n, lp_n, lp, top_id, top_lp)
    T, V = logits.shape
    cap, k = top_id.shape[1], top_id.shape[2]
    assert logits.stride(1) == 1 and V % 8 == 0 and tok.dtype == torch.long and tok.is_contiguous() and tok.numel() == T
    for v in (n, lp_n):
        assert v.dtype == torch.long and v.numel() == T and v.is_contiguous()
    assert lp.dtype == torch.float32 and lp.shape == (T, cap) and lp.is_contiguous()
    assert top_id.dtype == torch.int32 and top_id.shape == (T, cap, k) and top_id.is_contiguous()
    assert top_lp.dtype == torch.float32 and top_lp.shape == (T, cap, k) and top_lp.is_contiguous() and 0 <= k <= min(LOGPROBS_MAX, V)
    with torch.cuda.device(logits.device):
        check(lib().bd_srv_step_logprobs(ptr(logits), logits.stride(0), V, ptr(tok), ptr(n), ptr(lp_n), ptr(lp), ptr(top_id) if k else None,
                                         ptr(top_lp) if k else None, cap, k, T, DTYPE_CODE[logits.dtype], stream_ptr()), "srv_step_logprobs")


LOGIT_BIAS_MAX = 64        # include/bitdelta_hip.h (BD_LOGIT_BIAS_MAX): pairs per row of a bias list


def _penalty_args(logits, out, hist, pen, bias_id, bias_val):
    """the checks penalize_rows and step_penalize share; returns (out, nb, bias_id pointer, bias_val pointer)"""
    R, V = logits.shape
    assert logits.stride(1) == 1 and V % 8 == 0 and logits.dtype in (torch.float16, torch.bfloat16)
    if out is None:
        out = torch.empty((R, V), dtype=logits.dtype, device=logits.device)
    require_gpu(out, hist, pen)
    assert out.shape == (R, V) and out.dtype == logits.dtype and out.stride(1) == 1
    assert hist.shape == (R, V) and hist.dtype == torch.int16 and hist.stride(1) == 1
    assert pen.shape == (R, 4) and pen.dtype == torch.float32 and pen.is_contiguous()
    if bias_id is None or bias_id.shape[1] == 0:
        return out, 0, None, None
    require_gpu(bias_id, bias_val)
    nb = bias_id.shape[1]
    assert bias_id.shape == bias_val.shape == (R, nb) and nb <= LOGIT_BIAS_MAX and bias_id.is_contiguous() and bias_val.is_contiguous()
    assert bias_id.dtype == torch.int32 and bias_val.dtype == torch.float32
    return out, nb, ptr(bias_id), ptr(bias_val)


def penalize_rows(logits, hist, pen, bias_id=None, bias_val=None, out=None):
    """The penalised copy of logits [R, V] (16-bit, V % 8 == 0): repetition / presence / frequency penalties from the rows' token history hist
    int16 [R, V] (bit 15: in the context; bits 0 .. 14: times generated this turn) and pen float32 [R, 4] = (r, float(1 / r), presence,
    frequency), then the bias list bias_id int32 / bias_val float32 [R, nb <= 64] (id -1: an empty slot; None: no list), rounded to the logits'
    dtype; include/bitdelta_hip.h (bd_srv_penalize_rows) is the definition.  Every row is live and hist is only read.  Rows may be strided
    (stride % 8 == 0, 16-byte aligned; logits of another layout are copied first, as in token_logprobs); out: a tensor of the logits' shape
    and dtype to write into instead of a new one."""
    require_gpu(logits)
    assert logits.dim() == 2
    R, V = logits.shape
    sl = logits.stride(0) if R > 1 else V
    if logits.stride(1) != 1 or sl % 8 or sl < V or logits.data_ptr() % 16:             # (token_logprobs' rule: such rows are copied first)
        logits, sl = logits.contiguous(), V
    out, nb, bi, bv = _penalty_args(logits, out, hist, pen, bias_id, bias_val)
    with torch.cuda.device(logits.device):
        check(lib().bd_srv_penalize_rows(ptr(logits), sl, V, ptr(out), out.stride(0) if R > 1 else V, ptr(hist), hist.stride(0) if R > 1 else V,
                                         ptr(pen), bi, bv, nb, R, DTYPE_CODE[logits.dtype], stream_ptr()), "srv_penalize_rows")
    return out


def step_penalize(logits, out, hist, tok, active, pen, bias_id=None, bias_val=None):
    """penalize_rows inside a ragged decode step, logits [T, V] -> out [T, V], and it counts: for an active tenant t the element tok[t] (the token
    generated last and fed in this step) of hist [T, V] gains one (saturating at 32767) before the penalties read it, and that one element is
    stored.  An inactive tenant's rows of out and hist are not touched.  tok [T] or [T, 1] long, active [T] bool / uint8."""
    require_gpu(logits, tok, active)
    out, nb, bi, bv = _penalty_args(logits, out, hist, pen, bias_id, bias_val)
    T, V = logits.shape
    assert tok.dtype == torch.long and tok.is_contiguous() and tok.numel() == T
    assert active.dtype in (torch.bool, torch.uint8) and active.is_contiguous() and active.numel() == T
    with torch.cuda.device(logits.device):
        check(lib().bd_srv_step_penalize(ptr(logits), logits.stride(0), V, ptr(out), out.stride(0), ptr(hist), hist.stride(0), ptr(tok), ptr(active),
                                         ptr(pen), bi, bv, nb, T, DTYPE_CODE[logits.dtype], stream_ptr()), "srv_step_penalize")
    return out


CONSTRAINT_STATES_MAX = 1 << 16      # include/bitdelta_hip.h (BD_CONSTRAINT_STATES_MAX / _EDGES_MAX / _STOP_MAX)
CONSTRAINT_EDGES_MAX = 1 << 20
CONSTRAINT_STOP_MAX = 64


def _automaton_args(R, state, off, edge_tok, accepting, edge_next=None):
    """the checks the three constraint launches share on the per-row automaton arrays; returns (S, E, edge_tok pointer, edge_next pointer)"""
    require_gpu(state, off, accepting)
    assert state.dtype == torch.int32 and state.is_contiguous() and state.numel() == R
    assert off.dim() == 2 and off.shape[0] == R and off.dtype == torch.int32 and off.is_contiguous()
    S = off.shape[1] - 1
    assert 1 <= S <= CONSTRAINT_STATES_MAX
    assert accepting.shape == (R, S) and accepting.dtype in (torch.bool, torch.uint8) and accepting.is_contiguous()
    assert edge_tok.dim() == 2 and edge_tok.shape[0] == R and edge_tok.dtype == torch.int32 and edge_tok.is_contiguous()
    E = edge_tok.shape[1]
    assert E <= CONSTRAINT_EDGES_MAX
    if edge_next is not None:
        assert edge_next.shape == (R, E) and edge_next.dtype == torch.int32 and edge_next.is_contiguous()
    if E == 0:
        return S, 0, None, None
    require_gpu(edge_tok, *([] if edge_next is None else [edge_next]))
    return S, E, ptr(edge_tok), None if edge_next is None else ptr(edge_next)


def _constrain_args(logits, out, state, off, edge_tok, accepting, stop_ids):
    """the checks constrain_rows and step_constrain share; returns (out, S, E, edge_tok pointer, ns, stop_ids pointer)"""
    R, V = logits.shape
    assert logits.stride(1) == 1 and V % 8 == 0 and logits.dtype in (torch.float16, torch.bfloat16)
    if out is None:
        out = torch.empty((R, V), dtype=logits.dtype, device=logits.device)
    require_gpu(out)
    assert out.shape == (R, V) and out.dtype == logits.dtype and out.stride(1) == 1
    S, E, et, _ = _automaton_args(R, state, off, edge_tok, accepting)
    if stop_ids is None or stop_ids.shape[1] == 0:
        return out, S, E, et, 0, None
    require_gpu(stop_ids)
    ns = stop_ids.shape[1]
    assert stop_ids.shape == (R, ns) and ns <= CONSTRAINT_STOP_MAX and stop_ids.dtype == torch.long and stop_ids.is_contiguous()
    return out, S, E, et, ns, ptr(stop_ids)


def constrain_rows(logits, state, off, edge_tok, accepting, stop_ids=None, out=None):
    """The constrained copy of logits [R, V] (16-bit, V % 8 == 0): every element whose token the row's automaton state does not allow is -inf,
    every other element keeps its bits; include/bitdelta_hip.h (bd_srv_constrain_rows) is the definition.  state int32 [R] (negative: no
    constraint, the row is copied); per row, in CSR form, off int32 [R, S + 1], edge_tok int32 [R, E] (sorted within a state), accepting
    bytes [R, S]; stop_ids long [R, ns <= 64] (-1: an empty slot; None: no list), allowed in an accepting state.  Rows may be strided
    (stride % 8 == 0, 16-byte aligned; logits of another layout are copied first, as in penalize_rows); out: a tensor of the logits' shape and
    dtype to write into instead of a new one."""
    require_gpu(logits)
    assert logits.dim() == 2
    R, V = logits.shape
    sl = logits.stride(0) if R > 1 else V
    if logits.stride(1) != 1 or sl % 8 or sl < V or logits.data_ptr() % 16:             # (token_logprobs' rule: such rows are copied first)
        logits, sl = logits.contiguous(), V
    out, S, E, et, ns, sp = _constrain_args(logits, out, state, off, edge_tok, accepting, stop_ids)
    with torch.cuda.device(logits.device):
        check(lib().bd_srv_constrain_rows(ptr(logits), sl, V, ptr(out), out.stride(0) if R > 1 else V, ptr(state), ptr(off), et, ptr(accepting),
                                          S, E, sp, ns, R, DTYPE_CODE[logits.dtype], stream_ptr()), "srv_constrain_rows")
    return out


def step_constrain(logits, out, state, off, edge_tok, accepting, stop_ids, active):
    """constrain_rows inside a ragged decode step, logits [T, V] -> out [T, V], between the lm_head (or step_penalize) and the step end, which
    then reads `out`.  An inactive tenant's row of out is not touched.  The launch only reads state; step_constrain_advance moves it.  active
    [T] bool / uint8."""
    require_gpu(logits, active)
    out, S, E, et, ns, sp = _constrain_args(logits, out, state, off, edge_tok, accepting, stop_ids)
    T, V = logits.shape
    assert active.dtype in (torch.bool, torch.uint8) and active.is_contiguous() and active.numel() == T
    with torch.cuda.device(logits.device):
        check(lib().bd_srv_step_constrain(ptr(logits), logits.stride(0), V, ptr(out), out.stride(0), ptr(state), ptr(off), et, ptr(accepting), S, E,
                                          sp, ns, ptr(active), T, DTYPE_CODE[logits.dtype], stream_ptr()), "srv_step_constrain")
    return out


def step_constrain_advance(tok, n, c_n, state, off, edge_tok, edge_next, accepting, active, done):
    """The automaton's transition behind the step end: for every tenant whose token count n[t] moved past the launch's own counter c_n[t]
    (which then follows it), state[t] follows the edge on tok[t] when its state has one; a tenant that reaches a final state (accepting, no
    edges) while still active is retired: active[t] = 0, done[t] |= 8.  include/bitdelta_hip.h (bd_srv_step_constrain_advance) is the
    definition.  tok [T] or [T, 1], n, c_n long; state int32 [T]; edge_next int32 [T, E]; active, done [T] bool / uint8."""
    require_gpu(tok, n, c_n, active, done)
    T = state.numel()
    S, E, et, en = _automaton_args(T, state, off, edge_tok, accepting, edge_next)
    for x in (tok, n, c_n):
        assert x.dtype == torch.long and x.is_contiguous() and x.numel() == T
    for x in (active, done):
        assert x.dtype in (torch.bool, torch.uint8) and x.is_contiguous() and x.numel() == T
    with torch.cuda.device(state.device):
        check(lib().bd_srv_step_constrain_advance(ptr(tok), ptr(n), ptr(c_n), ptr(state), ptr(off), et, en, ptr(accepting), S, E, ptr(active),
                                                  ptr(done), T, stream_ptr()), "srv_step_constrain_advance")


STOP_SEQ_MAX = 16          # include/bitdelta_hip.h (BD_STOP_SEQ_MAX / BD_STOP_SEQ_LEN_MAX): sequences per request, ids per sequence
STOP_SEQ_LEN_MAX = 32


def step_stop_sequences(out, n, ss_n, seq_tok, seq_len, hit, hold, active, done):
    """The LAST launch of a ragged step, behind the step end, step_logprobs and step_constrain_advance: for every tenant whose token count n[t]
    moved past the launch's own counter ss_n[t] (which then follows it), hit[t] = the lowest q whose stop sequence seq_tok[t, q, :seq_len[t, q]]
    ends this turn's tokens out[t, :n[t]] (-1: none) and hold[t] = the longest proper prefix of a sequence those tokens end with (0 on a hit); a
    hit retires the tenant: active[t] = 0, done[t] |= 16 -- also next to the reason of a tenant the step end retired in this step.
    include/bitdelta_hip.h (bd_srv_step_stop_sequences) is the definition.  out [T, cap] long, rows may be strided; n, ss_n [T] long; seq_tok
    int32 [T, Q, W] and seq_len int32 [T, Q], Q <= 16, W <= 32; hit, hold int32 [T]; active, done [T] bool / uint8."""
    require_gpu(out, n, ss_n, seq_tok, seq_len, hit, hold, active, done)
    assert seq_tok.dim() == 3 and seq_tok.dtype == torch.int32 and seq_tok.is_contiguous()
    T, Q, W = seq_tok.shape
    assert 1 <= Q <= STOP_SEQ_MAX and 1 <= W <= STOP_SEQ_LEN_MAX
    assert seq_len.shape == (T, Q) and seq_len.dtype == torch.int32 and seq_len.is_contiguous()
    assert out.dim() == 2 and out.dtype == torch.long and out.shape[0] == T and (out.stride(1) == 1 or out.shape[1] <= 1)
    cap = out.shape[1]
    s_out = out.stride(0) if T > 1 else cap
    assert s_out >= cap
    for x in (n, ss_n):
        assert x.dtype == torch.long and x.is_contiguous() and x.numel() == T
    for x in (hit, hold):
        assert x.dtype == torch.int32 and x.is_contiguous() and x.numel() == T
    for x in (active, done):
        assert x.dtype in (torch.bool, torch.uint8) and x.is_contiguous() and x.numel() == T
    with torch.cuda.device(out.device):
        check(lib().bd_srv_step_stop_sequences(ptr(out), s_out, cap, ptr(n), ptr(ss_n), ptr(seq_tok), ptr(seq_len), Q, W, ptr(hit), ptr(hold),
                                               ptr(active), ptr(done), T, stream_ptr()), "srv_step_stop_sequences")


BAN_NGRAM_MAX = 8          # include/bitdelta_hip.h (BD_BAN_NGRAM_MAX / BD_BAN_WORDS_MAX / BD_BAN_WORD_LEN_MAX / BD_BAN_STOP_MAX)
BAN_WORDS_MAX = 64
BAN_WORD_LEN_MAX = 32
BAN_STOP_MAX = 64


def _ban_args(logits, out, ctx, ctx_len, toks, n, ban_ngram, ban_tok, ban_len, ban_min, stop_ids):
    """the checks ban_rows and step_ban share; returns (out, Lc, toks pointer, s_tok, tok_cap, n pointer, Q, W, ns, stop_ids pointer)"""
    R, V = logits.shape
    assert logits.stride(1) == 1 and V % 8 == 0 and logits.dtype in (torch.float16, torch.bfloat16)
    if out is None:
        out = torch.empty((R, V), dtype=logits.dtype, device=logits.device)
    require_gpu(out, ctx, ctx_len, ban_ngram, ban_tok, ban_len, ban_min)
    assert out.shape == (R, V) and out.dtype == logits.dtype and out.stride(1) == 1
    assert ctx.dim() == 2 and ctx.shape[0] == R and ctx.dtype == torch.int32 and ctx.is_contiguous()
    Lc = ctx.shape[1]
    assert ban_tok.dim() == 3 and ban_tok.shape[0] == R and ban_tok.dtype == torch.int32 and ban_tok.is_contiguous()
    Q, W = ban_tok.shape[1:]
    assert 1 <= Q <= BAN_WORDS_MAX and 1 <= W <= BAN_WORD_LEN_MAX
    assert ban_len.shape == (R, Q) and ban_len.dtype == torch.int32 and ban_len.is_contiguous()
    for x in (ctx_len, ban_ngram, ban_min):
        assert x.dtype == torch.int32 and x.is_contiguous() and x.numel() == R
    tp, s_tok, cap, np_ = None, 0, 0, None
    if n is not None:
        require_gpu(toks, n)
        assert n.dtype == torch.long and n.is_contiguous() and n.numel() == R
        assert toks.dim() == 2 and toks.dtype == torch.long and toks.shape[0] == R and (toks.stride(1) == 1 or toks.shape[1] <= 1)
        cap = toks.shape[1]
        s_tok = toks.stride(0) if R > 1 else cap
        assert s_tok >= cap
        tp, np_ = ptr(toks), ptr(n)
    if stop_ids is None or stop_ids.shape[1] == 0:
        return out, Lc, tp, s_tok, cap, np_, Q, W, 0, None
    require_gpu(stop_ids)
    ns = stop_ids.shape[1]
    assert stop_ids.shape == (R, ns) and ns <= BAN_STOP_MAX and stop_ids.dtype == torch.long and stop_ids.is_contiguous()
    return out, Lc, tp, s_tok, cap, np_, Q, W, ns, ptr(stop_ids)


def ban_rows(logits, ctx, ctx_len, ban_ngram, ban_tok, ban_len, ban_min, stop_ids=None, toks=None, n=None, out=None):
    """The copy of logits [R, V] (16-bit, V % 8 == 0) with every token -inf that the row's no-repeat n-gram size, bad words or minimum turn length
    ban after its history, every other element keeping its bits; include/bitdelta_hip.h (bd_srv_ban_rows) is the definition.  The history of
    row r is ctx[r, :ctx_len[r]] (int32 [R, Lc], int32 [R]) followed by toks[r, :n[r]] (long [R, cap], rows may be strided; long [R]); n=None:
    no turn tokens yet (admission).  ban_ngram int32 [R] (0 = off); ban_tok int32 [R, Q, W] with ban_len int32 [R, Q] (0 = an unused slot);
    ban_min int32 [R]; stop_ids long [R, ns <= 64] (-1: an empty slot; None: no list), banned while n < ban_min.  Rows of logits may be strided
    (stride % 8 == 0, 16-byte aligned; logits of another layout are copied first, as in constrain_rows); out: a tensor of the logits' shape and
    dtype to write into instead of a new one."""
    require_gpu(logits)
    assert logits.dim() == 2
    R, V = logits.shape
    sl = logits.stride(0) if R > 1 else V
    if logits.stride(1) != 1 or sl % 8 or sl < V or logits.data_ptr() % 16:             # (token_logprobs' rule: such rows are copied first)
        logits, sl = logits.contiguous(), V
    out, Lc, tp, s_tok, cap, np_, Q, W, ns, sp = _ban_args(logits, out, ctx, ctx_len, toks, n, ban_ngram, ban_tok, ban_len, ban_min, stop_ids)
    with torch.cuda.device(logits.device):
        check(lib().bd_srv_ban_rows(ptr(logits), sl, V, ptr(out), out.stride(0) if R > 1 else V, ptr(ctx) if Lc else None, Lc, ptr(ctx_len), tp,
                                    s_tok, cap, np_, ptr(ban_ngram), ptr(ban_tok), ptr(ban_len), Q, W, ptr(ban_min), sp, ns, R,
                                    DTYPE_CODE[logits.dtype], stream_ptr()), "srv_ban_rows")
    return out


def step_ban(logits, out, ctx, ctx_len, toks, n, ban_ngram, ban_tok, ban_len, ban_min, stop_ids, active):
    """ban_rows inside a ragged decode step, logits [T, V] -> out [T, V], behind the lm_head, step_penalize and step_constrain and in front of the
    step end, which then reads `out`; toks / n are the step end's output rows and token counts.  An inactive tenant's row of out is not touched.
    The launch only reads: it keeps no counter.  active [T] bool / uint8."""
    require_gpu(logits, active)
    assert n is not None
    out, Lc, tp, s_tok, cap, np_, Q, W, ns, sp = _ban_args(logits, out, ctx, ctx_len, toks, n, ban_ngram, ban_tok, ban_len, ban_min, stop_ids)
    T, V = logits.shape
    assert active.dtype in (torch.bool, torch.uint8) and active.is_contiguous() and active.numel() == T
    with torch.cuda.device(logits.device):
        check(lib().bd_srv_step_ban(ptr(logits), logits.stride(0), V, ptr(out), out.stride(0), ptr(ctx) if Lc else None, Lc, ptr(ctx_len), tp,
                                    s_tok, cap, np_, ptr(ban_ngram), ptr(ban_tok), ptr(ban_len), Q, W, ptr(ban_min), sp, ns,
                                    ptr(active), T, DTYPE_CODE[logits.dtype], stream_ptr()), "srv_step_ban")
    return out


def _truncate_args(logits, out, tau, params):
    """the checks truncate_rows and step_truncate share; returns out"""
    R, V = logits.shape
    assert logits.stride(1) == 1 and V % 8 == 0 and logits.dtype in (torch.float16, torch.bfloat16)
    if out is None:
        out = torch.empty((R, V), dtype=logits.dtype, device=logits.device)
    require_gpu(out, tau, params)
    assert out.shape == (R, V) and out.dtype == logits.dtype and out.stride(1) == 1
    assert tau.dtype == torch.float32 and tau.is_contiguous() and tau.numel() == R
    assert params.dtype == torch.float32 and params.is_contiguous() and params.shape == (R, 4)
    return out


def truncate_rows(logits, tau, params, out=None):
    """The copy of logits [R, V] (16-bit, V % 8 == 0) with every element -inf that the row's min_p / typical_p / epsilon_cutoff / eta_cutoff drop at
    its temperature, every other element keeping its bits; include/bitdelta_hip.h (bd_srv_truncate_rows) is the definition.  tau float32 [R];
    params float32 [R, 4] = (min_p, typical_p, epsilon_cutoff, eta_cutoff) per row, (0, 1, 0, 0) = nothing.  A row with neutral parameters, a
    temperature outside (0, inf), a NaN, a +inf or nothing finite is copied bit for bit.  Rows of logits may be strided (stride % 8 == 0, 16-byte
    aligned; logits of another layout are copied first, as in ban_rows); out: a tensor of the logits' shape and dtype to write into instead of a
    new one (it must not overlap logits)."""
    require_gpu(logits)
    assert logits.dim() == 2
    R, V = logits.shape
    sl = logits.stride(0) if R > 1 else V
    if logits.stride(1) != 1 or sl % 8 or sl < V or logits.data_ptr() % 16:             # (token_logprobs' rule: such rows are copied first)
        logits, sl = logits.contiguous(), V
    out = _truncate_args(logits, out, tau, params)
    with torch.cuda.device(logits.device):
        check(lib().bd_srv_truncate_rows(ptr(logits), sl, V, ptr(out), out.stride(0) if R > 1 else V, ptr(tau), ptr(params), R,
                                         DTYPE_CODE[logits.dtype], stream_ptr()), "srv_truncate_rows")
    return out


def step_truncate(logits, out, tau, params, active):
    """truncate_rows inside a ragged decode step, logits [T, V] -> out [T, V], the last of the masks: behind the lm_head, step_penalize,
    step_constrain and step_ban and in front of step_end_sample, which then reads `out`; tau is the step end's temperature array.  An inactive
    tenant's row of out is not touched.  The launch only reads: it keeps no counter.  active [T] bool / uint8."""
    require_gpu(logits, active)
    assert logits.dim() == 2
    out = _truncate_args(logits, out, tau, params)
    T, V = logits.shape
    assert active.dtype in (torch.bool, torch.uint8) and active.is_contiguous() and active.numel() == T
    with torch.cuda.device(logits.device):
        check(lib().bd_srv_step_truncate(ptr(logits), logits.stride(0) if T > 1 else V, V, ptr(out), out.stride(0) if T > 1 else V, ptr(tau), ptr(params), ptr(active), T,
                                         DTYPE_CODE[logits.dtype], stream_ptr()), "srv_step_truncate")
    return out


def step_end_sample(logits, tok, out, n, pos, limit, stop_ids, active, done, cache_len, temperature, top_k, top_p, seed, dbg=None):
    """step_end_ragged with tenant t's token chosen by sample_rows' rule from (temperature[t], top_k[t], top_p[t], seed[t]) and the draw index
    pos[t] + 1 (the cache row the token will occupy); temperature[t] == 0 is step_end_ragged's token.  The parameters are device arrays [T]."""
    require_gpu(logits, tok, out, n, pos, limit, stop_ids, active, done, temperature, top_k, top_p, seed, dbg)
    T, V = logits.shape
    assert logits.stride(1) == 1 and V % 8 == 0 and tok.dtype == torch.long and tok.is_contiguous() and tok.numel() == T
    assert out.dtype == torch.long and out.shape[0] == T and out.stride(1) == 1 and stop_ids.dtype == torch.long and stop_ids.is_contiguous()
    assert stop_ids.shape[0] == T and active.dtype == torch.bool and active.is_contiguous() and active.numel() == T
    assert done.dtype == torch.uint8 and done.is_contiguous() and done.numel() == T
    for v in (n, pos, limit):
        assert v.dtype == torch.long and v.numel() == T and v.is_contiguous()
    _sampling_arrays(T, temperature, top_k, top_p, seed, dbg)
    with torch.cuda.device(logits.device):
        check(lib().bd_srv_step_end_sample(ptr(logits), logits.stride(0), V, ptr(tok), ptr(out), out.stride(0), out.shape[1], ptr(stop_ids),
                                           stop_ids.shape[1], ptr(pos), ptr(n), ptr(limit), ptr(active), ptr(done), int(cache_len),
                                           ptr(temperature), ptr(top_k), ptr(top_p), ptr(seed), ptr(dbg), T, DTYPE_CODE[logits.dtype],
                                           stream_ptr()), "srv_step_end_sample")


def rope_kv_append_(qkv, cos, sin, kcache, vcache, heads, kvh, pos0=0):
    """Prefill from position pos0: rope_ on the q and k heads of the fused projection output qkv [T, S, (heads + 2 kvh) * 128] (in place) and, in the
    same launch, the rotated k rows and the v rows into the caches [T, kvh, Lc, 128] at positions pos0 .. pos0 + S - 1 (what
    `kcache[:, :, pos0:pos0 + S] = k.transpose(1, 2)` and its v twin do after rope_).  cos / sin [Lmax, 128], or contiguous [T, Lmax, 128]: tenant
    t's own tables (bd_srv_rope_kv_append_tab).  Returns qkv."""
    T, S, W = qkv.shape
    s_tab = table_stride(cos, sin, T)
    require_gpu(qkv, cos, sin, kcache, vcache)
    assert W == (heads + 2 * kvh) * 128 and qkv.stride(2) == 1 and (T == 1 or qkv.stride(0) == S * qkv.stride(1))
    assert cos.is_contiguous() and sin.is_contiguous() and cos.dtype == qkv.dtype and cos.shape[-2] >= pos0 + S
    Lc = kcache.shape[2]
    assert kcache.shape == (T, kvh, Lc, 128) and vcache.shape == kcache.shape and kcache.is_contiguous() and vcache.is_contiguous()
    assert kcache.dtype == qkv.dtype and vcache.dtype == qkv.dtype and pos0 + S <= Lc
    with torch.cuda.device(qkv.device):
        if cos.dim() == 3:
            check(lib().bd_srv_rope_kv_append_tab(ptr(qkv), ptr(cos), ptr(sin), s_tab, ptr(kcache), ptr(vcache), T, S, heads, kvh, 128, qkv.stride(1),
                                                  Lc, pos0, DTYPE_CODE[qkv.dtype], stream_ptr()), "srv_rope_kv_append_tab")
            return qkv
        check(lib().bd_srv_rope_kv_append(ptr(qkv), ptr(cos), ptr(sin), ptr(kcache), ptr(vcache), T, S, heads, kvh, 128, qkv.stride(1), Lc, pos0,
                                          DTYPE_CODE[qkv.dtype], stream_ptr()), "srv_rope_kv_append")
    return qkv
