"""The three e4m3 KV-cache kernels (csrc/bd_attn_kv8.h) against the definition in include/bitdelta_hip.h, through serving_ops and the C ABI.
Appended bytes: the parent's 16-bit entry on the same inputs gives the row a 16-bit cache would hold; the kv8 launch must store
quantise(that row) = (x.float() * inv).clamp(-448, 448).to(float8_e4m3fn), computed with torch on the CPU, bit for bit.
Output: fp64 softmax attention over the DEVICE's cache bytes after the launch, times the scales, under `valid`; q from the fp64 RoPE model of
tests/glue_ref.py.  fp8 -> fp32 is exact, so the bound is the one tests/test_gpu_attention_exact.py holds the 16-bit decode kernel to against fp64:
|got - ref| <= 2u P|V| + tiny per element (u = 2^-11 fp16 / 2^-8 bf16, its RANGE_C = 1).
Visibility: rows above pos, rows with valid = 0 and (T > 1) every row of the last tenant set to byte 0x7f (NaN) change no bit of the others' output."""
import ctypes

import pytest
import torch

import glue_ref

pytestmark = pytest.mark.gpu
HD, DEV, F8 = 128, "cuda", torch.float8_e4m3fn
DT_ID = {torch.float16: "f16", torch.bfloat16: "bf16"}
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}          # tests/test_gpu_attention_exact.py: UNIT, TINY, RANGE_C = 1
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}
# (left pads, per-tenant rotary tables, random scales): every pair of values occurs
VARIANTS = {"pad0-shared-s1": (0, False, False), "pad5-shared-rand": (5, False, True), "pad0-tenant-rand": (0, True, True), "pad5-tenant-s1": (5, True, False)}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib, serving_ops
    _lib.lib()
    return serving_ops


def quantise(x16, inv):                                                   # the definition, on the CPU: x16 [T, KVH, ..., 128], inv [T, KVH] fp32
    inv = inv.cpu().view(*inv.shape, *([1] * (x16.dim() - 2)))
    return (x16.cpu().float() * inv).clamp(-448.0, 448.0).to(F8)


def u8(x):
    return x.view(torch.uint8)


def deq(c8):                                                              # float8_e4m3fn -> fp64, through the 256-entry table of the CPU cast
    return torch.arange(256, dtype=torch.uint8).view(F8).double().to(c8.device)[u8(c8).long()]


def make(ops, T, heads, kvh, Lc, dtype, per_tenant, rand_scale, seed):
    from bitdelta_amd.serving_loop import rope_spec, rope_tables
    g = torch.Generator().manual_seed(seed)
    sc = [(0.25 + 3.75 * torch.rand(T, kvh, generator=g)) if rand_scale else torch.ones(T, kvh) for _ in range(2)]
    (ks, ki), (vs, vi) = ops.kv8_scale_pair(sc[0], DEV), ops.kv8_scale_pair(sc[1], DEV)
    if per_tenant:
        pairs = [rope_tables(Lc, HD, DEV, dtype, rope_spec(theta=10000.0 * (t + 1))) for t in range(T)]
        cos, sin = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    else:
        cos, sin = rope_tables(Lc, HD, DEV, dtype)
    kc = quantise(torch.randn(T, kvh, Lc, HD, generator=g).to(dtype), ki).to(DEV)
    vc = quantise(torch.randn(T, kvh, Lc, HD, generator=g).to(dtype), vi).to(DEV)
    qkv = torch.randn(T, 1, (heads + 2 * kvh) * HD, generator=g).to(dtype).to(DEV)
    return qkv, cos, sin, kc, vc, ks, vs, ki, vi


def positions(ns, Lc):
    """0, 1, Lc - 1 and the largest pos just below / at / just above the first split boundary (per_split: whole iterations of 32 rows)"""
    out, best = {0, 1, Lc - 1}, {}
    for pos in range(Lc if ns > 1 else 0):
        per = ((pos + ns) // ns + 31) // 32 * 32
        c, r = divmod(pos, per)
        if (c == 0 and r == per - 1) or (c == 1 and r <= 1):
            best[(c, r == per - 1, r)] = pos
    return sorted(out | set(best.values()))


def check(out, qkv, cos, sin, kc, vc, ks, vs, valid, pos, heads, kvh, dtype, tag):
    """out against fp64 attention of each tenant's q heads at pos[t] over the cache bytes given, within 2u P|V| + tiny per element"""
    T, G = qkv.shape[0], heads // kvh
    q16 = qkv[:, 0, :heads * HD].view(T, heads, HD)
    q = torch.empty(T, heads, HD, dtype=torch.float64)
    for t in range(T):
        c, s = (cos[t], sin[t]) if cos.dim() == 3 else (cos, sin)
        q[t] = torch.from_numpy(glue_ref.rope(glue_ref.to64(q16[t:t + 1]), glue_ref.to64(c), glue_ref.to64(s), [pos[t]], dtype)[0][0])
    K = (deq(kc) * ks.double()[:, :, None, None]).repeat_interleave(G, dim=1)
    V = (deq(vc) * vs.double()[:, :, None, None]).repeat_interleave(G, dim=1)
    sc = torch.einsum("thd,thld->thl", q.to(DEV), K) / HD ** 0.5
    p = torch.softmax(sc.masked_fill(~valid[:, None, :], float("-inf")), dim=-1)
    ref, absv = torch.einsum("thl,thld->thd", p, V).reshape(T, -1), torch.einsum("thl,thld->thd", p, V.abs()).reshape(T, -1)
    err = (out[:, 0].double() - ref).abs()
    assert bool(torch.isfinite(out).all()), tag
    ratio = float(((err - TINY[dtype]).clamp_min(0) / (2 * UNIT[dtype] * absv.clamp_min(1e-300))).max())
    print(f"KV8 {tag}: max |err| / (2u P|V|) = {ratio:.3f}")
    assert ratio <= 1.0, (tag, ratio)


@pytest.mark.parametrize("dtype", list(DT_ID), ids=DT_ID.get)
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("Lc", [96, 320, 576])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("heads,kvh", [(2, 2), (4, 1), (8, 1)])
def test_decode_append_output_and_visibility(ops, heads, kvh, T, Lc, variant, dtype):
    from bitdelta_amd import _lib
    pad, per_tenant, rand_scale = VARIANTS[variant]
    qkv, cos, sin, kc0, vc0, ks, vs, ki, vi = make(ops, T, heads, kvh, Lc, dtype, per_tenant, rand_scale, Lc + heads + T)
    rows, pidx = torch.arange(Lc, device=DEV), torch.tensor([0], device=DEV)          # (one launch to learn the split count the library picks)
    ops.decode_attention_kv8(qkv, cos, sin, kc0.clone(), vc0.clone(), ks, vs, ki, vi, torch.zeros(T, Lc, dtype=torch.bool, device=DEV), pidx, heads, kvh)
    form = _lib.lib().bd_last_attention_form()
    ns = form & 0xff
    assert form >> 30 == 1 and (form >> 24) & 0x3f == heads // kvh and (ns > 1) == (Lc >= 256) and (T > 1 or Lc < 576 or ns == 16)
    for pos in positions(ns, Lc):
        tag = f"G={heads // kvh} T={T} Lc={Lc} {variant} {DT_ID[dtype]} pos={pos} nsplit={ns}"
        pidx = torch.tensor([pos], device=DEV)
        valid0 = ((rows >= min(pad, pos)) & (rows < pos) & (rows != pad + 2))[None].repeat(T, 1)
        # the row a 16-bit cache would hold: the parent's entry on the same inputs
        k16, v16 = (torch.zeros(T, kvh, Lc, HD, device=DEV, dtype=dtype) for _ in range(2))
        ops.decode_attention(qkv, cos, sin, k16, v16, valid0.clone(), pidx, heads, kvh)
        kc, vc, valid = kc0.clone(), vc0.clone(), valid0.clone()
        out = ops.decode_attention_kv8(qkv, cos, sin, kc, vc, ks, vs, ki, vi, valid, pidx, heads, kvh)
        assert torch.equal(u8(kc[:, :, pos]).cpu(), u8(quantise(k16[:, :, pos], ki))), f"{tag}: appended key bytes"
        assert torch.equal(u8(vc[:, :, pos]).cpu(), u8(quantise(v16[:, :, pos], vi))), f"{tag}: appended value bytes"
        other = rows != pos
        assert torch.equal(u8(kc)[:, :, other], u8(kc0)[:, :, other]) and torch.equal(u8(vc)[:, :, other], u8(vc0)[:, :, other]), f"{tag}: other rows"
        assert torch.equal(valid[:, other], valid0[:, other]) and bool(valid[:, pos].all()), f"{tag}: valid"
        check(out, qkv, cos, sin, kc, vc, ks, vs, valid, [pos] * T, heads, kvh, dtype, tag)
        # visibility: NaN bytes where nothing may be read
        kp, vp = u8(kc0.clone()), u8(vc0.clone())
        hidden = ~valid0 & other[None]                                    # rows above pos, pads, the hole (row pos itself is rewritten)
        for c in (kp, vp):
            c[hidden[:, None, :].expand(T, kvh, Lc)] = 0x7f
            if T > 1:
                c[T - 1] = 0x7f
        out_p = ops.decode_attention_kv8(qkv, cos, sin, kp.view(F8), vp.view(F8), ks, vs, ki, vi, valid0.clone(), pidx, heads, kvh)
        assert torch.equal(out_p[:max(T - 1, 1)].view(torch.int16), out[:max(T - 1, 1)].view(torch.int16)), f"{tag}: a hidden row was read"


@pytest.mark.parametrize("dtype", list(DT_ID), ids=DT_ID.get)
@pytest.mark.parametrize("heads,kvh,Lc", [(2, 2, 96), (4, 1, 320), (8, 1, 576)])
def test_ragged_stay_out_and_equal_positions(ops, heads, kvh, Lc, dtype):
    T = 3
    qkv, cos, sin, kc0, vc0, ks, vs, ki, vi = make(ops, T, heads, kvh, Lc, dtype, True, True, 7 + Lc)
    valid0 = torch.zeros(T, Lc, dtype=torch.bool, device=DEV)
    valid0[:, :Lc // 2] = True
    pos = Lc // 2
    run = lambda p, a, kc, vc, valid: ops.decode_attention_kv8(qkv, cos, sin, kc, vc, ks, vs, ki, vi, valid, p, heads, kvh, active=a)
    # equal positions: the scalar launch's bits
    a_s, a_r = [kc0.clone(), vc0.clone(), valid0.clone()], [kc0.clone(), vc0.clone(), valid0.clone()]
    out_s = run(torch.tensor([pos], device=DEV), None, *a_s)
    out_r = run(torch.full((T,), pos, device=DEV), torch.ones(T, dtype=torch.bool, device=DEV), *a_r)
    assert torch.equal(out_s.view(torch.int16), out_r.view(torch.int16)) and all(torch.equal(u8(x), u8(y)) for x, y in zip(a_s, a_r))
    # tenant 0 inactive, tenant 1 outside the cache (one launch each side of it), tenant 2 live at its own position
    for outside in (-1, Lc):
        kc, vc, valid = kc0.clone(), vc0.clone(), valid0.clone()
        p = torch.tensor([pos, outside, pos - 3], device=DEV)
        out = run(p, torch.tensor([False, True, True], device=DEV), kc, vc, valid)
        assert not bool(out[:2].any()) and torch.equal(u8(kc[:2]), u8(kc0[:2])) and torch.equal(u8(vc[:2]), u8(vc0[:2])) and torch.equal(valid[:2], valid0[:2])
        live = valid0 & (torch.arange(Lc, device=DEV) <= pos - 3)         # tenant 2 sees its rows up to its own position
        check(out[2:], qkv[2:], cos[2:], sin[2:], kc[2:], vc[2:], ks[2:], vs[2:], live[2:], [pos - 3], heads, kvh, dtype, f"ragged G={heads // kvh} Lc={Lc} {DT_ID[dtype]}")
    from bitdelta_amd._lib import _WORKSPACES
    assert all(not bool(b[:16384].any()) for bufs in _WORKSPACES.values() for b in bufs), "tickets are zero at exit"


@pytest.mark.parametrize("dtype", list(DT_ID), ids=DT_ID.get)
def test_saturation_and_nan(ops, dtype):
    T, heads, kvh, Lc = 1, 2, 2, 96
    qkv, cos, sin, kc, vc, ks, vs, ki, vi = make(ops, T, heads, kvh, Lc, dtype, False, False, 3)
    v0 = (heads + kvh) * HD
    qkv[0, 0, v0:v0 + 4] = torch.tensor([30000.0, -30000.0, float("nan"), 448.0], dtype=dtype)
    ks, ki = ops.kv8_scale_pair(torch.full((T, kvh), 0.25), DEV)             # |k| * 4 passes 448 for |k| > 112
    qkv[0, 0, heads * HD] = 20000.0
    cos, sin = torch.ones_like(cos), torch.zeros_like(sin)                    # (the identity rotation: the key is stored as given)
    ops.decode_attention_kv8(qkv, cos, sin, kc, vc, ks, vs, ki, vi, torch.zeros(T, Lc, dtype=torch.bool, device=DEV), torch.tensor([0], device=DEV), heads, kvh)
    assert u8(vc)[0, 0, 0, [0, 1, 3]].tolist() == [0x7e, 0xfe, 0x7e] and bool(vc[0, 0, 0, 2].float().isnan()) and u8(kc)[0, 0, 0, 0].item() == 0x7e
    x = torch.randn(T, 17, (heads + 2 * kvh) * HD).to(dtype).to(DEV)
    x[0, 3, v0:v0 + 3] = torch.tensor([30000.0, float("nan"), -30000.0], dtype=dtype)
    ops.rope_kv_append_kv8_(x, cos, sin, kc, vc, ki, vi, heads, kvh, 40)
    assert u8(vc)[0, 0, 43, [0, 2]].tolist() == [0x7e, 0xfe] and bool(vc[0, 0, 43, 1].float().isnan())


@pytest.mark.parametrize("dtype", list(DT_ID), ids=DT_ID.get)
@pytest.mark.parametrize("per_tenant", [False, True], ids=["shared", "tenant"])
@pytest.mark.parametrize("S,pos0", [(64, 0), (17, 0), (64, 40), (17, 40)])
def test_rope_kv_append_kv8_against_the_16_bit_entry(ops, S, pos0, per_tenant, dtype):
    T, heads, kvh, Lc = 3, 4, 2, 128
    _, cos, sin, kc, vc, ks, vs, ki, vi = make(ops, T, heads, kvh, Lc, dtype, per_tenant, True, S + pos0)
    x = torch.randn(T, S, (heads + 2 * kvh) * HD).to(dtype).to(DEV)
    x16, k16, v16 = x.clone(), torch.zeros(T, kvh, Lc, HD, device=DEV, dtype=dtype), torch.zeros(T, kvh, Lc, HD, device=DEV, dtype=dtype)
    ops.rope_kv_append_(x16, cos, sin, k16, v16, heads, kvh, pos0)
    kc0, vc0 = kc.clone(), vc.clone()
    ops.rope_kv_append_kv8_(x, cos, sin, kc, vc, ki, vi, heads, kvh, pos0)
    assert torch.equal(x.view(torch.int16), x16.view(torch.int16)), "qkv after the launch"
    new = slice(pos0, pos0 + S)
    assert torch.equal(u8(kc[:, :, new]).cpu(), u8(quantise(k16[:, :, new], ki))) and torch.equal(u8(vc[:, :, new]).cpu(), u8(quantise(v16[:, :, new], vi)))
    old = (torch.arange(Lc, device=DEV) < pos0) | (torch.arange(Lc, device=DEV) >= pos0 + S)
    assert torch.equal(u8(kc)[:, :, old], u8(kc0)[:, :, old]) and torch.equal(u8(vc)[:, :, old], u8(vc0)[:, :, old])


@pytest.mark.parametrize("dtype", list(DT_ID), ids=DT_ID.get)
@pytest.mark.parametrize("r0,r1", [(0, 96), (5, 38), (95, 96), (7, 7)])
def test_expand_bits_and_canary(ops, r0, r1, dtype):
    T, kvh, Lc = 3, 2, 96
    _, _, _, kc, vc, ks, vs, _, _ = make(ops, T, 4, kvh, Lc, dtype, False, True, r0 + r1)
    k16, v16 = (torch.full((T, kvh, Lc, HD), 7.0, device=DEV, dtype=dtype) for _ in range(2))
    ops.kv8_expand(kc, vc, ks, vs, k16, v16, r0, r1)
    for c8, sc, got in ((kc, ks, k16), (vc, vs, v16)):
        want = torch.full((T, kvh, Lc, HD), 7.0, dtype=dtype)
        want[:, :, r0:r1] = (c8.cpu().float() * sc.cpu()[:, :, None, None]).to(dtype)[:, :, r0:r1]
        assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


def test_refusals_in_the_documented_order(ops):
    from bitdelta_amd import _lib
    L, p, z = _lib.lib(), ctypes.c_void_p(4096), ctypes.c_void_p(0)          # p: non-NULL, aligned, never dereferenced -- validation comes first

    def call(heads=4, kvh=1, hd=128, kc=p, scale=p, dtype=0, T=1):
        return L.bd_srv_decode_attention_kv8(p, p, p, 0, kc, p, scale, p, p, p, p, p, z, p, T, heads, kvh, hd, 96, 768, 512, dtype, z, 0, z)
    BAD_SHAPE, BAD_DTYPE, NULL = call(heads=3, kvh=2), call(dtype=7), call(scale=z)
    assert len({0, BAD_SHAPE, BAD_DTYPE, NULL}) == 4 and L.bd_error_string(NULL) == b"null pointer"
    assert call(heads=2, kvh=1) == BAD_SHAPE and call(hd=64) == BAD_SHAPE and call(kc=ctypes.c_void_p(4104)) == BAD_SHAPE
    assert call(heads=2, kvh=1, scale=z) == NULL and call(heads=3, kvh=2, dtype=7, scale=z) == BAD_SHAPE and call(dtype=7, scale=z) == BAD_DTYPE
    assert call(T=0, scale=z, dtype=0) == 0 and L.bd_srv_rope_kv_append_kv8(p, p, p, 0, p, p, z, p, 1, 1, 4, 1, 128, 768, 96, 0, 0, z) == NULL
    assert L.bd_srv_kv8_expand(p, p, p, p, p, p, 1, 1, 128, 96, 5, 97, 0, z) == BAD_SHAPE and L.bd_srv_kv8_expand(p, p, z, p, p, p, 1, 1, 128, 96, 0, 9, 0, z) == NULL
