"""CPU-only checks of a tenant's rotary embedding as data (serving_loop.rope_spec / rope_inv_freq / rope_tables): the neutral spec is the table
every decoder had before, the frequencies are transformers' bit for bit, every refusal is raised before anything is touched, and the ops
wrappers refuse a per-tenant table pair whose leading dimension is not the launch's tenant count."""
import pytest
import torch

from bitdelta_amd import serving_ops as ops
from bitdelta_amd.serving_loop import (ROPE_DEFAULT, RopeSpec, TenantDecoder, _rope_tables, rope_inv_freq, rope_spec, rope_tables)

LLAMA3 = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_neutral_spec_is_the_table_every_decoder_had(dtype):
    cos0, sin0 = _rope_tables(96, 128, "cpu", dtype)
    for spec in (ROPE_DEFAULT, rope_spec(), rope_spec(10000), rope_spec(10000.0, {"rope_type": "default"})):
        cos, sin = rope_tables(96, 128, "cpu", dtype, spec)
        assert cos.dtype == dtype and cos.shape == (96, 128)
        assert torch.equal(cos, cos0) and torch.equal(sin, sin0)
    assert rope_spec() == ROPE_DEFAULT and hash(rope_spec()) == hash(ROPE_DEFAULT)
    # the arithmetic the tables were always made with, restated: fp32 angle, sign folded into sin, then the cast
    inv = 1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.float32) / 128))
    ang = torch.outer(torch.arange(96, dtype=torch.float32), inv)
    assert torch.equal(cos0, torch.cat([ang, ang], -1).cos().to(dtype))
    assert torch.equal(sin0, torch.cat([-ang.sin(), ang.sin()], -1).to(dtype))


def test_tables_follow_the_spec():
    """a linear factor changes the angle of EVERY position: row p of the factor-4 table is row p / 4 of the neutral one"""
    c1, s1 = rope_tables(96, 128, "cpu", torch.float32, rope_spec())
    c4, s4 = rope_tables(96, 128, "cpu", torch.float32, rope_spec(scaling={"type": "linear", "factor": 4.0}))
    assert torch.equal(c4[::4][:24], c1[:24]) and torch.equal(s4[::4][:24], s1[:24])          # (a power-of-two factor: exact)
    assert not torch.equal(c4[1], c1[1])
    inv = torch.linspace(1.0, 0.01, 64)
    cu, su = rope_tables(8, 128, "cpu", torch.float32, rope_spec(inv_freq=inv))
    assert torch.equal(rope_inv_freq(rope_spec(inv_freq=inv), 128), inv)
    ang = torch.outer(torch.arange(8, dtype=torch.float32), inv)
    assert torch.equal(cu, torch.cat([ang, ang], -1).cos()) and torch.equal(su, torch.cat([-ang.sin(), ang.sin()], -1))


def _hf_inv_freq(kind, theta, extra):
    """transformers' own frequencies for a LlamaConfig with the same fields (head_dim 128).  The installed transformers keeps "linear" and
    "llama3" in ROPE_INIT_FUNCTIONS; the unscaled definition left that table in 5.x and lives on the model's rotary module."""
    mru = pytest.importorskip("transformers.modeling_rope_utils")
    from transformers import LlamaConfig
    params = dict(extra or {"rope_type": "default"}, rope_theta=theta)
    try:
        cfg = LlamaConfig(hidden_size=512, num_attention_heads=4, max_position_embeddings=32768, rope_parameters=params)
    except TypeError:                                                   # transformers 4.x: rope_theta / rope_scaling
        cfg = LlamaConfig(hidden_size=512, num_attention_heads=4, max_position_embeddings=32768, rope_theta=theta, rope_scaling=extra)
    if kind in mru.ROPE_INIT_FUNCTIONS:
        inv, attention_factor = mru.ROPE_INIT_FUNCTIONS[kind](cfg, "cpu")
    else:
        from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding
        inv, attention_factor = LlamaRotaryEmbedding.compute_default_rope_parameters(cfg, "cpu")
    assert attention_factor == 1.0
    return inv


@pytest.mark.parametrize("theta", [1e4, 1e6, 5e5])
@pytest.mark.parametrize("kind,extra", [("default", None), ("linear", {"rope_type": "linear", "factor": 4.0}),
                                        ("linear", {"rope_type": "linear", "factor": 3.0}), ("llama3", LLAMA3)])
def test_inv_freq_is_transformers_bit_for_bit(theta, kind, extra):
    hf = _hf_inv_freq(kind, theta, extra)
    ours = rope_inv_freq(rope_spec(theta, extra), 128)
    assert ours.dtype == torch.float32 and ours.shape == (64,)
    bad = (ours != hf).nonzero().flatten().tolist()
    assert not bad, [(i, float(ours[i]), float(hf[i])) for i in bad]
    if kind == "linear":                                                # (current transformers scales the frequencies: exactly base / factor)
        assert torch.equal(ours, rope_inv_freq(rope_spec(theta), 128) / extra["factor"])


def test_linear_scaling_of_the_position_agrees_at_power_of_two_factors():
    """transformers 4.31 (the reference's pin) divides the POSITION by the factor, current transformers the frequency: the fp32 angles are the
    same bits at a power-of-two factor (vicuna-16k's 4) and within an ulp of the angle elsewhere"""
    pos = torch.arange(4096, dtype=torch.float32)
    base = rope_inv_freq(rope_spec(), 128)
    for factor, exact in ((4.0, True), (2.0, True), (3.0, False)):
        new = torch.outer(pos, rope_inv_freq(rope_spec(scaling={"type": "linear", "factor": factor}), 128))
        old = torch.outer(pos / factor, base)
        if exact:
            assert torch.equal(new, old)
        else:
            assert not torch.equal(new, old)
            # two roundings on each side (the division, the product), 2^-24 relative each: |new - old| <= 4 * 2^-24 * angle (+ second order)
            ulp = torch.finfo(torch.float32).eps * old.abs()
            assert bool(((new - old).abs() <= 2.25 * ulp).all())


@pytest.mark.parametrize("kwargs", [
    dict(scaling={"rope_type": "dynamic", "factor": 2.0}),
    dict(scaling={"rope_type": "yarn", "factor": 4.0}),
    dict(scaling={"rope_type": "longrope", "factor": 4.0}),
    dict(scaling={"type": "ntk-by-parts", "factor": 2.0}),
    dict(scaling={"rope_type": "linear", "factor": 0.5}),
    dict(scaling={"rope_type": "linear"}),
    dict(scaling={"rope_type": "linear", "factor": float("nan")}),
    dict(scaling={"rope_type": "llama3", "factor": 8.0}),
    dict(scaling="linear"),
    dict(theta=0.0), dict(theta=-1.0), dict(theta=float("inf")), dict(theta=float("nan")), dict(theta="big"),
    dict(inv_freq=[1.0, float("nan")]), dict(inv_freq=[1.0, float("inf")]), dict(inv_freq=[]), dict(inv_freq=[[1.0, 0.5]]),
    dict(inv_freq=[1.0] * 64, scaling={"rope_type": "linear", "factor": 2.0}),
])
def test_rope_spec_refusals(kwargs):
    with pytest.raises(ValueError):
        rope_spec(**kwargs)


def test_spec_records_are_values():
    a = rope_spec(1e6, {"type": "linear", "factor": 4})
    b = rope_spec(1000000, {"rope_type": "linear", "factor": 4.0})
    assert isinstance(a, RopeSpec) and a == b and hash(a) == hash(b) and a != rope_spec(1e6)
    assert rope_spec(inv_freq=torch.ones(64)) == rope_spec(inv_freq=[1.0] * 64) and len({a, b, rope_spec()}) == 2
    with pytest.raises(ValueError):
        rope_inv_freq(rope_spec(inv_freq=[1.0] * 32), 128)              # the length meets the head size here
    with pytest.raises(ValueError):
        rope_inv_freq((10000.0, "default"), 128)                        # not a rope_spec() record


def test_decoder_takes_and_refuses_specs_on_the_host():
    """construction on the CPU builds tables only (no kernel runs): shapes, tenant_rope, and the refusals before anything exists"""
    lin4, big = rope_spec(scaling={"type": "linear", "factor": 4.0}), rope_spec(1e6)
    d0 = TenantDecoder((512, 1024, 2, 4, 1, 512), 3, "cpu", torch.float16, max_len=96)
    assert d0.cos.shape == (96, 128) and not d0.rope_per_tenant and [d0.tenant_rope(t) for t in range(3)] == [ROPE_DEFAULT] * 3
    assert torch.equal(d0.cos, _rope_tables(96, 128, "cpu", torch.float16)[0])
    d1 = TenantDecoder((512, 1024, 2, 4, 1, 512), 3, "cpu", torch.float16, max_len=96, rope=big)
    assert d1.cos.shape == (96, 128) and not d1.rope_per_tenant and d1.tenant_rope(2) == big
    assert torch.equal(d1.sin, rope_tables(96, 128, "cpu", torch.float16, big)[1])
    d3 = TenantDecoder((512, 1024, 2, 4, 1, 512), 3, "cpu", torch.float16, max_len=96, rope=[ROPE_DEFAULT, lin4, big])
    assert d3.cos.shape == (3, 96, 128) and d3.sin.shape == (3, 96, 128) and d3.cos.is_contiguous() and d3.rope_per_tenant
    assert [d3.tenant_rope(t) for t in range(3)] == [ROPE_DEFAULT, lin4, big]
    for t, sp in enumerate((ROPE_DEFAULT, lin4, big)):
        c, s = rope_tables(96, 128, "cpu", torch.float16, sp)
        assert torch.equal(d3.cos[t], c) and torch.equal(d3.sin[t], s)
    assert torch.equal(d3.cos[0], d0.cos)
    # the stock-op arm's gather: [S, D] from a shared table, [T, 1, S, D] (broadcast over the heads) from per-tenant tables
    pos = torch.tensor([3, 7])
    assert d0._rope_rows(pos)[0].shape == (2, 128) and d3._rope_rows(pos)[0].shape == (3, 1, 2, 128)
    assert torch.equal(d3._rope_rows(pos)[1][1, 0], d3.sin[1][pos])
    for bad in ([ROPE_DEFAULT, lin4], [ROPE_DEFAULT, lin4, (1e6,)], rope_spec(inv_freq=[1.0] * 32), "linear"):
        with pytest.raises(ValueError):
            TenantDecoder((512, 1024, 2, 4, 1, 512), 3, "cpu", torch.float16, max_len=96, rope=bad)
    # a load's refusals are decided before the first write: a shared-table decoder cannot give one slot another spec
    with pytest.raises(ValueError):
        d1._load_rope(0, lin4)
    assert d1._load_rope(0, None) == big and d1._load_rope(0, big) == big and d0._load_rope(1, None) == ROPE_DEFAULT
    assert d3._load_rope(1, None) == ROPE_DEFAULT and d3._load_rope(1, big) == big
    with pytest.raises(ValueError):
        d3._load_rope(1, rope_spec(inv_freq=[1.0] * 32))
    assert d3.tenant_rope(1) == lin4 and d1.tenant_rope(0) == big


def test_wrappers_refuse_tables_of_another_tenant_count():
    """a [T', Lmax, 128] pair in a launch of T != T' tenants is refused on the host, before the device check and before any launch"""
    T, S, heads, kvh, Lc = 3, 4, 4, 2, 16
    cos2, sin2 = torch.zeros(Lc, 128, dtype=torch.float16), torch.zeros(Lc, 128, dtype=torch.float16)
    cos3, sin3 = torch.zeros(T, Lc, 128, dtype=torch.float16), torch.zeros(T, Lc, 128, dtype=torch.float16)
    assert ops.table_stride(cos2, sin2, T) == 0 and ops.table_stride(cos3, sin3, T) == Lc * 128
    for bad_T in (1, 2, 4):
        with pytest.raises((AssertionError, ValueError)):
            ops.table_stride(cos3, sin3, bad_T)
    with pytest.raises((AssertionError, ValueError)):
        ops.table_stride(cos3, sin2, T)
    with pytest.raises((AssertionError, ValueError)):
        ops.table_stride(cos3[None], sin3[None], T)
    qkv = torch.zeros(T + 1, S, (heads + 2 * kvh) * 128, dtype=torch.float16)
    kc = torch.zeros(T + 1, kvh, Lc, 128, dtype=torch.float16)
    valid = torch.zeros(T + 1, Lc, dtype=torch.bool)
    pos, active = torch.zeros(T + 1, dtype=torch.long), torch.ones(T + 1, dtype=torch.bool)
    calls = [lambda: ops.rope_(qkv[..., :heads * 128], cos3, sin3, heads, S, 0),
             lambda: ops.rope_kv_append_(qkv, cos3, sin3, kc, kc.clone(), heads, kvh, 0),
             lambda: ops.decode_attention(qkv[:, :1], cos3, sin3, kc, kc.clone(), valid, pos[:1], heads, kvh),
             lambda: ops.decode_attention_ragged(qkv[:, :1], cos3, sin3, kc, kc.clone(), valid, pos, active, heads, kvh)]
    for call in calls:
        with pytest.raises((AssertionError, ValueError)):
            call()


def test_tab_entries_check_the_stride_before_any_device_call():
    """bd_srv_*_tab: s_tab < 0, s_tab % 8 != 0 and a misaligned table pointer are BD_E_BAD_SHAPE from the host checks; NULL handling as in the originals"""
    import ctypes
    from bitdelta_amd._lib import SIGNATURES, lib
    L = lib()
    BAD_SHAPE, NULL = L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None), L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 0, None)
    for name in ("bd_srv_rope", "bd_srv_rope_kv_append", "bd_srv_decode_attention", "bd_srv_decode_attention_ragged"):
        old, new = SIGNATURES[name][1], SIGNATURES[name + "_tab"][1]
        assert len(new) == len(old) + 1 and new[3] is ctypes.c_int64 and new[:3] == old[:3] and new[4:] == old[3:]
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 15) & ~15                              # a 16-byte aligned host address: never dereferenced by the checks
    for s_tab, cos_p, want in ((4, a, BAD_SHAPE), (-8, a, BAD_SHAPE), (12, a, BAD_SHAPE), (0, a + 2, BAD_SHAPE), (2048, a + 8, BAD_SHAPE)):
        assert L.bd_srv_rope_tab(a, cos_p, a, s_tab, 4, 1, 128, 128, 2, 0, 0, None) == want
        assert L.bd_srv_rope_tab(a, a, cos_p, s_tab, 4, 1, 128, 128, 2, 0, 0, None) == want
        assert L.bd_srv_rope_kv_append_tab(a, cos_p, a, s_tab, a, a, 2, 2, 1, 1, 128, 384, 8, 0, 0, None) == want
        assert L.bd_srv_decode_attention_tab(a, cos_p, a, s_tab, a, a, a, a, a, 2, 4, 1, 128, 64, 768, 512, 0, None, 0, None) == want
        assert L.bd_srv_decode_attention_tab(a, a, cos_p, s_tab, a, a, a, a, a, 2, 4, 1, 128, 64, 768, 512, 0, None, 0, None) == want
        assert L.bd_srv_decode_attention_ragged_tab(a, cos_p, a, s_tab, a, a, a, a, a, a, 2, 4, 1, 128, 64, 768, 512, 0, None, 0, None) == want
    # NULL tables / an empty launch: as in the originals
    assert L.bd_srv_rope_tab(a, None, a, 2048, 4, 1, 128, 128, 2, 0, 0, None) == NULL
    assert L.bd_srv_rope_tab(None, None, None, 2048, 0, 1, 128, 128, 2, 0, 0, None) == 0
    assert L.bd_srv_rope_kv_append_tab(a, a, None, 2048, a, a, 2, 2, 1, 1, 128, 384, 8, 0, 0, None) == NULL
    assert L.bd_srv_decode_attention_tab(a, None, a, 2048, a, a, a, a, a, 2, 4, 1, 128, 64, 768, 512, 0, None, 0, None) == NULL
    assert L.bd_srv_decode_attention_ragged_tab(a, a, a, 2048, a, a, a, a, None, a, 2, 4, 1, 128, 64, 768, 512, 0, None, 0, None) == NULL
    assert L.bd_srv_decode_attention_tab(None, None, None, 2048, None, None, None, None, None, 0, 4, 1, 128, 64, 768, 512, 0, None, 0, None) == 0
    # the entries without the argument never asked for aligned tables in the attention launch, and keep not asking: a NULL cache is what they see first
    assert L.bd_srv_decode_attention(a, a + 2, a, None, a, a, a, a, 2, 4, 1, 128, 64, 768, 512, 0, None, 0, None) == NULL
