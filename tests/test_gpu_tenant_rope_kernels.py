"""GPU tests of per-tenant rotary tables in the four launches that rotate (bd_srv_rope_tab, bd_srv_rope_kv_append_tab, bd_srv_decode_attention_tab,
bd_srv_decode_attention_ragged_tab; serving_ops routes a [T, Lmax, 128] table pair to them).  The oracle is the shared-table entry, itself pinned
to fp64 models by test_gpu_glue_exact.py and test_gpu_attention_exact.py: tenant t's rows of ONE launch on the stacked tables are, bit for bit,
tenant t's rows of the same launch on table t alone -- same geometry, same instantiation, only the table address differs.  Three specs whose
tables differ everywhere: neutral, linear factor 4, theta 1e6."""
import ctypes

import numpy as np
import pytest
import torch

import glue_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
DT_ID = {torch.float16: "f16", torch.bfloat16: "bf16"}.get
NSPEC = 3


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def tables():
    """(dtype, length, T) -> ([(cos, sin)] of the three specs, stacked cos [T, length, 128], stacked sin); tenant t carries spec t % 3"""
    from bitdelta_amd.serving_loop import rope_spec, rope_tables
    specs = (rope_spec(), rope_spec(scaling={"rope_type": "linear", "factor": 4.0}), rope_spec(1e6))
    made = {}

    def get(dtype, length, T):
        key = (dtype, length, T)
        if key not in made:
            pairs = [rope_tables(length, 128, "cuda", dtype, sp) for sp in specs]
            for i in range(NSPEC):                                        # clearly different tables: from row 1 on, no two rows agree
                for j in range(i):
                    assert not bool((pairs[i][0][1:] == pairs[j][0][1:]).all(dim=1).any())
            made[key] = (pairs, torch.stack([pairs[t % NSPEC][0] for t in range(T)]).contiguous(),
                         torch.stack([pairs[t % NSPEC][1] for t in range(T)]).contiguous())
        return made[key]
    return get


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _code(dtype):
    from bitdelta_amd._lib import DTYPE_CODE
    return DTYPE_CODE[dtype]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _nan_fill(t):
    """a NaN pattern that is not the canonical NaN: a row the kernel must not touch cannot look untouched by accident"""
    t.view(torch.int16).fill_(0x7e5a if t.dtype == torch.float16 else 0x7fa5)
    return t


# ------------------------------------------------------------------------------------------------ rope_
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_rope_rows_follow_their_tenants_table(L, tables, dtype):
    from bitdelta_amd import serving_ops as ops
    T, seq, heads, pos0, PAD = 3, 5, 2, 3, 64
    W = heads * 128
    pairs, cos3, sin3 = tables(dtype, 16, T)
    gen = torch.Generator().manual_seed(11)
    full = torch.randn(T * seq, W + PAD, generator=gen).to(dtype)
    buf = full.cuda()
    x = buf.view(T, seq, W + PAD)[..., :W]                              # a strided view of a wider buffer
    assert not x.is_contiguous()
    assert ops.rope_(x, cos3, sin3, heads, seq, pos0) is x
    torch.cuda.synchronize()
    after = buf.cpu()
    assert torch.equal(_bits(after[:, W:]), _bits(full[:, W:])), "the padding between the rows changed"
    for t in range(T):
        alone = full.cuda()
        ops.rope_(alone.view(T, seq, W + PAD)[..., :W], pairs[t][0], pairs[t][1], heads, seq, pos0)
        rows = slice(t * seq, (t + 1) * seq)
        assert torch.equal(_bits(after[rows, :W]), _bits(alone.cpu()[rows, :W])), t
        for u in range(T):                                               # ... and not any other tenant's table
            if u != t:
                assert not torch.equal(_bits(after[u * seq:(u + 1) * seq, :W]), _bits(alone.cpu()[u * seq:(u + 1) * seq, :W])), (t, u)
        x64 = ref.to64(full[rows, :W]).reshape(seq, heads, 128)
        want, inter = ref.rope(x64, ref.to64(pairs[t][0]), ref.to64(pairs[t][1]), pos0 + np.arange(seq), dtype)
        v = ref.accept(after[rows, :W].reshape(seq, heads, 128), want, inter, np.ones(1), dtype, *ref.ROPE_LIMITS)
        print(f"TENANT-ROPE rope_ tenant {t} {DT_ID(dtype)}: worst ulp {v.worst_ulp}, bit-equal share {v.equal_share:.6f}")
        assert v.ok, (t, v)


# ------------------------------------------------------------------------------------------------ rope_kv_append_
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_rope_kv_append_rows_follow_their_tenants_table(L, tables, dtype):
    from bitdelta_amd import serving_ops as ops
    T, S, H, KVH, Lc, pos0 = 3, 4, 4, 2, 16, 5
    pairs, cos3, sin3 = tables(dtype, Lc, T)
    gen = torch.Generator().manual_seed(12)
    qkv0 = torch.randn(T, S, (H + 2 * KVH) * 128, generator=gen).to(dtype).cuda()

    def run(cos, sin):
        qkv = qkv0.clone()
        kc, vc = (_nan_fill(torch.empty(T, KVH, Lc, 128, dtype=dtype, device="cuda")) for _ in range(2))
        ops.rope_kv_append_(qkv, cos, sin, kc, vc, H, KVH, pos0)
        torch.cuda.synchronize()
        return qkv, kc, vc

    qkv, kc, vc = run(cos3, sin3)
    blank = _nan_fill(torch.empty(KVH, Lc, 128, dtype=dtype, device="cuda"))
    for t in range(T):
        q1, k1, v1 = run(*pairs[t])
        assert torch.equal(_bits(qkv[t]), _bits(q1[t])), t                          # q and k heads rotated, v heads as they were
        assert torch.equal(_bits(kc[t]), _bits(k1[t])) and torch.equal(_bits(vc[t]), _bits(v1[t])), t
        assert torch.equal(_bits(qkv[t, :, (H + KVH) * 128:]), _bits(qkv0[t, :, (H + KVH) * 128:]))
        # the cache rows [5, 9) are the rotated k rows / the raw v rows; every other row keeps its NaN pattern
        k_rows = qkv[t, :, H * 128:(H + KVH) * 128].reshape(S, KVH, 128).transpose(0, 1)
        v_rows = qkv0[t, :, (H + KVH) * 128:].reshape(S, KVH, 128).transpose(0, 1)
        assert torch.equal(_bits(kc[t, :, pos0:pos0 + S]), _bits(k_rows)) and torch.equal(_bits(vc[t, :, pos0:pos0 + S]), _bits(v_rows))
        for c in (kc, vc):
            assert torch.equal(_bits(c[t, :, :pos0]), _bits(blank[:, :pos0])) and torch.equal(_bits(c[t, :, pos0 + S:]), _bits(blank[:, pos0 + S:]))
        for u in range(T):
            if u != t:
                assert not torch.equal(_bits(qkv[u]), _bits(q1[u])), (t, u)


# ------------------------------------------------------------------------------------------------ decode attention
def _attention(L, ragged, qkv, cos, sin, s_tab, kc, vc, valid, pos, active, heads, kvh):
    """the scalar or the ragged launch through the C entry -- the *_tab sibling when s_tab is not None -- into an output pre-filled with a NaN
    pattern.  Returns (out, last attention form, workspace)."""
    from bitdelta_amd._lib import check, workspace
    T, Lc = qkv.shape[0], kc.shape[2]
    out = _nan_fill(torch.empty(T, 1, heads * 128, device=qkv.device, dtype=qkv.dtype))
    need = L.bd_srv_decode_attention_workspace_bytes(T, heads, kvh, 128, Lc)
    ws, need = workspace(need, qkv.device, zeroed=True) if need > 0 else (None, 0)
    name = "bd_srv_decode_attention" + ("_ragged" if ragged else "") + ("_tab" if s_tab is not None else "")
    args = [_p(qkv), _p(cos), _p(sin)] + ([s_tab] if s_tab is not None else []) + [_p(kc), _p(vc), _p(valid), _p(pos)]
    args += ([_p(active)] if ragged else []) + [_p(out), T, heads, kvh, 128, Lc, qkv.stride(0), out.stride(0), _code(qkv.dtype), _p(ws), need, _stream()]
    check(getattr(L, name)(*args), name)
    torch.cuda.synchronize()
    return out, L.bd_last_attention_form(), ws


ATTN_CASES = [(dt, 4, h, k, Lc) for dt in DTYPES for h, k in ((8, 2), (4, 4), (8, 1)) for Lc in (96, 320)]
ATTN_CASES += [(dt, 12, 8, 2, 320) for dt in DTYPES]                       # 24 (tenant, kv head) pairs: the rule keeps 4 splits


@pytest.mark.parametrize("dtype,T,heads,kvh,Lc", ATTN_CASES)
def test_attention_rows_follow_their_tenants_table(L, tables, dtype, T, heads, kvh, Lc):
    """Row t of ONE launch on the stacked tables == row t of the same-T launch on table t % 3 alone, bit for bit: output, appended k / v row,
    validity bytes; the same instantiation and split count in both arms; tickets back at zero.  Lc 96 runs unsplit, 320 split (T = 4: the
    MAXS = 16 merge; T = 12: the 4-split merge).  Scalar form at six positions, ragged form at two position sets, then tenants that stay out."""
    from bitdelta_amd import serving_ops as ops
    pairs, cos3, sin3 = tables(dtype, Lc, T)
    s_tab = Lc * 128
    g = torch.Generator(device="cuda").manual_seed(heads * 1000 + kvh * 100 + Lc)
    qkv = torch.randn(T, 1, (heads + 2 * kvh) * 128, device="cuda", generator=g).to(dtype)
    kc0 = torch.randn(T, kvh, Lc, 128, device="cuda", generator=g).to(dtype)
    vc0 = torch.randn(T, kvh, Lc, 128, device="cuda", generator=g).to(dtype)
    mid = Lc // 2 + 5                                            # inside a middle split, not on an iteration boundary
    pads = [0, 3, 17, 30]
    act_all = torch.ones(T, dtype=torch.bool, device="cuda")

    def base_valid(pos_l):
        v = torch.zeros(T, Lc, dtype=torch.bool, device="cuda")
        for t, p in enumerate(pos_l):
            if 0 < p <= Lc:
                v[t, min(pads[t % 4], p - 1):min(p, Lc)] = True  # a different left padding per tenant; nothing at or beyond its position
        return v

    def both_arms(ragged, pos_l, active):
        """the launch on the stacked tables, and on each of the three tables alone; returns (out, kc, vc, valid) and asserts the comparison"""
        valid0 = base_valid(pos_l)
        pos = torch.tensor(pos_l if ragged else pos_l[:1], device="cuda")
        kc, vc, valid = kc0.clone(), vc0.clone(), valid0.clone()
        out, form, ws = _attention(L, ragged, qkv, cos3, sin3, s_tab, kc, vc, valid, pos, active, heads, kvh)
        if ws is not None:
            assert int(ws[:16384].max()) == 0                    # tickets back at zero
        differs = 0
        for i in range(NSPEC):
            k_, v_, vl_ = kc0.clone(), vc0.clone(), valid0.clone()
            o_, form_s, _ = _attention(L, ragged, qkv, pairs[i][0], pairs[i][1], None, k_, v_, vl_, pos, active, heads, kvh)
            assert form == form_s, (hex(form), hex(form_s))      # the same instantiation and split count
            for t in range(T):
                if t % NSPEC == i:
                    assert torch.equal(_bits(out[t]), _bits(o_[t])), (t, pos_l)
                    assert torch.equal(_bits(kc[t]), _bits(k_[t])) and torch.equal(_bits(vc[t]), _bits(v_[t])) and torch.equal(valid[t], vl_[t]), (t, pos_l)
                elif bool(active[t]) and 0 < pos_l[t if ragged else 0] < Lc:
                    differs += int(not torch.equal(_bits(out[t]), _bits(o_[t])))
        return out, kc, vc, valid, valid0, form, differs

    for p in (0, 33, mid, Lc - 1, 31, 32):                       # scalar form: every tenant at p
        out, kc, vc, valid, valid0, form, differs = both_arms(False, [p] * T, act_all)
        assert bool(valid[:, p].all()) and torch.equal(kc[:, :, :p], kc0[:, :, :p]) and torch.equal(kc[:, :, p + 1:], kc0[:, :, p + 1:])
        assert p == 0 or differs > 0                             # (another tenant's table gives other bits: the comparison can fail)
        # the wrapper routes a 3-D pair to the same entry
        k_, v_, vl_ = kc0.clone(), vc0.clone(), valid0.clone()
        o_ = ops.decode_attention(qkv, cos3, sin3, k_, v_, vl_, torch.tensor([p], device="cuda"), heads, kvh)
        assert torch.equal(_bits(o_), _bits(out)) and torch.equal(_bits(k_), _bits(kc)) and torch.equal(vl_, valid)
    nsplit, maxs = form & 0xff, (form >> 16) & 0xff
    assert (nsplit == 1) == (Lc < 256), hex(form)
    assert Lc < 256 or ((nsplit, maxs) == (4, 4) if T == 12 else (nsplit > 4 and maxs == 16)), hex(form)

    live = {}
    for pos_l in ([0, 33, mid, Lc - 1], [31, 32, Lc - 1, mid]):  # ragged form: one position per tenant
        pos_l = (pos_l * 3)[:T]
        out, kc, vc, valid, valid0, form, differs = both_arms(True, pos_l, act_all)
        assert differs > 0
        for t, p in enumerate(pos_l):
            assert bool(valid[t, p]) and torch.equal(kc[t, :, :p], kc0[t, :, :p]) and torch.equal(kc[t, :, p + 1:], kc0[t, :, p + 1:])
        k_, v_, vl_ = kc0.clone(), vc0.clone(), valid0.clone()
        o_ = ops.decode_attention_ragged(qkv, cos3, sin3, k_, v_, vl_, torch.tensor(pos_l, device="cuda"), act_all, heads, kvh)
        assert torch.equal(_bits(o_), _bits(out)) and torch.equal(_bits(k_), _bits(kc)) and torch.equal(vl_, valid)
        live[tuple(pos_l)] = (out, kc, vc, valid)

    # tenants that stay out, exactly as with one table: tenant 1 inactive, tenant 2 at pos == Lc.  The others are as before.
    pos_l = ([0, 33, mid, Lc - 1] * 3)[:T]
    out_a, kc_a, vc_a, valid_a = live[tuple(pos_l)]
    pos2, act2 = list(pos_l), [True] * T
    act2[1], pos2[2] = False, Lc
    out, kc, vc, valid, valid0, _, _ = both_arms(True, pos2, torch.tensor(act2, device="cuda"))
    for t in range(T):
        if t in (1, 2):
            assert int(out[t].view(torch.int16).abs().max()) == 0, t                        # exactly zero (+0.0 bits)
            assert torch.equal(kc[t], kc0[t]) and torch.equal(vc[t], vc0[t]) and torch.equal(valid[t], valid0[t]), t
        else:
            assert torch.equal(_bits(out[t]), _bits(out_a[t])) and torch.equal(kc[t], kc_a[t]) and torch.equal(vc[t], vc_a[t]), t
            assert torch.equal(valid[t], valid_a[t]), t


# ------------------------------------------------------------------------------------------------ s_tab = 0 and the refusals
def _rope_args(x, cos, sin, s_tab, rows, heads, seq, pos0):
    return [_p(x), cos if isinstance(cos, ctypes.c_void_p) else _p(cos), _p(sin)] + ([s_tab] if s_tab is not None else []) + \
        [rows, heads, 128, x.stride(-2), seq, pos0, _code(x.dtype), _stream()]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_stride_zero_through_the_new_entries_is_the_old_entry(L, tables, dtype):
    T, S, H, KVH, Lc = 3, 4, 4, 1, 320
    pairs, _, _ = tables(dtype, Lc, T)
    cos, sin = pairs[1]
    gen = torch.Generator(device="cuda").manual_seed(5)
    x0 = torch.randn(T * S, (H + 2 * KVH) * 128, device="cuda", generator=gen).to(dtype)
    got, forms = [], []
    for s_tab in (None, 0):
        x = x0.clone()
        fn = L.bd_srv_rope if s_tab is None else L.bd_srv_rope_tab
        assert fn(*_rope_args(x[:, :H * 128], cos, sin, s_tab, T * S, H, S, 7)) == 0
        y = x0.clone()
        kc, vc = (_nan_fill(torch.empty(T, KVH, Lc, 128, dtype=dtype, device="cuda")) for _ in range(2))
        fn = L.bd_srv_rope_kv_append if s_tab is None else L.bd_srv_rope_kv_append_tab
        assert fn(*([_p(y), _p(cos), _p(sin)] + ([0] if s_tab is not None else []) + [_p(kc), _p(vc), T, S, H, KVH, 128, y.stride(0), Lc, 9,
                                                                                      _code(dtype), _stream()])) == 0
        torch.cuda.synchronize()
        res = [x, y, kc, vc]
        qkv = x0[:T].clone().view(T, 1, -1)
        for ragged in (False, True):
            kd = torch.randn(T, KVH, Lc, 128, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6)).to(dtype)
            vd, valid = kd.flip(2).contiguous(), torch.zeros(T, Lc, dtype=torch.bool, device="cuda")
            valid[:, 2:200] = True
            pos = torch.tensor([200, 150, 37] if ragged else [200], device="cuda")
            if ragged:
                for t, p in enumerate(pos.tolist()):
                    valid[t, p:] = False
            out, form, _ = _attention(L, ragged, qkv, cos, sin, s_tab, kd, vd, valid, pos, torch.ones(T, dtype=torch.bool, device="cuda"), H, KVH)
            res += [out, kd, vd, valid.to(dtype)]
            forms.append(form)
        got.append(res)
    assert forms[:2] == forms[2:] and all(f & 0xff > 1 for f in forms), [hex(f) for f in forms]      # (split launches, the same in both arms)
    for a, b in zip(*got):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_bad_stride_and_misaligned_tables_are_refused_before_the_launch(L, tables, dtype):
    """s_tab = 4 and a table pointer off by one element: BD_E_BAD_SHAPE from all four entries, and what the launch would have written is untouched"""
    BAD_SHAPE = L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None)
    T, S, H, KVH, Lc = 3, 4, 4, 1, 32
    _, cos3, sin3 = tables(dtype, Lc, T)
    off = ctypes.c_void_p(cos3.data_ptr() + 2)
    gen = torch.Generator(device="cuda").manual_seed(8)
    x0 = torch.randn(T * S, (H + 2 * KVH) * 128, device="cuda", generator=gen).to(dtype)
    for s_tab, cos in ((4, _p(cos3)), (Lc * 128, off)):
        x = x0.clone()
        kc, vc = (_nan_fill(torch.empty(T, KVH, Lc, 128, dtype=dtype, device="cuda")) for _ in range(2))
        out = _nan_fill(torch.empty(T, 1, H * 128, dtype=dtype, device="cuda"))
        valid = torch.ones(T, Lc, dtype=torch.bool, device="cuda")
        pos, active = torch.full((T,), 5, device="cuda"), torch.ones(T, dtype=torch.bool, device="cuda")
        assert L.bd_srv_rope_tab(*_rope_args(x[:, :H * 128], cos, sin3, s_tab, T * S, H, S, 0)) == BAD_SHAPE
        assert L.bd_srv_rope_kv_append_tab(_p(x), cos, _p(sin3), s_tab, _p(kc), _p(vc), T, S, H, KVH, 128, x.stride(0), Lc, 0, _code(dtype),
                                           _stream()) == BAD_SHAPE
        assert L.bd_srv_decode_attention_tab(_p(x), cos, _p(sin3), s_tab, _p(kc), _p(vc), _p(valid), _p(pos), _p(out), T, H, KVH, 128, Lc, S * x.stride(0),
                                             out.stride(0), _code(dtype), None, 0, _stream()) == BAD_SHAPE
        assert L.bd_srv_decode_attention_ragged_tab(_p(x), cos, _p(sin3), s_tab, _p(kc), _p(vc), _p(valid), _p(pos), _p(active), _p(out), T, H, KVH, 128,
                                                    Lc, S * x.stride(0), out.stride(0), _code(dtype), None, 0, _stream()) == BAD_SHAPE
        torch.cuda.synchronize()
        blank = _nan_fill(torch.empty_like(kc))
        assert torch.equal(_bits(x), _bits(x0)) and torch.equal(_bits(kc), _bits(blank)) and torch.equal(_bits(vc), _bits(blank))
        assert torch.equal(_bits(out), _bits(_nan_fill(torch.empty_like(out)))) and bool(valid.all())
