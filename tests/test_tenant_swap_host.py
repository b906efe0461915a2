"""Host side of loading one fine-tune into one tenant slot (no GPU): the C ABI's argument validation, the ONE definition of the fused column /
alpha-group rule against a literal restatement of what FusedDeltaLinear.__init__ used to spell out, and the Python refusals, which all come
before any launch."""
import math
import os

import pytest
import torch

from bitdelta_amd import _lib
from bitdelta_amd._lib import BitDeltaHipError


def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_abi_validates_before_any_device_work():
    f = L().bd_tenant_signs_load
    #      src   ld  KW  N_src mask ld_m packed Nf  t_pad slot off blk stride stream
    ok = (None, 48, 8, 48, None, 48, None, 48, 4, 1, 0, 48, 0, None)

    def call(**kw):
        names = ("src", "ld_src", "KW", "N_src", "mask", "ld_mask", "packed", "N_fused", "t_pad", "slot", "col_off", "col_blk", "col_stride", "stream")
        a = dict(zip(names, ok))
        a.update(kw)
        return f(*[a[n] for n in names])

    assert call() == -8                                          # everything valid but the pointers: BD_E_NULL, after the shape checks
    for tp in (0, 3, 5, 7, 9, 10, 14, 17, 32, -1):
        assert call(t_pad=tp, slot=0) == -5
    for tp in (1, 2, 4, 6, 8, 12, 16):
        assert call(t_pad=tp, slot=tp - 1) == -8 and call(t_pad=tp, slot=tp) == -5 and call(t_pad=tp, slot=-1) == -5
    assert call(col_blk=0) == -3 and call(col_blk=-8) == -3 and call(col_blk=32) == -3        # col_blk >= 1 and N_src % col_blk == 0
    assert call(col_off=1) == -5 and call(N_fused=47) == -5 and call(col_off=-1) == -5        # a mapped column outside N_fused
    assert call(N_fused=96, col_blk=8, col_stride=16, col_off=8) == -8                        # an interleaved pair's second half fits exactly
    assert call(N_fused=95, col_blk=8, col_stride=16, col_off=8) == -5
    assert call(N_fused=96, col_blk=8, col_stride=4) == -5                                    # blocks would overlap
    assert call(ld_src=47) == -5
    assert call(N_src=0, col_blk=1) == 0 and call(KW=0) == 0                                  # nothing to load: a no-op
    assert call(KW=-1) == -5 and call(N_src=-16, col_blk=16) == -5


def _literal_init_rule(weights, masks, coeffs, interleave8):
    """the lines FusedDeltaLinear.__init__ carried before the rule was factored out, restated"""
    widths = [w.shape[0] for w in weights]
    weight, mask = torch.cat(weights, 0), torch.cat(masks, 2)
    if interleave8:
        inter = widths[0]
        perm = torch.arange(2 * inter).view(2, inter // 8, 8).transpose(0, 1).reshape(-1)
        weight, mask = weight[perm], mask[:, :, perm]
        alpha = torch.stack([c.float().reshape(-1) for c in coeffs], 1)
        return weight, mask, alpha.repeat(1, inter // 8), alpha
    gsz = 0
    for n in widths:
        gsz = math.gcd(gsz, n)
    alpha = torch.cat([c.float().reshape(-1, 1).expand(-1, n // gsz) for c, n in zip(coeffs, widths)], 1)
    return weight, mask, alpha, None


def _parts(widths, K, T, gen):
    ws = [torch.randn(n, K, generator=gen).half() for n in widths]
    ms = [torch.randint(-2 ** 31, 2 ** 31 - 1, (T, K // 32, n), generator=gen, dtype=torch.int64).to(torch.int32) for n in widths]
    cs = [torch.rand(T, generator=gen) for _ in widths]
    return ws, ms, cs


@pytest.mark.parametrize("widths,inter8", [((32, 16, 16), False), ((24, 8, 8), False), ((48,), False), ((24, 24), True), ((512, 512), True),
                                           ((24, 24), False), ((6, 10), False)])
def test_column_and_alpha_helper_is_the_rule_init_used(widths, inter8):
    from bitdelta_amd.serving_loop import FusedDeltaLinear, fused_alpha, fused_columns, fused_perm
    gen = torch.Generator().manual_seed(5)
    T, K = 3, 128
    ws, ms, cs = _parts(widths, K, T, gen)
    weight, mask, alpha, pair = _literal_init_rule(ws, ms, cs, inter8)
    mod = FusedDeltaLinear(ws, ms, cs, interleave8=inter8, decode_copies=False)
    assert torch.equal(mod.weight, weight) and torch.equal(mod.mask, mask) and torch.equal(mod.alpha, alpha)
    assert (mod.alpha_pair is None) == (pair is None) and (pair is None or torch.equal(mod.alpha_pair, pair))
    gsz, maps = fused_columns(widths, inter8)
    perm = fused_perm(widths, inter8)
    assert mod.groups == sum(widths) // gsz and (perm is None) == (not inter8)
    if inter8:          # the permutation made from the maps is the one __init__ spelled out
        assert torch.equal(perm, torch.arange(2 * widths[0]).view(2, widths[0] // 8, 8).transpose(0, 1).reshape(-1))
    # the affine map of every projection lands on exactly the columns the permutation gives it
    cat_col = torch.arange(sum(widths)) if perm is None else perm          # stored column -> column of the plain concatenation
    off = 0
    for n_i, (c0, blk, stride) in zip(widths, maps):
        n = torch.arange(n_i)
        stored = c0 + (n // blk) * stride + n % blk
        assert torch.equal(cat_col[stored], off + n)
        off += n_i
    # one tenant's row through the helper = that row of the whole set's
    for t in range(T):
        a1, p1 = fused_alpha([c[t:t + 1] for c in cs], widths, inter8)
        assert torch.equal(a1[0], alpha[t]) and (pair is None or torch.equal(p1[0], pair[t]))
    # ... and tenant_signs undoes the fusion
    for t in range(T):
        m_t, c_t = mod.tenant_signs(t)
        for i in range(len(widths)):
            assert torch.equal(m_t[i], ms[i][t]) and float(c_t[i]) == float(cs[i][t])


def _cpu_linear(widths=(32, 16, 16), inter8=False, T=3, K=128):
    from bitdelta_amd.serving_loop import FusedDeltaLinear
    gen = torch.Generator().manual_seed(9)
    ws, ms, cs = _parts(widths, K, T, gen)
    return FusedDeltaLinear(ws, ms, cs, interleave8=inter8), ms, cs


def test_linear_refusals_come_before_any_launch():
    mod, ms, cs = _cpu_linear()
    before = [b.clone() for b in (mod.mask, mod.mask_packed, mod.alpha)]
    good_m, good_c = [m[1] for m in ms], [c[1] for c in cs]
    with pytest.raises(IndexError):
        mod.load_tenant(3, good_m, good_c)
    with pytest.raises(IndexError):
        mod.load_tenant(-1, good_m, good_c)
    with pytest.raises(ValueError):
        mod.load_tenant(0, good_m[:2], good_c[:2])                                     # a projection missing
    with pytest.raises(ValueError):
        mod.load_tenant(0, [good_m[0], good_m[1], good_m[2][:, :8]], good_c)           # wrong width
    with pytest.raises(ValueError):
        mod.load_tenant(0, [good_m[0][:2], good_m[1], good_m[2]], good_c)              # wrong K / 32
    with pytest.raises(ValueError):
        mod.load_tenant(0, [good_m[0].long(), good_m[1], good_m[2]], good_c)           # wrong dtype
    with pytest.raises(ValueError):
        mod.load_tenant(0, good_m, [good_c[0], good_c[1], torch.ones(2)])              # not a scalar
    with pytest.raises(BitDeltaHipError):
        mod.load_tenant(0, good_m, good_c)                                             # all in order, but on the CPU: no fallback
    for b, a in zip(before, (mod.mask, mod.mask_packed, mod.alpha)):
        assert torch.equal(a, b)


def test_load_decode_masks_refuses_cpu_tensors():
    from bitdelta_amd.binary_gemm_kernel import load_decode_masks, pack_decode_masks
    m = torch.zeros(2, 4, 16, dtype=torch.int32)
    with pytest.raises(BitDeltaHipError):
        load_decode_masks(m[0], mask=m[1], packed=pack_decode_masks(m), slot=1)


def _cpu_decoder(shared):
    """a two-layer decoder on the CPU: construction is torch plumbing, only launches need the device"""
    from bitdelta_amd.serving_loop import FusedDeltaLinear, TenantDecoder
    import torch.nn as nn
    cfg, T = (128, 256, 2, 1, 1, 64), 3
    hid, inter, nl, heads, kvh, vocab = cfg
    dec = TenantDecoder(cfg, T, "cpu", torch.float16, max_len=80)
    gen = torch.Generator().manual_seed(2)

    def fused(*widths, inter8=False, K=hid):
        ws, ms, cs = _parts(widths, K, T, gen)
        return FusedDeltaLinear(ws, ms, cs, interleave8=inter8)

    def rows(*shape):
        r = torch.randn(1 if shared else T, *shape, generator=gen).half()
        return r.expand(T, *shape) if shared else r

    for _ in range(nl):
        layer = nn.Module()
        layer.qkv, layer.o = fused(hid, hid, hid), fused(hid)
        layer.gate_up, layer.down = fused(inter, inter, inter8=True), fused(hid, K=inter)
        layer.norm1, layer.norm2 = rows(hid), rows(hid)
        dec.layers.append(layer)
    dec.embed, dec.final_norm, dec.lm_head = rows(vocab, hid), rows(hid), rows(vocab, hid)
    return dec


def _clone_state(s):
    cl = lambda x: [v.clone() for v in x]
    return {"layers": [{k: (v.clone() if torch.is_tensor(v) else (cl(v[0]), cl(v[1]))) for k, v in d.items()} for d in s["layers"]],
            "embed": s["embed"].clone(), "final_norm": s["final_norm"].clone(), "lm_head": s["lm_head"].clone()}


def test_decoder_refusals_come_before_any_launch():
    dec = _cpu_decoder(shared=False)
    state = _clone_state(dec.tenant_state(1))
    snap = _clone_state(dec.tenant_state(0))
    with pytest.raises(IndexError):
        dec.load_tenant(3, state)
    bad = _clone_state(state)
    bad["layers"][1]["down"] = (bad["layers"][1]["down"][0], [torch.ones(2)])
    with pytest.raises(ValueError):
        dec.load_tenant(0, bad)                                    # the LAST Linear is wrong: nothing before it may have been written
    bad = _clone_state(state)
    bad["lm_head"] = bad["lm_head"][:, :64]
    with pytest.raises(ValueError):
        dec.load_tenant(0, bad)
    bad = _clone_state(state)
    bad["layers"][0]["norm1"] = bad["layers"][0]["norm1"].float()
    with pytest.raises(ValueError):
        dec.load_tenant(0, bad)
    bad = _clone_state(state)
    bad["layers"].pop()
    with pytest.raises(ValueError):
        dec.load_tenant(0, bad)
    with pytest.raises(BitDeltaHipError):
        dec.load_tenant(0, state)                                  # a good state on the CPU: no fallback
    now = dec.tenant_state(0)
    for a, b in zip(now["layers"], snap["layers"]):
        assert torch.equal(a["norm1"], b["norm1"]) and all(torch.equal(x, y) for x, y in zip(a["qkv"][0], b["qkv"][0]))
    assert torch.equal(now["embed"], snap["embed"])


def test_decoder_refuses_expanded_per_tenant_tensors():
    dec = _cpu_decoder(shared=True)
    state = _clone_state(dec.tenant_state(1))
    with pytest.raises(ValueError, match="expanded"):
        dec.load_tenant(0, state)
