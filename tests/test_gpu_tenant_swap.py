"""Loading a new fine-tune into ONE tenant slot of a live decoder (GPU): the sign-load kernel against pack_decode_masks, its column map against a
freshly built FusedDeltaLinear, FusedDeltaLinear.load_tenant on the three base forms, and the decoder / session operations against a decoder
built fresh over the new tenant set.  Integer work and identical launches on identical buffers: every comparison is torch.equal."""
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from canary import POISON, CanaryOut  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = POISON * 0x01010101
T_PADS = (1, 2, 4, 6, 8, 12, 16)


def _words(gen, *shape):
    """random int32 words with the two values a signed shuffle gets wrong first planted in every tensor"""
    w = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=gen, dtype=torch.int64).to(torch.int32)
    flat = w.view(-1)
    flat[0], flat[-1] = -1, -2 ** 31
    if flat.numel() > 5:
        flat[3], flat[5] = -2 ** 31, -1
    return w


def _poison_padding(packed, T, N):
    """sentinel into everything of a packed tensor that belongs to no (tenant, column): the padding slots and the columns past N"""
    packed[..., T:] = SENT
    tiles = packed.shape[0]
    col = (torch.arange(tiles, device=packed.device)[:, None] * 16 + torch.arange(16, device=packed.device)[None, :]) >= N      # [tile, c]
    packed.permute(0, 3, 1, 2, 4)[col] = SENT
    return packed


# ------------------------------------------------------------------------------------------------ 1. the kernel against pack_decode_masks
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6, 8, 11, 12, 16])
@pytest.mark.parametrize("KW,N", [(4, 16), (5, 40), (8, 48), (3, 20), (64, 528), (5, 18)])
def test_kernel_matches_pack_decode_masks(KW, N, T):
    from bitdelta_amd.binary_gemm_kernel import load_decode_masks, pack_decode_masks
    gen = torch.Generator().manual_seed(1000 * KW + N + T)
    old = _words(gen, T, KW, N).to(DEV)
    packed_old = pack_decode_masks(old)
    t_pad = packed_old.shape[-1]
    assert t_pad == next(v for v in T_PADS if v >= T)
    margin = 4096
    for t in sorted({0, T // 2, T - 1}):
        for ld_extra in (0, 7):
            new = _words(gen, KW, N).to(DEV)
            src = new
            if ld_extra:                                   # a source whose row stride exceeds N (and is no multiple of 4: unaligned rows)
                wide = torch.full((KW, N + ld_extra), SENT, dtype=torch.int32, device=DEV)
                wide[:, :N] = new
                src = wide[:, :N]
            want_set = old.clone()
            want_set[t] = new
            # destination inside a sentinel-filled buffer; the padding slots and columns carry the sentinel too
            buf = torch.full((margin + packed_old.numel() + margin,), SENT, dtype=torch.int32, device=DEV)
            dst = buf[margin:margin + packed_old.numel()].view(packed_old.shape)
            dst.copy_(packed_old)
            _poison_padding(dst, T, N)
            want = buf.clone()
            want[margin:margin + packed_old.numel()].view(packed_old.shape).copy_(_poison_padding(pack_decode_masks(want_set), T, N))
            plane = CanaryOut(1, KW, N, torch.int32, device=DEV, row_margin=4, col_margin=8)
            plane.view.copy_(old[t:t + 1])
            load_decode_masks(src, mask=plane.view[0], packed=dst, slot=t)
            assert torch.equal(buf, want), (t, ld_extra)            # slot t as pack_decode_masks has it; margins, other slots, padding unchanged
            assert torch.equal(plane.view[0], new) and plane.untouched_outside()
            if ld_extra:
                assert bool((wide[:, N:] == SENT).all())
    # either destination alone
    new = _words(gen, KW, N).to(DEV)
    only_packed, only_mask = packed_old.clone(), old[0].clone()
    load_decode_masks(new, packed=only_packed, slot=T - 1)
    load_decode_masks(new, mask=only_mask)
    want_set = old.clone()
    want_set[T - 1] = new
    assert torch.equal(only_packed, pack_decode_masks(want_set)) and torch.equal(only_mask, new)


# ------------------------------------------------------------------------------------------------ 2. the column map
def _linear_parts(gen, widths, K, T):
    ws = [(torch.randn(n, K, generator=gen) * 0.02).half().to(DEV) for n in widths]
    ms = [_words(gen, T, K // 32, n).to(DEV) for n in widths]
    cs = [(torch.rand(T, generator=gen) * 1e-3 + 1e-4).to(DEV) for _ in widths]
    return ws, ms, cs


def _replaced(ms, cs, t, new_m, new_c):
    ms2, cs2 = [m.clone() for m in ms], [c.clone() for c in cs]
    for i in range(len(ms)):
        ms2[i][t] = new_m[i]
        cs2[i][t] = new_c[i]
    return ms2, cs2


@pytest.mark.parametrize("widths,inter8", [((32, 16, 16), False), ((24, 8, 8), False), ((24, 24), True), ((512, 512), True),
                                           ((6, 10), False)])         # (6, 10): a map that is not 4-aligned -> the one-column-at-a-time stores
def test_column_map_matches_a_fresh_module(widths, inter8):
    from bitdelta_amd.binary_gemm_kernel import load_decode_masks
    from bitdelta_amd.serving_loop import FusedDeltaLinear, fused_columns
    gen = torch.Generator().manual_seed(sum(widths) + inter8)
    T, K, t = 3, 160, 1
    ws, ms, cs = _linear_parts(gen, widths, K, T)
    mod = FusedDeltaLinear(ws, ms, cs, interleave8=inter8)
    new_m = [_words(gen, K // 32, n).to(DEV) for n in widths]
    ms2, cs2 = _replaced(ms, cs, t, new_m, [c[t] for c in cs])
    fresh = FusedDeltaLinear(ws, ms2, cs2, interleave8=inter8)
    assert mod.mask_packed is not None and not torch.equal(mod.mask_packed, fresh.mask_packed)
    for m, (off, blk, stride) in zip(new_m, fused_columns(widths, inter8)[1]):
        load_decode_masks(m, mask=mod.mask[t], packed=mod.mask_packed, slot=t, col_off=off, col_blk=blk, col_stride=stride)
    assert torch.equal(mod.mask, fresh.mask) and torch.equal(mod.mask_packed, fresh.mask_packed)


# ------------------------------------------------------------------------------------------------ 3. FusedDeltaLinear.load_tenant
_BUFFERS = ("weight", "mask", "alpha", "alpha_pair", "mask_packed", "weight_tiled", "wscale", "group_params")


@pytest.mark.parametrize("widths,inter8", [((256, 128, 128), False), ((256, 256), True)])
@pytest.mark.parametrize("base", ["w16", "int8", "gptq4"])
def test_linear_load_tenant(base, widths, inter8):
    from bitdelta_amd.serving_loop import FusedDeltaLinear
    gen = torch.Generator().manual_seed(31 + inter8)
    T, K = 3, 256
    kw = dict(interleave8=inter8, base_int8=base == "int8", base_gptq4=base == "gptq4")
    ws, ms, cs = _linear_parts(gen, widths, K, T)
    x1 = torch.randn(T, 1, K, generator=gen).half().to(DEV)
    x32 = torch.randn(T, 32, K, generator=gen).half().to(DEV)
    mod = FusedDeltaLinear(ws, ms, cs, **kw)
    assert mod.weight.shape[0] == 512 and mod._decode_ok(x1) and not mod._decode_ok(x32)
    ptrs = {n: getattr(mod, n).data_ptr() for n in _BUFFERS if getattr(mod, n) is not None}
    for t in (0, 2, 1):
        new_m = [_words(gen, K // 32, n).to(DEV) for n in widths]
        new_c = [(torch.rand((), generator=gen) * 1e-3 + 1e-4).to(DEV) for _ in widths]
        ms, cs = _replaced(ms, cs, t, new_m, new_c)
        mod.load_tenant(t, new_m, new_c)
        fresh = FusedDeltaLinear(ws, ms, cs, **kw)
        for n in ("mask", "mask_packed", "alpha") + (("alpha_pair",) if inter8 else ()):
            assert torch.equal(getattr(mod, n), getattr(fresh, n)), n
        assert ptrs == {n: getattr(mod, n).data_ptr() for n in _BUFFERS if getattr(mod, n) is not None}
        assert torch.equal(mod(x1), fresh(x1)) and torch.equal(mod(x32), fresh(x32))
    m_t, c_t = mod.tenant_signs(1)
    assert all(torch.equal(a, b) for a, b in zip(m_t, new_m)) and all(float(a) == float(b) for a, b in zip(c_t, new_c))


def test_linear_load_tenant_without_decode_copies():
    from bitdelta_amd.serving_loop import FusedDeltaLinear
    gen = torch.Generator().manual_seed(77)
    widths, K, T = (48, 16), 128, 17                         # more than 16 tenants: no packed words to update
    ws, ms, cs = _linear_parts(gen, widths, K, T)
    for mod in (FusedDeltaLinear(ws, ms, cs), FusedDeltaLinear([w[:, :K] for w in ws], [m[:3] for m in ms], [c[:3] for c in cs], decode_copies=False)):
        assert mod.mask_packed is None
        t = mod.mask.shape[0] - 1
        new_m = [_words(gen, K // 32, n).to(DEV) for n in widths]
        mod.load_tenant(t, new_m, [0.5, 0.25])
        assert torch.equal(mod.mask[t], torch.cat(new_m, 1)) and torch.equal(mod.mask[:t], torch.cat([m[:t] for m in ms], 2))
        assert mod.alpha[t].tolist() == [0.5, 0.5, 0.5, 0.25]


# ------------------------------------------------------------------------------------------------ 4 - 6. decoder and session
_LIN = ("qkv", "o", "gate_up", "down")
_FT = {}


def _finetunes(name):
    """one base and four fine-tunes (a, b, c, d) of a small config, made with this file's own generator and binarize: (base, [state, ...]) with
    each state in the form TenantDecoder.load_tenant takes.  Norm weights are kept inside (0.6, 1.9): the hand-off scale of every set is 2."""
    if name in _FT:
        return _FT[name]
    from bitdelta_amd.diff import binarize
    from bitdelta_amd.serving_loop import MODEL_CONFIGS
    hid, inter, nl, heads, kvh, vocab = MODEL_CONFIGS[name]
    hd = hid // heads
    gen = torch.Generator(device=DEV).manual_seed(len(name))
    shapes = {"qkv": [(heads * hd, hid), (kvh * hd, hid), (kvh * hd, hid)], "o": [(hid, heads * hd)], "gate_up": [(inter, hid), (inter, hid)],
              "down": [(hid, inter)]}
    rn = lambda *s: torch.randn(*s, device=DEV, generator=gen)
    base = [{k: [(rn(*s) * 0.02).half() for s in shapes[k]] for k in _LIN} for _ in range(nl)]
    states = []
    for _ in range(4):
        layers = []
        for li in range(nl):
            d = {}
            for k in _LIN:
                mc = [binarize(w, (w.float() + rn(*w.shape) * 5e-4).half()) for w in base[li][k]]
                d[k] = ([m for m, _ in mc], [c for _, c in mc])
            d["norm1"], d["norm2"] = [(1.0 + 0.1 * rn(hid)).clamp(0.6, 1.9).half() for _ in range(2)]
            layers.append(d)
        states.append({"layers": layers, "embed": (rn(vocab, hid) * 0.02).half(), "final_norm": (1.0 + 0.1 * rn(hid)).clamp(0.6, 1.9).half(),
                       "lm_head": (rn(vocab, hid) * 0.02).half()})
    torch.cuda.synchronize()
    _FT[name] = (base, states)
    return _FT[name]


def _decoder(name, base, states):
    from bitdelta_amd.serving_loop import MODEL_CONFIGS, FusedDeltaLinear, TenantDecoder
    dec = TenantDecoder(MODEL_CONFIGS[name], len(states), DEV, torch.float16, max_len=96)
    for li, bl in enumerate(base):
        layer = nn.Module()
        for k in _LIN:
            n_proj = len(bl[k])
            masks = [torch.stack([s["layers"][li][k][0][i] for s in states], 0) for i in range(n_proj)]
            coeffs = [torch.stack([s["layers"][li][k][1][i].reshape(()) for s in states], 0) for i in range(n_proj)]
            setattr(layer, k, FusedDeltaLinear(bl[k], masks, coeffs, interleave8=(k == "gate_up")))
        layer.norm1 = torch.stack([s["layers"][li]["norm1"] for s in states], 0)
        layer.norm2 = torch.stack([s["layers"][li]["norm2"] for s in states], 0)
        dec.layers.append(layer)
    for k in ("embed", "final_norm", "lm_head"):
        setattr(dec, k, torch.stack([s[k] for s in states], 0))
    return dec


def _assert_same_tenant_buffers(X, Y):
    for lx, ly in zip(X.layers, Y.layers):
        for k in _LIN:
            for n in ("mask", "mask_packed", "alpha", "alpha_pair"):
                a, b = getattr(getattr(lx, k), n), getattr(getattr(ly, k), n)
                assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), (k, n)
        assert torch.equal(lx.norm1, ly.norm1) and torch.equal(lx.norm2, ly.norm2)
    for k in ("embed", "final_norm", "lm_head"):
        assert torch.equal(getattr(X, k), getattr(Y, k)), k


def _next_logits(dec):
    """the logits of the step AFTER the last generate(): one eager decode forward on the request state generate left behind"""
    st = next(reversed(dec._static.values()))["st"]
    cache = st["cache"]
    cache["valid"].index_fill_(1, st["pos"], True)
    return dec.forward(st["tok"], st["pos"], cache, cache["valid"][:, None, None, :]).clone()


PROMPTS = [[5, 17, 300, 41], [9, 2, 77, 130, 6, 250, 12], [400, 3, 3, 19, 88]]


@pytest.mark.parametrize("name", ["tiny128", "tiny2048"])
def test_decoder_load_tenant_equals_a_fresh_decoder(name):
    base, (a, b, c, d) = _finetunes(name)
    X, Y = _decoder(name, base, [a, b, c]), _decoder(name, base, [d, b, c])
    Z = _decoder(name, base, [a, b, c])
    tok_a, _ = X.generate(PROMPTS, max_new_tokens=6)          # the graph is captured (and the hand-off norms cached) with fine-tune a in slot 0
    graphs = [s["graph"] for s in X._static.values()]
    assert graphs[0] is not None
    handoff = name == "tiny2048"
    assert (getattr(X.layers[0], "_hn_norm2", None) is not None) == handoff and (getattr(X.layers[1], "_hn_norm1", None) is not None) == handoff
    tok_y, n_y = Y.generate(PROMPTS, max_new_tokens=6)
    logits_y = _next_logits(Y)
    assert not torch.equal(tok_a[0], tok_y[0]) and torch.equal(tok_a[1:], tok_y[1:])      # the fine-tunes differ; tenants are independent
    assert X.load_tenant(0, d) is False                       # every set's hand-off scale is 2: nothing captured moves
    assert [s["graph"] for s in X._static.values()] == graphs
    _assert_same_tenant_buffers(X, Y)
    tok_x, n_x = X.generate(PROMPTS, max_new_tokens=6)
    assert n_x == n_y and torch.equal(tok_x, tok_y)
    assert torch.equal(_next_logits(X), logits_y)
    if handoff:
        for lx, ly in zip(X.layers, Y.layers):
            for w in ("norm1", "norm2"):
                hx, hy = getattr(lx, "_hn_" + w, None), getattr(ly, "_hn_" + w, None)
                assert (hx is None) == (hy is None) and (hx is None or (hx[1] == hy[1] == 2.0 and torch.equal(hx[0], hy[0])))
    # round trip: Y's slot 0 into another decoder's slot 0
    Z.generate(PROMPTS, max_new_tokens=6)
    Z.load_tenant(0, Y.tenant_state(0))
    _assert_same_tenant_buffers(Z, Y)
    tok_z, _ = Z.generate(PROMPTS, max_new_tokens=6)
    assert torch.equal(tok_z, tok_y) and torch.equal(_next_logits(Z), logits_y)


def _tokens(sess, ts):
    return [sess.result(t)[0] for t in ts]


def test_session_load_while_others_generate():
    name = "tiny128"
    base, (a, b, c, d) = _finetunes(name)
    X, U, Y = _decoder(name, base, [a, b, c]), _decoder(name, base, [a, b, c]), _decoder(name, base, [d, b, c])
    sx, su, sy = X.session(), U.session(), Y.session()
    for s in (sx, su):
        s.submit(1, PROMPTS[1], max_new_tokens=12)
        s.submit(2, PROMPTS[2], max_new_tokens=9)
        s.step(3)
    assert sx.active() == [False, True, True]
    graphs = dict(sx._graphs)
    assert len(graphs) == 1
    with pytest.raises(RuntimeError):
        sx.load_tenant(1, d)                                   # tenant 1 is generating
    with pytest.raises(IndexError):
        sx.load_tenant(3, d)
    assert sx.load_tenant(0, d) is False
    assert sx._graphs == graphs                                # no re-capture: the same graph object goes on replaying
    sx.submit(0, PROMPTS[0], max_new_tokens=8)
    sx.run()
    su.run()
    assert sx._graphs == graphs
    sy.submit(0, PROMPTS[0], max_new_tokens=8)
    sy.run()
    for got, want in zip(_tokens(sx, (1, 2)), _tokens(su, (1, 2))):
        assert torch.equal(got, want)                          # exactly the tokens of the untouched decoder
    assert len(sx.result(1)[0]) == 12 and len(sx.result(2)[0]) == 9
    assert torch.equal(sx.result(0)[0], sy.result(0)[0]) and len(sx.result(0)[0]) == 8
    # a finished tenant's slot is cleared by the load
    sx.load_tenant(2, a)
    assert int(sx.n[2]) == 0 and int(sx.done[2]) == 0 and not bool(sx.cache["valid"][2].any()) and not bool(sx.out[2].any())
    assert int(sx.n[1]) == 12 and bool(sx.cache["valid"][1].any())


def test_handoff_scale_change_drops_captured_graphs():
    name = "tiny2048"
    base, (a, b, c, d) = _finetunes(name)
    big = {**d, "layers": [dict(l) for l in d["layers"]]}
    for l in big["layers"]:
        for w in ("norm1", "norm2"):
            l[w] = l[w].clone()
            l[w][5] = 3.0                                      # above the current power of two (2): s becomes 4
    X, Y = _decoder(name, base, [a, b, c]), _decoder(name, base, [big, b, c])
    assert X.norm_handoff
    X.generate(PROMPTS, max_new_tokens=5)
    sx = X.session()
    sx.submit_all(PROMPTS, max_new_tokens=4)
    sx.run()
    assert X.layers[1]._hn_norm1[1] == 2.0 and X.layers[0]._hn_norm2[1] == 2.0
    assert all(s["graph"] is not None for s in X._static.values()) and len(sx._graphs) == 1
    assert sx.load_tenant(0, big) is True
    assert all(s["graph"] is None for s in X._static.values()) and len(sx._graphs) == 0       # they baked s = 2
    assert X.layers[1]._hn_norm1[1] == 4.0 and X.layers[0]._hn_norm2[1] == 4.0
    _assert_same_tenant_buffers(X, Y)
    tok_x, _ = X.generate(PROMPTS, max_new_tokens=5)
    tok_y, _ = Y.generate(PROMPTS, max_new_tokens=5)
    assert torch.equal(tok_x, tok_y)                           # all three tenants
    assert all(s["graph"] is not None for s in X._static.values())                            # ... on a graph made again
    sy = Y.session()
    for s in (sx, sy):
        s.submit_all(PROMPTS, max_new_tokens=5)
        s.run()
    assert len(sx._graphs) == 1
    for t in range(3):
        assert torch.equal(sx.result(t)[0], sy.result(t)[0])
    for lx, ly in zip(X.layers, Y.layers):
        for w in ("norm1", "norm2"):
            hx, hy = getattr(lx, "_hn_" + w, None), getattr(ly, "_hn_" + w, None)
            assert (hx is None) == (hy is None) and (hx is None or (hx[1] == hy[1] and torch.equal(hx[0], hy[0])))
    # back below the power of two: s returns to 2, which is again a rebuild
    assert X.load_tenant(0, a) is True and X.layers[1]._hn_norm1[1] == 2.0
