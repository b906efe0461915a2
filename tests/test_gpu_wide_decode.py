"""The wide decode Linear on the GPU: binary_linear_decode(layout="wide") -- 17 .. 64 tenants, ONE launch, two accumulators per group of 16
tenants (csrc/bd_gemv_wide.h) -- against the fp64 evaluation of x . W^T + alpha * (x . S) from the same 16-bit inputs; tenant isolation
inside the shared delta accumulator; FusedDeltaLinear / TenantDecoder with wide_decode=True."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_decode_forms import fp64_parts, poisoned, rel  # noqa: E402
from test_gpu_parity import within_one_ulp  # noqa: E402

pytestmark = pytest.mark.gpu


def problem(dtype, T, N, K, groups, seed=0):
    """test_gpu_decode_forms.run_matrix's input distributions"""
    g = torch.Generator(device="cuda").manual_seed(seed + 7 * K + N + T)
    x = (torch.randn(T, 1, K, device="cuda", generator=g) * 1.5).to(dtype)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(dtype)
    mask = torch.randint(-2**31, 2**31 - 1, (T, K // 32, N), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)
    alpha = torch.rand(T, groups, device="cuda", generator=g) * 1e-3 + 2e-4
    res = torch.randn(T, 1, N, device="cuda", generator=g).to(dtype)
    return x, w, mask, alpha, res


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("N,K", [(1040, 128), (528, 640)])
@pytest.mark.parametrize("T", [1, 17, 33, 64])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_wide_launch_matches_fp64(dtype, T, N, K, groups):
    from bitdelta_amd.binary_gemm_kernel import binary_linear_decode, pack_decode_masks_wide, tile_weight
    x, w, mask, alpha, res = problem(dtype, T, N, K, groups)
    wide, wt = pack_decode_masks_wide(mask), tile_weight(w)
    base, delta = fp64_parts(x.double()[:, 0][None], w, mask)
    want = base[0] + alpha.double()[:, torch.arange(N, device="cuda") // (N // groups)] * delta[0]        # [T, N]
    run = lambda **kw: binary_linear_decode(x, wt, wide, alpha, layout="wide", weight_tiled=True, groups=groups, **kw)[:, 0]
    got = {"plain": (run(out=poisoned((T, 1, N), dtype)), want),
           "residual": (run(residual=res.clone()), res.double()[:, 0] + want),
           "f32": (run(out_dtype=torch.float32, out=poisoned((T, 1, N), torch.float32)), want)}
    for kind, (y, ref) in got.items():
        ok, frac = within_one_ulp(y.to(dtype), ref.to(dtype), K)
        print(f"{kind}: bit-equal {frac:.4f}, rel {rel(y, ref):.2e}")
        assert ok and frac >= 0.99, (kind, frac, rel(y, ref))
    assert got["f32"][0].dtype == torch.float32 and rel(got["f32"][0], want) <= 1e-5      # (test_gpu_decode_forms' bound for un-rounded sums)


@pytest.mark.parametrize("j", [0, 15, 16, 32])
def test_tenants_do_not_leak_into_each_other(j):
    """the 16 tenants of a group share ONE delta accumulator: changing tenant j's signs, activation row and scale moves row j alone"""
    from bitdelta_amd.binary_gemm_kernel import binary_linear_decode, pack_decode_masks_wide, tile_weight
    T, N, K = 33, 528, 640
    x, w, mask, alpha, _ = problem(torch.float16, T, N, K, 1)
    wt = tile_weight(w)
    run = lambda: binary_linear_decode(x, wt, pack_decode_masks_wide(mask), alpha, layout="wide", weight_tiled=True)
    y0 = run()
    mask[j] = ~mask[j]
    x[j] = x[j].flip(-1)
    alpha[j] *= 3
    y1 = run()
    others = [t for t in range(T) if t != j]
    assert torch.equal(y1[others], y0[others]) and not torch.equal(y1[j], y0[j])


def test_module_load_tenant_equals_a_fresh_module():
    from bitdelta_amd.serving_loop import FusedDeltaLinear
    T, K, widths = 20, 256, (64, 48)
    g = torch.Generator(device="cuda").manual_seed(5)
    ws = [(torch.randn(n, K, device="cuda", generator=g) * 0.02).half() for n in widths]
    rnd = lambda n: torch.randint(-2**31, 2**31 - 1, (T, K // 32, n), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)
    masks, coeffs = [rnd(n) for n in widths], [torch.rand(T, device="cuda", generator=g) * 1e-3 for _ in widths]
    new_m, new_c = [rnd(n)[0] for n in widths], [torch.tensor(7e-4), torch.tensor(2e-4)]
    live = FusedDeltaLinear(ws, masks, coeffs, wide_decode=True)
    assert live.mask_packed is None and live.mask_wide.shape[0] == 2 and FusedDeltaLinear(ws, masks, coeffs).mask_wide is None
    live.load_tenant(17, new_m, new_c)
    for m, c, nm, nc in zip(masks, coeffs, new_m, new_c):
        m[17], c[17] = nm, nc
    fresh = FusedDeltaLinear(ws, masks, coeffs, wide_decode=True)
    x = torch.randn(T, 1, K, device="cuda", generator=g).half()
    assert torch.equal(live.mask_wide, fresh.mask_wide) and torch.equal(live.alpha, fresh.alpha) and torch.equal(live(x), fresh(x))


def dense_logits64(bd, dec, t, ids):
    """tenant t's model as one dense fp64 network (delta merged into the weights) over an unpadded sequence: the last row's logits"""
    from bitdelta_amd.serving_loop import _rope
    _, _, _, heads, kvh, _ = dec.cfg
    L, hd = ids.shape[0], dec.hd
    merged = lambda fl: fl.weight.double() + fl.column_alpha(t).double()[:, None] * (bd.unpack(fl.mask[t]).double() * 2 - 1).T
    rms = lambda v, wn: v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + dec.eps) * wn.double()
    cos, sin = dec.cos[:L].double(), dec.sin[:L].double()
    causal = torch.ones(L, L, dtype=torch.bool, device=ids.device).tril()
    x = dec.embed[t][ids].double()
    for layer in dec.layers:
        q, k, v = layer.qkv.split(rms(x, layer.norm1[t]) @ merged(layer.qkv).T)
        q = _rope(q.view(L, heads, hd).transpose(0, 1)[None], cos, sin)[0]
        k = _rope(k.view(L, kvh, hd).transpose(0, 1)[None], cos, sin)[0].repeat_interleave(heads // kvh, 0)
        v = v.view(L, kvh, hd).transpose(0, 1).repeat_interleave(heads // kvh, 0)
        s = ((q @ k.transpose(1, 2)) / hd ** 0.5).masked_fill(~causal, float("-inf"))
        x = x + (s.softmax(-1) @ v).transpose(0, 1).reshape(L, heads * hd) @ merged(layer.o).T
        gate, up = layer.gate_up.split(rms(x, layer.norm2[t]) @ merged(layer.gate_up).T)
        x = x + (torch.nn.functional.silu(gate) * up) @ merged(layer.down).T
    return rms(x[-1], dec.final_norm[t]) @ dec.lm_head[t].double().T


@pytest.mark.parametrize("wide", [True, False])
def test_decoder_step_matches_dense_models(wide):
    """64 prompt tokens, then ONE decode step of 20 tenants (one row each: the wide launches when asked for) against 20 dense fp64 models,
    at test_gpu_serving.py's bound for logits against a dense model (3e-3 of the logits' norm)"""
    import bitdelta_amd as bd
    from bitdelta_amd.serving_loop import TenantDecoder
    T, L = 20, 64
    dec = TenantDecoder.synthetic("tiny", T, "cuda", dtype=torch.float16, seed=31, max_len=128, wide_decode=wide)
    assert (dec.layers[0].qkv.mask_wide is not None) == wide
    ids = torch.randint(1, 512, (T, L + 1), generator=torch.Generator().manual_seed(3)).cuda()
    cache = dec.new_cache()
    dec.prefill(ids[:, :L], torch.ones(T, L, dtype=torch.bool, device="cuda"), cache)
    logits = dec.prefill_chunk(ids[:, L:], L, cache)
    for t in range(T):
        assert rel(logits[t], dense_logits64(bd, dec, t, ids[t])) <= 3e-3, (t, rel(logits[t], dense_logits64(bd, dec, t, ids[t])))
