"""binary_linear(tile-major nibbles, group_params=) -- bd_binary_linear_q4 -- against the fp64 evaluation of
    Y[b,m,n] = sum_k X[b,m,k] Wdq[n,k]  +  alpha[b,g(n)] * sum_k X[b,m,k] S_b[k,n]  [+ residual],   Wdq = quant.dequantize_base_gptq4(...)
rounded once: within_one_ulp with >= 0.99 bit-equal (fp32 output: rel <= 1e-5), as test_gpu_w8_prefill.py; outputs sit in poisoned margins.
Cases: K one iteration / ring wrap / odd count, and K = 512 at group 256 (the group changes mid-loop); N = 16, 48 and 144 (3 and 9 tiles:
the two-tile plan's last pair is half empty); M in every plan (2, 16 | 17 | 64 | 129: a ragged second row tile); col_margin 66 leaves rows
4-byte aligned (the element-wise store path).  Scales span four decades, z = 1 and z = 16 are both present, one column has scale 0."""
import pytest
import torch
from canary import CanaryOut
from test_gpu_parity import within_one_ulp
from test_gpu_q4_decode import random_checkpoint

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
#        dtype B  M    N    K   GS  G  bcast  resid  f32    xpad col_margin
CASES = [(F16, 1, 2, 16, 128, 128, 1, False, False, False, 0, 64),
         (BF16, 3, 16, 48, 256, 128, 2, True, True, False, 0, 64),
         (F16, 3, 17, 144, 384, 128, 2, False, True, False, 0, 64),
         (BF16, 1, 64, 144, 512, 256, 1, False, False, False, 64, 64),
         (F16, 3, 129, 144, 384, 128, 2, True, False, False, 0, 64),
         (BF16, 1, 129, 48, 128, 128, 1, False, True, False, 0, 66),
         (F16, 2, 129, 16, 512, 256, 1, False, True, False, 64, 64),
         (F16, 1, 17, 48, 256, 256, 1, False, False, True, 0, 64),
         (BF16, 3, 64, 16, 384, 128, 1, False, True, True, 0, 66)]


@pytest.mark.parametrize("dtype,B,M,N,K,GS,G,bcast,resid,f32,xpad,cm", CASES,
                         ids=["%s-B%d-M%d-N%d-K%d-g%d" % (str(c[0])[6:], *c[1:6]) for c in CASES])
def test_q4_prefill_linear_matches_fp64(dtype, B, M, N, K, GS, G, bcast, resid, f32, xpad, cm):
    from bitdelta_amd.binary_gemm_kernel import binary_linear
    from bitdelta_amd.quant import dequantize_base_gptq4, pack_gptq4_params, tile_weight_gptq4
    g = torch.Generator(device="cuda").manual_seed(1000 * M + N + K + B)
    xbuf = (torch.randn(B, M, K + xpad, device="cuda", generator=g) * 1.5).to(dtype)
    x = xbuf[..., :K]
    qw, qz, _ = random_checkpoint(N, K, GS, g)
    qz[0, 0] = (qz[0, 0] & ~0xFF) | 0x0F                                                  # column 0: z = 16, column 1: z = 1
    sc = (10.0 ** (-5 + 4 * torch.rand(K // GS, N, device="cuda", generator=g))).half()   # four decades: a misplaced group or column shows
    sc[:, N // 2] = 0.0                                                                   # an all-zero column
    wdq = dequantize_base_gptq4(qw, qz, sc, dtype).double()
    mask = torch.randint(-2**31, 2**31 - 1, (1 if bcast else B, K // 32, N), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)
    alpha = torch.rand(B, G, device="cuda", generator=g) * 1e-3 + 2e-4
    odt = torch.float32 if f32 else dtype
    res = torch.randn(B, M, N, device="cuda", generator=g).to(odt)
    bits = (mask.long()[:, :, None, :] >> torch.arange(32, device="cuda")[None, None, :, None]) & 1      # [., K/32, 32, N]
    S = (bits.reshape(mask.shape[0], K, N) * 2 - 1).double().expand(B, K, N)
    want = x.double() @ wdq.T + alpha.double().repeat_interleave(N // G, 1)[:, None, :] * (x.double() @ S)
    if resid:
        want = want + res.double()
    out = CanaryOut(B, M, N, odt, row_margin=8, col_margin=cm)
    if resid:
        out.view.copy_(res)
    binary_linear(x, tile_weight_gptq4(qw), mask, alpha, groups=G, group_params=pack_gptq4_params(qz, sc), group_size=GS, out_dtype=odt,
                  **({"residual": out.view} if resid else {"out": out.view}))
    got = out.result()
    assert out.untouched_outside(), "a store outside the [B, M, N] output"
    if f32:
        rel = ((got.double() - want).norm() / want.norm()).item()
        assert rel <= 1e-5, rel
    else:
        ok, frac = within_one_ulp(got, want.to(dtype), K)
        assert ok and frac >= 0.99, frac
