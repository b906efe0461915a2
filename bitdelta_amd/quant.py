"""8-bit base weights for the decode path: the LLM.int8 vector-wise format BitDelta evaluates its deltas on.

The reference only *reads* this format: bitdelta/misc.py:70-126 (`dequantize_model`) turns a bitsandbytes 8-bit Linear back into an fp16
one with  (CB * SCB.unsqueeze(1)) / 127  (misc.py:72-73; CB int8 [N, K], SCB = per-output-row absmax) and runs the fp16 path.  Here the
same pair (CB, SCB) is what the streaming decode kernel consumes directly (bd_binary_linear_decode_w8): CB stays one byte per weight in
HBM, in the kernel's tile-major order, and SCB / 127 multiplies the finished base sum.

Registration-time helpers (torch ops on the weight's device, run once per base); nothing here is on the hot path.
"""
import torch


def quantize_base_int8(weight):
    """W [N, K] (fp16 / bf16 / fp32) -> (CB int8 [N, K], SCB fp32 [N]).

    SCB[n] = max_k |W[n, k]| (fp32);  CB[n, k] = clamp(round_half_even(W[n, k] * 127 / SCB[n]), -127, 127).
    An all-zero row gives CB = 0, SCB = 0.  |W - CB * SCB / 127| <= SCB / 254 per element (half a quantisation step)."""
    assert weight.dim() == 2 and weight.is_floating_point()
    w = weight.float()
    scb = w.abs().amax(dim=1)
    step = torch.where(scb > 0, scb, torch.ones_like(scb))           # (an all-zero row: any divisor, the quotient is 0)
    cb = torch.round(w * 127.0 / step[:, None]).clamp_(-127, 127).to(torch.int8)      # torch.round: half to even
    return cb.contiguous(), scb.contiguous()


def dequantize_base_int8(cb, scb, dtype=torch.float16):
    """The reference's dequantisation (bitdelta/misc.py:72-73), restated: fp32 product CB * SCB[:, None], divided by 127, rounded to fp16
    as the reference's `.half()` does, then cast to `dtype` (fp16: nothing more; bf16: a second rounding, what `model.to(bfloat16)` after
    `dequantize_model` would give)."""
    assert cb.dtype == torch.int8 and cb.dim() == 2 and scb.dtype == torch.float32 and scb.shape == (cb.shape[0],)
    return ((cb * scb[:, None]) / 127).half().to(dtype)


def weight_scale(scb):
    """wscale[n] = SCB[n] / 127 in fp32: the per-output-row factor of bd_binary_linear_decode_w8"""
    assert scb.dtype == torch.float32
    return (scb / 127).contiguous()


def tile_weight_int8(cb):
    """Decode copy of CB [N, K] (N % 16 == 0, K % 128 == 0) in the streaming kernel's int8 TILE-MAJOR order (csrc/bd_gemv_stream.h, WT = 2)
    [N/16][K/128][2 loads h][16 rows c][4 groups g][2 steps j][8]  with  W8'[tile][it][h][c][g][j][e] = CB[16 tile + c][128 it + 32 (2 h + j) + 8 g + e]:
    one (16-column tile, 128-k iteration) stage is ONE contiguous 2-KiB block read as two 1-KiB runs, and a lane's 16 bytes of run h are its
    k-octets of MFMA steps 2 h and 2 h + 1.  A permutation of the bytes; returned with shape [N, K] (a flat reinterpretation) so it can stand in
    for `weight` in binary_linear_decode(..., weight_scale=...)."""
    assert cb.dtype == torch.int8 and cb.dim() == 2
    N, K = cb.shape
    assert N % 16 == 0 and K % 128 == 0
    #            tile     c   it        h  j  g  e
    v = cb.reshape(N // 16, 16, K // 128, 2, 2, 4, 8)
    return v.permute(0, 2, 3, 1, 5, 4, 6).contiguous().view(N, K)
