"""Quantised base weights for the decode path: the two formats BitDelta evaluates its deltas on (LLM.int8 vector-wise, 4-bit GPTQ).

8 bits:

The reference only *reads* this format: bitdelta/misc.py:70-126 (`dequantize_model`) turns a bitsandbytes 8-bit Linear back into an fp16
one with  (CB * SCB.unsqueeze(1)) / 127  (misc.py:72-73; CB int8 [N, K], SCB = per-output-row absmax) and runs the fp16 path.  Here the
same pair (CB, SCB) is what the streaming decode kernel consumes directly (bd_binary_linear_decode_w8): CB stays one byte per weight in
HBM, in the kernel's tile-major order, and SCB / 127 multiplies the finished base sum.

4 bits: the reference's `dequantize_4bit` (bitdelta/misc.py:76-105) reads a GPTQ checkpoint layer -- qweight int32 [K/8, N], qzeros int32
[K/G, N/8], scales fp16 [K/G, N], no g_idx -- as  W[n, k] = fp16((q[k, n] - z[k // G, n]) * scales[k // G, n])  with
q[k, n] = (qweight[k // 8, n] >> 4 (k % 8)) & 15  and  z[g, n] = ((qzeros[g, n // 8] >> 4 (n % 8)) & 15) + 1.  Here the nibbles stay half a
byte per weight in HBM, in the kernel's tile-major order, and the streaming decode kernel rebuilds exactly that W in registers
(bd_binary_linear_decode_q4).

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


# ------------------------------------------------------------------------------------------------------------------ 4-bit GPTQ
def _unpack_nibbles(t, dim):
    """int32 [..] -> the 8 nibbles of every dword spread along `dim` (nibble i = bits 4 i .. 4 i + 3), int32 values 0 .. 15"""
    sh = torch.arange(8, device=t.device, dtype=torch.int32) * 4
    if dim == 0:
        return ((t[:, None, :] >> sh[None, :, None]) & 15).reshape(t.shape[0] * 8, t.shape[1])
    return ((t[:, :, None] >> sh[None, None, :]) & 15).reshape(t.shape[0], t.shape[1] * 8)


def _pack_nibbles(v, dim):
    """the inverse: values 0 .. 15, 8 consecutive ones along `dim` -> one int32 (nibble i = element i; bit 31 wraps into the sign)"""
    v = v.to(torch.int64)
    sh = torch.arange(8, device=v.device, dtype=torch.int64) * 4
    if dim == 0:
        u = (v.reshape(v.shape[0] // 8, 8, v.shape[1]) << sh[None, :, None]).sum(1)
    else:
        u = (v.reshape(v.shape[0], v.shape[1] // 8, 8) << sh[None, None, :]).sum(2)
    return torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32)


def _check_gptq4(qweight, qzeros, scales):
    assert qweight.dtype == torch.int32 and qzeros.dtype == torch.int32 and scales.dtype == torch.float16
    assert qweight.dim() == 2 and qzeros.dim() == 2 and scales.dim() == 2
    K, N = qweight.shape[0] * 8, qweight.shape[1]
    ng = scales.shape[0]
    assert N % 8 == 0 and scales.shape == (ng, N) and qzeros.shape == (ng, N // 8) and ng >= 1 and K % ng == 0
    return N, K, K // ng


def dequantize_base_gptq4(qweight, qzeros, scales, dtype=torch.float16):
    """The reference's dequantisation (bitdelta/misc.py:76-105), restated: q - z is an exact small integer (z = stored nibble + 1, so 1 .. 16 and
    q - z in [-16, 14]), ONE fp16 multiply by the group's scale (one rounding), transposed to [N, K]; then cast to `dtype` (fp16: nothing more;
    bf16: a second rounding, what dequantize_model's `.to(submodule.weight.dtype)` gives on a bf16 model).  Pinned bit for bit by
    tests/golden/gptq4.pt, which the reference itself wrote."""
    N, K, G = _check_gptq4(qweight, qzeros, scales)
    q = _unpack_nibbles(qweight, 0)                                   # [K, N]
    z = _unpack_nibbles(qzeros, 1) + 1                                # [K/G, N]
    d = (q - z.repeat_interleave(G, dim=0)).to(torch.float16)         # exact
    w = d * scales.repeat_interleave(G, dim=0)                        # the one fp16 multiply
    return w.T.contiguous().to(dtype)


def quantize_base_gptq4(weight, group_size=128):
    """W [N, K] (fp16 / bf16 / fp32) -> (qweight int32 [K/8, N], qzeros int32 [K/G, N/8], scales fp16 [K/G, N]) in the format above:
    round-to-nearest, asymmetric, one (scale, zero) per (group of `group_size` consecutive k, output column n).

    Per group, with lo = min(min W, 0) <= 0 <= hi = max(max W, 0) (zero is always representable: z is an integer):
      z  = clamp(round(-15 lo / (hi - lo)), 1, 15), and 14 instead of 15 when hi > 0       -- the zero point of the ideal 15-step grid, kept off
           the ends that would leave one side no room; stored as the nibble z - 1 (the reference adds the 1 back), so z is in 1 .. 16;
      s  = the smallest fp16 number >= max(-lo / z, hi / (15 - z), 2^-14)                   -- rounded UP, never to nearest: then
           (0 - z) s <= lo and (15 - z) s >= hi hold for the STORED scale -- checked directly: z s and (15 - z) s are exact in fp32 (5 x 11 significand bits), and a scale whose fp32
           quotient was rounded below the true one (possible for fp32 weights) is bumped one more fp16 step -- i.e. every element of the group
           lies inside [(0 - z) s, (15 - z) s]; the floor 2^-14 keeps an all-zero / all-equal-to-zero group off a division by zero and the
           scale a normal fp16 number;
      q  = clamp(round(W / s) + z, 0, 15)                                                   -- the clamp never moves a value: W / s is inside
           [-z, 15 - z], integer ends, and fp32 rounding is monotonic.
    Error bound per element, against the fp16 value the reference dequantises to:
      |W - fp16((q - z) s)|  <=  s / 2  +  2^-24 |W|  +  2^-7 s
    half a step of the stored scale; the fp32 rounding of the quotient W / s in front of round() (relative 2^-24); and the fp16 rounding of the
    product, relative 2^-11 of |(q - z) s| <= 16 s.  (Products below 2^-14 are exact: s >= 2^-14 is a multiple of 2^-24 and q - z an integer.)
    tests/test_q4_host.py asserts it.  This quantiser never emits z = 16 (it needs lo < -15 s); a checkpoint may."""
    assert weight.dim() == 2 and weight.is_floating_point()
    N, K = weight.shape
    G = int(group_size)
    assert G >= 8 and G % 8 == 0 and K % G == 0 and N % 8 == 0
    w = weight.float().T.reshape(K // G, G, N)                        # [groups, G, N]
    zero = torch.zeros((), device=w.device)
    lo, hi = torch.minimum(w.amin(1), zero), torch.maximum(w.amax(1), zero)
    span = hi - lo
    z = torch.where(span > 0, torch.round(-15 * lo / torch.where(span > 0, span, torch.ones_like(span))), torch.ones_like(span)).clamp_(1, 15)
    z = torch.where((hi > 0) & (z > 14), torch.full_like(z, 14), z)
    want = torch.maximum(-lo / z, hi / (15 - z).clamp_min(1)).clamp_min(2.0 ** -14)
    s16 = want.to(torch.float16)
    up = torch.full_like(s16, float("inf"))
    s16 = torch.where(s16.float() < want, torch.nextafter(s16, up), s16)                                        # round up, never to nearest
    # `want` is itself a rounded fp32 quotient: compare the exact products with the group's ends and take one more step where they fall short
    short = (z * s16.float() < -lo) | ((15 - z) * s16.float() < hi)
    s16 = torch.where(short, torch.nextafter(s16, up), s16)
    assert bool(torch.isfinite(s16).all()), "a group's range does not fit fp16"
    s = s16.float()
    q = (torch.round(w / s[:, None, :]) + z[:, None, :]).clamp_(0, 15)
    qweight = _pack_nibbles(q.reshape(K, N), 0)
    qzeros = _pack_nibbles(z - 1, 1)
    return qweight.contiguous(), qzeros.contiguous(), s16.contiguous()


# stored nibble position p of a decode-copy dword holds element e = 2 (p % 4) + p / 4 of the k-octet (see tile_weight_gptq4)
_Q4_ELEM_OF_NIBBLE = (0, 2, 4, 6, 1, 3, 5, 7)


def tile_weight_gptq4(qweight):
    """Decode copy of qweight int32 [K/8, N] (N % 16 == 0, K % 128 == 0) in the streaming kernel's 4-bit TILE-MAJOR order (csrc/bd_gemv_stream.h,
    WT = 3): dwords [N/16][K/128][16 rows c][4 groups g][4 steps s]  with  W4'[tile][it][c][g][s] = qweight[16 it + 4 s + g][16 tile + c]  -- the 8
    nibbles of k = 128 it + 32 s + 8 g + e of column 16 tile + c -- so one (16-column tile, 128-k iteration) stage is ONE contiguous 1-KiB block
    read by one 16-byte load per lane, whose four dwords are the lane's k-octets of MFMA steps 0 .. 3.  Inside a dword the nibbles are
    INTERLEAVED: stored nibble p = element e = 2 (p % 4) + p / 4 (GPTQ's own order is p = e), so that (dword >> 4 d) & 0x000f000f is the element
    pair (2 d, 2 d + 1) of the 16-bit fragment.  Returned as int32 [N, K/8] (a flat reinterpretation) so it can stand in for `weight` in
    binary_linear_decode(..., group_params=...)."""
    assert qweight.dtype == torch.int32 and qweight.dim() == 2
    K, N = qweight.shape[0] * 8, qweight.shape[1]
    assert N % 16 == 0 and K % 128 == 0
    nib = _unpack_nibbles(qweight, 0).reshape(K // 8, 8, N)           # [dword row, e, n]
    nib = nib[:, list(_Q4_ELEM_OF_NIBBLE), :]                         # [dword row, p, n]
    dw = _pack_nibbles(nib.reshape(K, N), 0)                          # [K/8, N], nibble p = element e(p)
    #              it      s  g   tile    c
    v = dw.reshape(K // 128, 4, 4, N // 16, 16)
    return v.permute(3, 0, 4, 2, 1).contiguous().view(N, K // 8)


def pack_gptq4_params(qzeros, scales):
    """Group parameters in the form the kernel reads: int32 [N/16][K/G][16 rows c], one dword per (tile, group, column) -- bits 0 .. 15 the fp16
    scale of column 16 tile + c in that group, bits 16 .. 31 the fp16 number 1024 + z = 0x6400 + z (z = stored nibble + 1 = 1 .. 16; ulp 1 there,
    so the kernel's (1024 + q) - (1024 + z) is q - z exactly)."""
    assert qzeros.dtype == torch.int32 and scales.dtype == torch.float16 and qzeros.dim() == 2 and scales.dim() == 2
    ng, N = scales.shape
    assert N % 16 == 0 and qzeros.shape == (ng, N // 8)
    z = _unpack_nibbles(qzeros, 1) + 1                                # [K/G, N]
    sb = scales.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    dw = sb | ((0x6400 + z) << 16)
    return dw.reshape(ng, N // 16, 16).permute(1, 0, 2).contiguous()


def cat_gptq4(parts, interleave8=False):
    """Several projections' (qweight, qzeros, scales) concatenated along N (q|k|v), or two of equal width interleaved in blocks of 8 output columns
    (gate|up: [g0..7 | u0..7 | g8..15 | ...]).  8 columns share a qzeros dword, so both are permutations of whole dwords."""
    qw, qz, sc = (torch.cat([p[i] for p in parts], dim=1) for i in range(3))
    if interleave8:
        assert len(parts) == 2 and parts[0][0].shape == parts[1][0].shape
        n = parts[0][0].shape[1]
        perm = torch.arange(2 * n, device=qw.device).reshape(2, n // 8, 8).permute(1, 0, 2).reshape(-1)
        qw, sc = qw[:, perm], sc[:, perm]
        qz = qz[:, perm[::8] // 8]
    return qw.contiguous(), qz.contiguous(), sc.contiguous()
