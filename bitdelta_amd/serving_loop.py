"""Multi-tenant greedy decoding without HF: SURVEY.md section 8(f) row 3, the caller of the batched 1-bit-delta Linear.

What the reference's demo does around the hot path (demo/demo_backend.py), restated for one process and one GPU:
  * one 16-bit base model + T fine-tunes, each a set of 1-bit deltas for the `*proj*` Linears plus its OWN dense embedding, norms
    and lm_head (register_diff_compress, :107-153); batch row t is tenant t (:182, :192);
  * a request is T prompts, left-padded with token 0 to max(2^ceil(log2(len)), 64) and refused beyond 1024 (:297-302);
  * prefill `model(input_ids, attention_mask)`, then greedy `argmax(logits[:, -1])` fed back one token per tenant with the KV cache
    until every tenant has produced a stop token or max_new_tokens is reached (:190-258).  Positions are the raw indices of the
    padded sequence (transformers 4.31's LlamaModel numbers positions from the cache length when none are passed).

This module is plumbing in PyTorch around the HIP ops -- attention, RoPE and norms are stock torch -- with three differences from
running the reference's modules under HF, all of them launch-count / traffic only, none numerical beyond rounding:
  * q+k+v and gate+up of a layer are ONE fused Linear each (weights and masks concatenated along the output dimension, one scale
    group per projection so every tenant keeps its own coeff per projection): 4 Linear launches per layer instead of 7;
  * the residual adds after o_proj / down_proj ride in the decode kernel's epilogue;
  * per-tenant embedding / norm / lm_head are batched (serving.DataParallelModule's mechanisms), not a Python loop;
  * the decode step is shape-static (KV cache of fixed length, a key-validity mask, the position held in a device tensor), so it
    is captured once as a hipGraph and replayed: greedy feedback happens on the device, the host only polls the stop flags.
"""
import collections.abc
import math
import operator
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from .binary_gemm_kernel import (binary_linear, binary_linear_residual_norm, binary_linear_swiglu, binary_linear_decode, decode_shape_ok, fused_norm_ok, handoff_ok,
                                 load_decode_masks, pack_decode_masks, tenant_linear, tile_weight)
from ._lib import require_gpu
from .quant import (cat_gptq4, dequantize_base_gptq4, dequantize_base_int8, pack_gptq4_params, quantize_base_gptq4, quantize_base_int8,
                    tile_weight_gptq4, tile_weight_int8, weight_scale)
from .diff import binarize
from .constraint import TokenAutomaton
from . import serving_ops as ops

MODEL_CONFIGS = {
    # name: (hidden, intermediate, layers, heads, kv_heads, vocab)
    "llama-2-7b": (4096, 11008, 32, 32, 32, 32000),
    "mistral-7b": (4096, 14336, 32, 32, 8, 32000),
    "llama-2-70b": (8192, 28672, 80, 64, 8, 32000),
    "tiny": (256, 512, 2, 4, 2, 512),
    "tiny128": (512, 1024, 2, 4, 1, 512),        # head_dim 128, 4 query heads per kv head: exercises the decode glue kernels
    "tiny4096": (4096, 4096, 2, 32, 8, 512),     # two Llama-width layers (the fused-norm launches need K >= 2048)
    "tiny2048": (2048, 2048, 2, 16, 4, 512),     # hidden % 2048 == 0: exercises the fused RMSNorm / SwiGLU launches
    "mistral-1layer": (4096, 14336, 1, 32, 8, 512),   # ONE full-width Mistral-7B layer (small vocabulary): full-size loop parity tests
}

NORM_HANDOFF_DEFAULT = True     # (profiles/r05_decode_step.txt)
PREFETCH_O_DEFAULT = False      # weight prefetch of the o projection on a graph side branch next to the attention launch (profiles/r06_decode_step.txt)
MAX_PROMPT = 1024      # demo/demo_backend.py:300-302
MIN_PAD = 64           # demo/demo_backend.py:299


def handoff_norm(nw):
    """RMSNorm hand-off, overflow-safe form (round 6).  The producing launch stores round16(x_raw * nw) of the UN-normalised residual
    stream; in fp16 that product could overflow on a massive-activation row with a large norm weight, where HF's order (normalise first) cannot.
    Returns (nw / s, s) with s the power of two >= max |nw| (over every tenant): |nw / s| <= 1, so |x * nw / s| <= |x| never overflows, whatever
    x is.  The producer is then given ssq_scale = 1 / s^2 and the consumer eps / s^2: its row scalar becomes s * rsqrt(mean(x^2) + eps), i.e. the
    SAME product -- powers of two, so the same bits wherever the unscaled form did not overflow / underflow."""
    m = float(nw.detach().abs().max())
    s = 1.0 if not math.isfinite(m) or m <= 0.0 else 2.0 ** math.ceil(math.log2(m))
    return (nw.float() / s).to(nw.dtype), s


def _pow2_scale(m):
    """handoff_norm's s for a largest |norm weight| of m"""
    return 1.0 if not math.isfinite(m) or m <= 0.0 else 2.0 ** math.ceil(math.log2(m))


def fused_columns(widths, interleave8):
    """Where the output columns of several projections sit in a FusedDeltaLinear -- the ONE definition, used by __init__ (which permutes whole
    tensors, through fused_perm) and by load_tenant (which writes one tenant's columns).  A few integers, no tensor.  Returns (gsz, maps):
    gsz   columns per alpha group;
    maps  one (col_off, col_blk, col_stride) per projection: its column n is stored at col_off + (n // col_blk) * col_stride + n % col_blk."""
    widths = [int(n) for n in widths]
    if interleave8:
        assert len(widths) == 2 and widths[0] == widths[1] and widths[0] % 8 == 0
        return 8, [(0, 8, 16), (8, 8, 16)]
    gsz, maps, off = 0, [], 0
    for n in widths:
        gsz = math.gcd(gsz, n)
        maps.append((off, n, 0))
        off += n
    return gsz, maps


def fused_perm(widths, interleave8, device=None):
    """fused_columns' maps as an index tensor: stored row -> row of the plain concatenation; None where that is the identity"""
    if not interleave8:
        return None
    perm = torch.empty(sum(widths), dtype=torch.long, device=device)
    first = 0
    for n_i, (off, blk, stride) in zip(widths, fused_columns(widths, True)[1]):
        n = torch.arange(n_i, device=device)
        perm[off + (n // blk) * stride + n % blk] = first + n
        first += n_i
    return perm


def fused_alpha(coeffs, widths, interleave8):
    """alpha [T, G] (one scale per group of fused_columns' gsz stored columns) and alpha_pair [T, 2] (interleaved pairs; else None) from one
    tensor of T coeffs per projection.  With T = 1 it is one tenant's row of both."""
    if interleave8:
        pair = torch.stack([c.float().reshape(-1) for c in coeffs], 1)                          # [T, 2] (gate, up)
        return pair.repeat(1, widths[0] // 8), pair                                              # [T, N/8]: g, u, g, u, ...
    gsz = fused_columns(widths, False)[0]
    return torch.cat([c.float().reshape(-1, 1).expand(-1, n // gsz) for c, n in zip(coeffs, widths)], 1), None


def padded_length(longest):
    """demo/demo_backend.py:297-299: next power of two, at least 64."""
    return max(1 << max(longest - 1, 0).bit_length(), MIN_PAD)


class FusedDeltaLinear(nn.Module):
    """Several DiffCompress Linears that read the same input, launched as ONE:  W = cat(W_i), masks = cat(masks_i) along N,
    alpha[t, g] = coeff of the projection that owns scale group g (group size = gcd of the output widths).

    interleave8=True (two projections of equal width, a gate|up pair): the output rows are stored interleaved in blocks of 8
    ([g0..7 | u0..7 | g8..15 | u8..15 | ...]) so that a 16-column tile of the decode kernel holds 8 gate columns and the 8 matching
    up columns and SwiGLU can run in its epilogue.  `split()` undoes the order for callers that want the separate outputs."""

    tile_decode_weight = True     # keep a tile-major decode copy of the base weight (class switch)

    def __init__(self, weights, masks, coeffs, interleave8=False, decode_copies=True, base_int8=False, base_gptq4=False, group_size=128,
                 gptq4=None, dtype=None):
        """decode_copies=False skips the decode-only copies (packed sign words, tile-major base weight): a prefill-only user.
        base_int8=True: the (concatenated, interleaved) base is quantised once to the LLM.int8 vector-wise format (quant.quantize_base_int8); the
        16-bit `weight` becomes the reference-dequantised weight (what bitdelta/misc.py dequantize_model leaves in the model: prefill and every
        M > 1 launch run the unchanged 16-bit kernels on it) and the decode copy is the int8 tile-major weight + one fp32 scale per row.
        base_gptq4=True (not together with base_int8): the same with the 4-bit GPTQ format, groups of `group_size` (a multiple of 128) along K:
        the base is quantised once (quant.quantize_base_gptq4), `weight` becomes quant.dequantize_base_gptq4 of it, and the decode copy is the
        tile-major nibbles + one packed (scale, zero) dword per (group, column).  gptq4 = one (qweight, qzeros, scales) triple per projection (a
        GPTQ checkpoint) takes the place of the quantiser AND of `weights`, which must then be None: the widths come from the triples, the
        group size from the checkpoint (K / scales.shape[0]) and `dtype` says what the dequantised weight is cast to.  from_gptq4 spells it."""
        super().__init__()
        self.base_int8 = bool(base_int8)
        self.base_gptq4 = bool(base_gptq4)
        self.group_size = int(group_size)
        assert not (self.base_int8 and self.base_gptq4), "one quantised base form at a time"
        assert (gptq4 is None or self.base_gptq4) and (gptq4 is None) == (weights is not None), "a checkpoint replaces `weights`"
        qw = qz = sc = None
        if gptq4 is not None:             # the 16-bit weight is made once, from the concatenated checkpoint, below
            dev = masks[0].device
            widths = [t[0].shape[1] for t in gptq4]
            qw, qz, sc = cat_gptq4([tuple(u.to(dev) for u in t) for t in gptq4], interleave8=bool(interleave8))
            self.group_size = qw.shape[0] * 8 // sc.shape[0]
            weights = [torch.empty(n, 0, device=dev, dtype=dtype or torch.float16) for n in widths]      # (widths, dtype and device only)
        widths = [w.shape[0] for w in weights]
        self.widths = widths
        self.interleave8 = bool(interleave8)
        weight, mask = torch.cat(weights, 0), torch.cat(masks, 2)                               # [N, K], [T, K/32, N]
        perm = fused_perm(widths, self.interleave8, weight.device)
        if perm is not None:
            weight, mask = weight[perm], mask[:, :, perm]
        alpha, pair = fused_alpha(coeffs, widths, self.interleave8)
        if pair is not None:
            self.register_buffer("alpha_pair", pair.contiguous())
        else:
            self.alpha_pair = None
        cb = None
        if self.base_int8:
            cb, scb = quantize_base_int8(weight)
            weight = dequantize_base_int8(cb, scb, weight.dtype)
            self.register_buffer("wscale", weight_scale(scb))
        else:
            self.wscale = None
        if self.base_gptq4:
            if gptq4 is None:
                qw, qz, sc = quantize_base_gptq4(weight, self.group_size)
            assert self.group_size % 128 == 0 and (qw.shape[0] * 8) % self.group_size == 0, "group_size: a multiple of 128 that divides K"
            weight = dequantize_base_gptq4(qw, qz, sc, weight.dtype)
            self.register_buffer("group_params", pack_gptq4_params(qz, sc) if weight.shape[0] % 16 == 0 else None)
        else:
            self.group_params = None
        self.register_buffer("weight", weight.contiguous())
        self.register_buffer("mask", mask.contiguous())
        self.register_buffer("alpha", alpha.contiguous())                                        # [T, G]
        self.groups = alpha.shape[1]
        # decode copy of the sign words in the streaming kernel's packed order (tenants interleaved, natural k order); prefill keeps
        # the reference layout
        self.register_buffer("mask_packed", pack_decode_masks(self.mask) if (decode_copies and self.mask.shape[0] <= 16) else None)
        # ... and of the base weight in the kernel's tile-major order (one contiguous 4-KiB block per stage; +2 bytes per weight of HBM)
        N, K = self.weight.shape
        tiled = self.mask_packed is not None and self.tile_decode_weight and N % 16 == 0 and K % 128 == 0
        if self.base_int8:        # the decode copy IS the int8 weight: without it the mode would silently stream 16 bits
            assert tiled, "base_int8 needs the decode copies: N % 16 == 0, K % 128 == 0, at most 16 tenants"
            self.register_buffer("weight_tiled", tile_weight_int8(cb))
        elif self.base_gptq4:     # ... or the nibbles
            assert tiled, "base_gptq4 needs the decode copies: N % 16 == 0, K % 128 == 0, at most 16 tenants"
            self.register_buffer("weight_tiled", tile_weight_gptq4(qw))
        else:
            self.register_buffer("weight_tiled", tile_weight(self.weight) if tiled else None)

    @classmethod
    def from_gptq4(cls, triples, masks, coeffs, dtype=torch.float16, interleave8=False, decode_copies=True):
        """A fused Linear over the projections of a GPTQ checkpoint: triples = [(qweight int32 [K/8, N_i], qzeros int32 [K/G, N_i/8], scales fp16
        [K/G, N_i]), ...]; masks / coeffs as in __init__.  The group size is the checkpoint's (K / scales.shape[0])."""
        return cls(None, masks, coeffs, interleave8=interleave8, decode_copies=decode_copies, base_gptq4=True, gptq4=triples, dtype=dtype)

    def _decode_ok(self, x):
        B, M, K = x.shape
        return self.mask_packed is not None and B == self.mask.shape[0] and B * M <= 16 and \
            decode_shape_ok(B, M, self.weight.shape[0], K, B) and x.data_ptr() % 16 == 0 and \
            x.stride(0) % 8 == 0 and x.stride(1) % 8 == 0 and x.stride(2) == 1

    def fusable(self, x, swiglu=False):
        """True when forward_fused can take this input: decode shape inside the fused-norm envelope (and an interleaved pair for SwiGLU)"""
        B, M, K = x.shape
        return self._decode_ok(x) and fused_norm_ok(B, M, K) and (not swiglu or self.interleave8)

    def _dec_weight(self, x):
        """(weight, weight_tiled flag) for a decode launch: the tile-major copy when it exists and the launch has one row per tenant"""
        if self.weight_tiled is not None and self.use_tiled and x.shape[1] == 1:
            return self.weight_tiled, True
        return self.weight, False

    def _dec_scale(self, tiled):
        """weight_scale of a decode launch: the int8 decode copy's row scales (the 16-bit weights take none)"""
        return self.wscale if (tiled and self.base_int8) else None

    def _dec_q4(self, tiled):
        """group_params / group_size keywords of a decode launch: the 4-bit decode copy's (the other weights take none)"""
        return dict(group_params=self.group_params, group_size=self.group_size) if (tiled and self.base_gptq4) else {}

    use_tiled = True              # (A/B switch)

    def forward(self, x, residual=None, out_dtype=None, ssq_out=None, next_norm=None, xw_out=None, out=None, ssq_scale=1.0):
        """out_dtype=torch.float32: un-rounded partial sums (the row-parallel shards of tp.py reduce them across ranks).
        ssq_out (decode, with residual): RMSNorm hand-off, producer side -- the launch also leaves the per-row partial sums of squares of the
        updated residual stream for the next launch (`handoff_producer_ok`), and with next_norm [T, N] + xw_out [T, 1, N] the copy of it
        pre-multiplied by the NEXT norm's weight.  out: caller-provided destination (tp.py: the all-reduce's peer-mapped buffer)."""
        if self._decode_ok(x):
            w, wt = self._dec_weight(x)
            return binary_linear_decode(x, w, self.mask_packed, self.alpha, layout="packed", groups=self.groups,
                                        residual=residual, weight_tiled=wt, out_dtype=out_dtype, ssq_out=ssq_out,
                                        norm_weight=next_norm if ssq_out is not None else None, xw_out=xw_out, out=out, ssq_scale=ssq_scale,
                                        weight_scale=self._dec_scale(wt), **self._dec_q4(wt))
        assert ssq_out is None and xw_out is None
        return binary_linear(x, self.weight, self.mask, self.alpha, groups=self.groups, residual=residual, out_dtype=out_dtype, out=out)

    def residual_norm_ok(self, x, residual):
        """forward_residual_norm can take this input: prefill rows on the fused GEMM's fast path, the residual stream contiguous, rows the norm
        kernels take whole (N % 8 == 0, N <= 8192)"""
        B, M, K = x.shape
        N = self.weight.shape[0]
        return (M > 16 and K % 64 == 0 and N % 8 == 0 and N <= 8192 and x.stride(2) == 1 and x.data_ptr() % 16 == 0 and x.stride(0) % 8 == 0 and
                x.stride(1) % 8 == 0 and residual.is_contiguous() and self.mask.shape[0] in (1, B))

    def forward_residual_norm(self, x, residual, norm_weight, eps):
        """(residual + Linear(x), rmsnorm_tenant(of that, norm_weight)): the residual Linear of a decoder layer and the norm in front of the next
        Linear, one launch fewer when the Linear is split over k (bd_binary_linear_residual_norm); bit-identical to the two calls"""
        return binary_linear_residual_norm(x, self.weight, self.mask, self.alpha, residual, norm_weight, eps, groups=self.groups)

    def handoff_producer_ok(self, x):
        """this (residual) Linear can leave the sums of squares of its output behind: decode shape, one row per tenant, tile-major weight"""
        return (self._decode_ok(x) and x.shape[1] == 1 and x.shape[0] <= 8 and self.weight.shape[0] % 16 == 0 and
                self.weight_tiled is not None and self.use_tiled)

    def handoff_consumer_ok(self, x, swiglu=False):
        """forward_fused(..., ssq_in=...) can take this input: the resident-row envelope, tile-major weight (an interleaved pair for SwiGLU)"""
        B, M, K = x.shape
        return (self._decode_ok(x) and handoff_ok(B, M, K) and self.weight_tiled is not None and self.use_tiled and
                (not swiglu or self.interleave8))

    def forward_fused(self, x, norm_weight, eps, swiglu=False, ssq_in=None):
        """[RMSNorm(x; norm_weight) ->] this Linear [-> SwiGLU] in ONE launch.  With norm_weight, x is the un-normalised residual stream
        (`fusable(x)`); norm_weight=None keeps only the SwiGLU epilogue (x already normalised; needs `_decode_ok(x)`).
        ssq_in: the partial sums of squares of the residual stream left by the launch that produced it -- the norm then costs no reduction at
        all (`handoff_consumer_ok`); with norm_weight=None, x is the producer's pre-multiplied copy."""
        if swiglu:
            w, wt = self._dec_weight(x)
            return binary_linear_decode(x, w, self.mask_packed, self.alpha_pair, layout="packed", groups=2,
                                        norm_weight=norm_weight, eps=eps, swiglu=True, weight_tiled=wt, ssq_in=ssq_in,
                                        weight_scale=self._dec_scale(wt), **self._dec_q4(wt))
        w, wt = self._dec_weight(x)
        return binary_linear_decode(x, w, self.mask_packed, self.alpha, layout="packed", groups=self.groups,
                                    norm_weight=norm_weight, eps=eps, weight_tiled=wt, ssq_in=ssq_in, weight_scale=self._dec_scale(wt),
                                    **self._dec_q4(wt))

    def swiglu_ok(self, x):
        """True when forward_swiglu can take this input: an interleaved gate|up pair at prefill size on the fused GEMM's fast path"""
        B, M, K = x.shape
        return self.interleave8 and M > 16 and K % 64 == 0 and x.data_ptr() % 16 == 0 and x.stride(2) == 1 and \
            x.stride(0) % 8 == 0 and x.stride(1) % 8 == 0 and (self.mask.shape[0] in (1, B))

    def forward_swiglu(self, x):
        """act_fn(gate_proj(x)) * up_proj(x) of the MLP in ONE launch at prefill size (bd_binary_linear_swiglu): [B, M, inter]"""
        return binary_linear_swiglu(x, self.weight, self.mask, self.alpha_pair)

    def tenant_view(self, t):
        """This Linear for tenant t alone, on the SAME storage: the base weight whole, mask / alpha / alpha_pair sliced [t:t+1].  No decode copies
        (they interleave the tenants), so it serves prompts (more than 16 rows), which is what a one-tenant prefill runs."""
        v = FusedDeltaLinear.__new__(FusedDeltaLinear)
        nn.Module.__init__(v)
        v.base_int8, v.base_gptq4, v.group_size = self.base_int8, self.base_gptq4, self.group_size
        v.widths, v.interleave8, v.groups = self.widths, self.interleave8, self.groups
        v.weight, v.mask, v.alpha = self.weight, self.mask[t:t + 1], self.alpha[t:t + 1]
        v.alpha_pair = self.alpha_pair[t:t + 1] if self.alpha_pair is not None else None
        v.wscale = v.group_params = v.mask_packed = v.weight_tiled = None
        return v

    def check_tenant(self, t, masks, coeffs):
        """load_tenant's refusals, without touching anything: raises ValueError / IndexError; returns the coeffs as one-element fp32 tensors"""
        T, KW, _ = self.mask.shape
        if not (isinstance(t, int) and 0 <= t < T):
            raise IndexError("tenant %r: this Linear holds slots 0 .. %d" % (t, T - 1))
        if len(masks) != len(self.widths) or len(coeffs) != len(self.widths):
            raise ValueError("one mask and one coeff per projection: %d expected" % len(self.widths))
        out = []
        for m, c, n in zip(masks, coeffs, self.widths):
            if not torch.is_tensor(m) or m.dtype != torch.int32:
                raise ValueError("sign words are int32 tensors")
            if tuple(m.shape) != (KW, n):
                raise ValueError("sign words of shape %s where the module was built with %s" % (tuple(m.shape), (KW, n)))
            if m.device != self.mask.device:
                raise ValueError("sign words on %s, the module on %s" % (m.device, self.mask.device))
            c = torch.as_tensor(c)
            if c.numel() != 1 or not (c.is_floating_point()):
                raise ValueError("one floating-point coeff per projection")
            out.append(c.detach().reshape(1))
        return out

    @torch.no_grad()
    def load_tenant(self, t, masks, coeffs):
        """Replace slot t's fine-tune IN PLACE: one [K/32, N_i] int32 mask and one scalar coeff per projection, the widths the module was built
        with.  One launch of the sign-load kernel per projection writes tenant t's plane of `mask` and slot t of `mask_packed` (where the module
        keeps decode copies); alpha[t] / alpha_pair[t] follow __init__'s rule (fused_alpha).  No buffer is reallocated -- every data_ptr stays,
        so captured graphs stay valid -- and the base (16-bit, int8 or GPTQ) is not touched."""
        coeffs = self.check_tenant(t, masks, coeffs)
        require_gpu(self.mask, *masks)
        maps = fused_columns(self.widths, self.interleave8)[1]
        for m, (off, blk, stride) in zip(masks, maps):
            load_decode_masks(m if m.stride(1) == 1 else m.contiguous(), mask=self.mask[t], packed=self.mask_packed, slot=t, col_off=off,
                              col_blk=blk, col_stride=stride)
        alpha, pair = fused_alpha([c.to(self.alpha.device) for c in coeffs], self.widths, self.interleave8)
        self.alpha[t].copy_(alpha[0])
        if pair is not None:
            self.alpha_pair[t].copy_(pair[0])

    def tenant_signs(self, t):
        """(masks, coeffs) of slot t, un-fused: what load_tenant takes.  Concatenated projections are views of `mask`, an interleaved pair
        is de-interleaved into copies; the coeffs are views of alpha / alpha_pair."""
        m = self.mask[t]
        if self.interleave8:
            v = m.view(m.shape[0], self.widths[0] // 8, 2, 8)
            return [v[:, :, i, :].reshape(m.shape[0], -1) for i in range(2)], [self.alpha_pair[t, i] for i in range(2)]
        gsz, maps = fused_columns(self.widths, False)
        return [m[:, off:off + n] for (off, n, _) in maps], [self.alpha[t, off // gsz] for (off, _, _) in maps]

    def split(self, y):
        """per-projection outputs of y = forward(x)  (undoes the interleaved row order)"""
        if self.interleave8:
            v = y.reshape(*y.shape[:-1], self.widths[0] // 8, 2, 8)
            return v[..., 0, :].reshape(*y.shape[:-1], -1), v[..., 1, :].reshape(*y.shape[:-1], -1)
        return y.split(self.widths, dim=-1)

    def column_alpha(self, t):
        """tenant t's scale of every stored output row, [N]"""
        return self.alpha[t].repeat_interleave(self.weight.shape[0] // self.groups)

    def linear_bytes(self):
        """algorithmic HBM bytes of one decode launch: base once (one byte per weight in base_int8 mode; half a byte plus the 4-byte group
        parameters in base_gptq4 mode) + every tenant's signs (activations / outputs / row scales are noise)"""
        if self.base_gptq4:
            return self.weight.numel() // 2 + self.group_params.numel() * 4 + self.mask.numel() * 4
        return self.weight.numel() * (1 if self.base_int8 else self.weight.element_size()) + self.mask.numel() * 4


class RopeSpec(collections.namedtuple("RopeSpec", "theta kind factor low_freq_factor high_freq_factor original_max_position_embeddings inv_freq")):
    """One fine-tune's rotary embedding as data (rope_spec makes and validates it): hashable, compared by value."""
    __slots__ = ()


_ROPE_REFUSED = {
    "dynamic": "its table depends on the sequence length, and the tables here are built once",
    "yarn": "it needs an attention factor other than 1 on cos / sin",
    "longrope": "it needs an attention factor other than 1 and switches tables with the sequence length",
}


def rope_spec(theta=10000.0, scaling=None, inv_freq=None):
    """A tenant's rotary embedding, validated on the host: a hashable RopeSpec.  theta: HF's `rope_theta`, finite and > 0.  scaling: HF's
    `rope_scaling` / `rope_parameters` dict or None -- `rope_type` (or the older key `type`) "default", "linear" (`factor` >= 1: every
    frequency divided by it) or "llama3" (`factor` >= 1, `low_freq_factor`, `high_freq_factor`, `original_max_position_embeddings`: the
    frequency-band rule).  inv_freq: instead of the formula, the head_dim / 2 inverse frequencies themselves (any fp32 sequence or tensor;
    finite), for a static scheme this module does not spell; not together with scaling.  Refused (ValueError): "dynamic" (the table
    depends on the sequence length), "yarn" and "longrope" (they scale cos / sin by an attention factor other than 1), unknown types,
    factor < 1, a theta that is not finite and positive, a bad inv_freq.  Its length is checked against the head size where the spec
    meets one (rope_inv_freq)."""
    try:
        th = float(theta)
    except (TypeError, ValueError):
        raise ValueError("rope theta = %r: a number is required" % (theta,))
    if not (math.isfinite(th) and th > 0.0):
        raise ValueError("rope theta = %r: a finite value > 0 is required" % (theta,))
    if inv_freq is not None:
        if scaling is not None:
            raise ValueError("inv_freq and scaling together: the caller's frequencies already are the scaled ones")
        try:
            vals = torch.as_tensor(inv_freq).detach().to("cpu", torch.float32)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError("inv_freq = %r: a vector of numbers is required" % (inv_freq,))
        if vals.dim() != 1 or vals.numel() == 0 or not bool(torch.isfinite(vals).all()):
            raise ValueError("inv_freq: a vector of head_dim / 2 finite values is required")
        return RopeSpec(th, "inv_freq", 1.0, None, None, None, tuple(vals.tolist()))
    if scaling is None:
        return RopeSpec(th, "default", 1.0, None, None, None, None)
    if not isinstance(scaling, collections.abc.Mapping):
        raise ValueError("rope scaling = %r: HF's rope_scaling dict is required" % (scaling,))
    kind = scaling.get("rope_type", scaling.get("type", "default"))
    if kind in _ROPE_REFUSED:
        raise ValueError("rope scaling type %r is not supported: %s" % (kind, _ROPE_REFUSED[kind]))
    if kind not in ("default", "linear", "llama3"):
        raise ValueError("rope scaling type %r: \"default\", \"linear\" or \"llama3\" is required" % (kind,))
    if kind == "default":
        return RopeSpec(th, "default", 1.0, None, None, None, None)

    def number(key):
        try:
            v = float(scaling[key])
        except (KeyError, TypeError, ValueError):
            raise ValueError("rope scaling %r needs a number %r" % (kind, key))
        if not math.isfinite(v):
            raise ValueError("rope scaling %s = %r: a finite value is required" % (key, scaling[key]))
        return v
    factor = number("factor")
    if factor < 1.0:
        raise ValueError("rope scaling factor = %r: a value >= 1 is required" % (scaling["factor"],))
    if kind == "linear":
        return RopeSpec(th, "linear", factor, None, None, None, None)
    lo, hi, old = number("low_freq_factor"), number("high_freq_factor"), number("original_max_position_embeddings")
    if not (old > 0 and lo > 0 and hi > lo):
        raise ValueError("rope scaling llama3: original_max_position_embeddings > 0 and 0 < low_freq_factor < high_freq_factor are required")
    return RopeSpec(th, "llama3", factor, lo, hi, int(old) if old == int(old) else old, None)


ROPE_DEFAULT = rope_spec()      # rope_theta 10000, no scaling: the table every decoder had before specs


def rope_inv_freq(spec, dim, device=None):
    """The inverse frequencies of a RopeSpec for head size `dim`, fp32 [dim / 2], computed on `device` with the torch operations -- and in the
    order -- of the current transformers definitions (modeling_rope_utils): 1 / theta^(2i / dim); "linear": that divided by factor;
    "llama3": wavelengths above original / low_freq_factor divided by factor, those below original / high_freq_factor kept, the band
    between interpolated.  A caller-supplied inv_freq is returned as given; a length other than dim / 2 is a ValueError."""
    if not isinstance(spec, RopeSpec):
        raise ValueError("%r: a rope_spec() record is required" % (spec,))
    if spec.kind == "inv_freq":
        if len(spec.inv_freq) != dim // 2:
            raise ValueError("inv_freq holds %d values where head_dim / 2 = %d are required" % (len(spec.inv_freq), dim // 2))
        return torch.tensor(spec.inv_freq, dtype=torch.float32, device=device)
    inv = 1.0 / (spec.theta ** (torch.arange(0, dim, 2, device=device, dtype=torch.float32) / dim))
    if spec.kind == "linear":
        inv /= spec.factor
    elif spec.kind == "llama3":
        factor, lo, hi, old = spec.factor, spec.low_freq_factor, spec.high_freq_factor, spec.original_max_position_embeddings
        low_wavelen, high_wavelen = old / lo, old / hi
        wavelen = 2 * math.pi / inv
        scaled = torch.where(wavelen > low_wavelen, inv / factor, inv)
        smooth = (old / wavelen - lo) / (hi - lo)
        smoothed = (1 - smooth) * scaled / factor + smooth * scaled
        medium = ~(wavelen < high_wavelen) * ~(wavelen > low_wavelen)
        inv = torch.where(medium, smoothed, scaled)
    return inv


def rope_tables(length, dim, device, dtype, spec=ROPE_DEFAULT):
    """(cos, sin) [length, dim] in `dtype` for a RopeSpec: the angle of (position, i) is the fp32 product position * inv_freq[i] (HF's matmul of
    the two), the rotate-half sign is folded into sin, then both are cast.  A position is a cache row."""
    inv = rope_inv_freq(spec, dim, device)
    ang = torch.outer(torch.arange(length, device=device, dtype=torch.float32), inv)
    ang = torch.cat([ang, ang], dim=-1)
    d = dim // 2
    sin = ang.sin()
    sin = torch.cat([-sin[:, :d], sin[:, d:]], dim=-1)                  # rotate-half sign folded in
    return ang.cos().to(dtype), sin.to(dtype)


def _rope_tables(length, dim, device, dtype, base=10000.0):
    return rope_tables(length, dim, device, dtype, rope_spec(base))


def _rope(x, cos, sin):
    # x [T, H, S, D]; cos / sin [S, D], or per tenant [T, 1, S, D]
    d = x.shape[-1] // 2
    rot = torch.cat([x[..., d:], x[..., :d]], dim=-1)
    return torch.addcmul(x * cos, rot, sin)


class TenantDecoder(nn.Module):
    """Llama / Mistral decoder for T tenants over one base: every `*proj*` Linear is base + T 1-bit deltas (fused HIP launches),
    embedding / norms / lm_head are per tenant (stacked)."""

    MIN_STOP_WIDTH = 8          # stop ids per tenant the static stop table holds before it has to grow (to the next power of two)
    MAX_STATIC_SLOTS = 4        # captured decode-step graphs kept alive at once (LRU over stop-table width x glue switches)

    def __init__(self, cfg, tenants, device, dtype, max_len=MAX_PROMPT + 64, eps=1e-5, base_int8=False, base_gptq4=False, rope=None):
        """rope: the rotary embedding (rope_spec).  None: rope_theta 10000, unscaled, one [max_len, head_dim] table pair for every tenant.  One
        spec: one shared pair built from it (a base with another rope_theta; same launches).  A list of `tenants` specs: a pair per tenant,
        cos / sin [tenants, max_len, head_dim] -- a fine-tune's RoPE scaling is part of the fine-tune -- which load_tenant(rope=) rewrites
        row by row."""
        super().__init__()
        hd_ = cfg[0] // cfg[3]
        self.rope_per_tenant = rope is not None and not isinstance(rope, RopeSpec)
        if self.rope_per_tenant:
            specs = list(rope)
            if len(specs) != tenants:
                raise ValueError("%d rope specs for %d tenants" % (len(specs), tenants))
            self._rope_default = ROPE_DEFAULT           # what load_tenant(rope=None) gives a slot
        else:
            self._rope_default = ROPE_DEFAULT if rope is None else rope
            specs = [self._rope_default] * tenants
        for sp in specs:
            rope_inv_freq(sp, hd_)                      # (refuses a record that is no spec, or frequencies of another head size)
        self._rope = specs                              # slot -> its spec (tenant_rope)
        self.base_gptq4 = bool(base_gptq4)  # ... or a 4-bit GPTQ base (FusedDeltaLinear(base_gptq4=True)); lm_head, embeddings and norms stay 16-bit
        self.base_int8 = bool(base_int8)    # the delta Linears stream an int8 base at decode (FusedDeltaLinear(base_int8=True)); lm_head stays 16-bit
        self.cfg, self.T, self.dtype, self.dev, self.eps = cfg, tenants, dtype, torch.device(device), eps
        hid, inter, nl, heads, kvh, vocab = cfg
        self.hd = hid // heads
        self.max_len = max_len
        self.layers = nn.ModuleList()
        self.embed = None           # [T, vocab, hid]
        self.final_norm = None      # [T, hid]
        self.lm_head = None         # [T, vocab, hid]
        if self.rope_per_tenant:
            pairs = [rope_tables(max_len, self.hd, self.dev, dtype, sp) for sp in specs]
            cos, sin = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
        else:
            cos, sin = rope_tables(max_len, self.hd, self.dev, dtype, self._rope_default)
        self.register_buffer("cos", cos, persistent=False)
        self.register_buffer("sin", sin, persistent=False)
        self._graph = None
        self.fast_glue = True       # decode steps use the HIP glue kernels (serving_ops); False = stock torch ops everywhere
        self.swiglu_epilogue = False  # prefill: SwiGLU inside the gate|up GEMM (256-row tiles from 256 rows per tenant, pair tiles for <= 64-row
                                      # prompts): measured slower than GEMM + one pass both times (6 x 64 rows: gate|up 162 -> 186 us against a 9-us pass)
        self.step_kernels = True      # decode step: mask extension + embedding gather, and argmax + token / output / stop / position updates, as
                                      # one HIP launch each instead of ~13 stock ops (round 6)
        self.short_prompt_fusions = True   # multi-tenant prefill of short prompts (round 6): RoPE + KV-cache append in one launch; <= 64 rows per
                                           # tenant: the norms ride on the split-k reduce launches of o / down
        self.hip_prefill_attention = True      # prefill: RoPE + flash-style attention kernels instead of torch SDPA over a [L, Lc] mask
        self.fuse_glue = True       # ... and fold RMSNorm / SwiGLU into the Linear launches where the shapes allow (bit-identical)
        # Which glue is folded where, by same-process A/B of the whole step (ms per step, Mistral-7B x 6, tile-major weights).  Round 2
        # (profiles/r02_decode_step.txt): separate launches 5.35 | SwiGLU in gate|up's epilogue 5.11 | + RMSNorm in gate|up's prologue
        # 5.17 | + RMSNorm in q|k|v's prologue 5.28.  Round 4, nt weight loads (profiles/r04_decode_step_ab.txt): 5.28 | 5.02 | 4.94 | 5.05.
        # The epilogue is free; a norm prologue makes 256 blocks each re-read and re-normalise all rows (~6 us in front of the launch)
        # to save a 4.4 us kernel: it pays on the long gate|up launch, not on the short q|k|v one.
        self._static = {}               # (stop-table width, glue switches) -> static request state + captured decode-step graph (LRU)
        self._kv_cache = None           # ONE KV cache per decoder, shared by every slot
        self._capture_stream = None
        self._tenant_views = {}         # tenant -> one-tenant view of this decoder (tenant_view)
        self._sessions = weakref.WeakSet()   # live TenantSessions: load_tenant drops their captured graphs when a hand-off scale changes
        # one tag per slot: WHICH fine-tune it holds, as far as anybody can tell.  A fresh unique object at construction and at every load_tenant;
        # load_tenant(tag=) names it instead (tenant_tag).
        self._tags = [object() for _ in range(tenants)]
        self.fuse_qkv_norm = False      # RMSNorm folded into the q|k|v launch
        # RMSNorm folded into the gate|up launch (SwiGLU stays in its epilogue either way): every block re-normalises all rows (rows + norm
        # weights from L2) to save one ~4.5 us launch.  Same-process A/Bs at the end of round 4, with the resident-row form (which needs no
        # norm) at 2 stages on every eligible launch: 1 tenant 3.353 fused vs 3.386 ms separate, 2 tenants 3.790 vs 3.823, 4 tenants 4.244
        # vs 4.226 (and 4.218 vs 4.243 in a later session: a wash), 6 tenants 4.771 vs 4.700 -- the prologue's cost grows with the rows,
        # the saved launch does not (profiles/r04_decode_step_ab.txt).
        self.fuse_gateup_norm = tenants <= 4
        # RMSNorm by HAND-OFF (round 5): o / down leave the per-row partial sums of squares of the residual stream they write; the next
        # q|k|v / gate|up launch applies the norm weight on its resident rows and 1/rms in its epilogue -- neither a stand-alone norm launch
        # nor a per-block reduction.  Takes precedence over the two switches above where its envelope holds (tile-major weights, <= 8
        # tenants, hidden >= 2048); not bit-identical to the separate launches (one rounding moves), same accuracy.
        self.norm_handoff = NORM_HANDOFF_DEFAULT
        # Weight prefetch on a hipGraph SIDE BRANCH (round 6): forked before the decode attention launch, joined before the o projection, a
        # cache_warm launch reads the o projection's tile-major weight and packed sign words so that they sit in the Infinity Cache when the
        # projection starts (the attention launch is a latency-bound chain that leaves HBM idle).  No arithmetic changes.
        self.prefetch_o = PREFETCH_O_DEFAULT
        self._pf_stream = None
        self._ssq = None                # [hidden / 16, 16] fp32: partial sums of squares of the current residual stream
        self._xw = None                 # [T, 1, hidden]: the residual stream times the weight of the norm that reads it next
        # (round 2 also shipped a persistent per-layer chain launch, bd_decode_chain: bit-identical but 5.91 vs 5.33 ms per step in every
        # same-process A/B, so it was removed from the library in round 3 -- profiles/r02_decode_chain_*.txt keep the measurements)

    # ---------------------------------------------------------------- construction
    @classmethod
    def synthetic(cls, name, tenants, device, dtype=torch.float16, seed=0, layers=None, max_len=MAX_PROMPT + 64, shared_heads=False, base_int8=False,
                  base_gptq4=False, rope=None):
        """Random weights with the statistics of SURVEY.md section 8(d): W ~ N(0, 0.02^2), fine-tune = W + N(0, (5e-4)^2) per
        tenant (alpha = mean|delta| ~ 4e-4).  Embedding / norm / lm_head are per tenant as in the reference's diff.pt files
        (`shared_heads=True` stores them once and expands -- same arithmetic, used only to keep test models small).  rope: as in __init__."""
        cfg = MODEL_CONFIGS[name] if isinstance(name, str) else tuple(name)
        hid, inter, nl, heads, kvh, vocab = cfg
        nl = layers or nl
        self = cls(cfg, tenants, device, dtype, max_len=max_len, base_int8=base_int8, base_gptq4=base_gptq4, rope=rope)
        gen = torch.Generator(device=device).manual_seed(seed)
        hd = hid // heads

        def delta_linear(n_out, n_in):
            w = (torch.randn(n_out, n_in, device=device, generator=gen) * 0.02).to(dtype)
            masks, coeffs = [], []
            for _ in range(tenants):
                fine = (w.float() + torch.randn(n_out, n_in, device=device, generator=gen) * 5e-4).to(dtype)
                m, c = binarize(w, fine)
                masks.append(m)
                coeffs.append(c)
            return w, torch.stack(masks, 0), torch.stack(coeffs, 0)

        def fused(*shapes, interleave8=False):
            parts = [delta_linear(o, i) for o, i in shapes]
            return FusedDeltaLinear([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts], interleave8=interleave8, base_int8=base_int8,
                                    base_gptq4=base_gptq4)

        def per_tenant(*shape, scale=None):
            reps = 1 if shared_heads else tenants
            if scale is None:
                t = 1.0 + 0.1 * torch.randn(reps, *shape, device=device, generator=gen)
            else:
                t = torch.randn(reps, *shape, device=device, generator=gen) * scale
            t = t.to(dtype)
            return t.expand(tenants, *shape) if shared_heads else t

        for _ in range(nl):
            layer = nn.Module()
            layer.qkv = fused((heads * hd, hid), (kvh * hd, hid), (kvh * hd, hid))
            layer.o = fused((hid, heads * hd))
            layer.gate_up = fused((inter, hid), (inter, hid), interleave8=(inter % 8 == 0))
            layer.down = fused((hid, inter))
            layer.norm1 = per_tenant(hid)
            layer.norm2 = per_tenant(hid)
            self.layers.append(layer)
        self.embed = per_tenant(vocab, hid, scale=0.02)
        self.final_norm = per_tenant(hid)
        self.lm_head = per_tenant(vocab, hid, scale=0.02)
        return self

    # ---------------------------------------------------------------- accounting
    def linear_bytes_per_step(self):
        """algorithmic HBM bytes of the Linear launches of one decode step (the roofline numerator): delta Linears + lm_heads"""
        b = sum(l.qkv.linear_bytes() + l.o.linear_bytes() + l.gate_up.linear_bytes() + l.down.linear_bytes() for l in self.layers)
        return b, self.T * self.lm_head.shape[1] * self.lm_head.shape[2] * self.lm_head.element_size()

    def linear_param_count(self):
        return sum(l.qkv.weight.numel() + l.o.weight.numel() + l.gate_up.weight.numel() + l.down.weight.numel() for l in self.layers)

    # ---------------------------------------------------------------- forward
    def new_cache(self, length=None):
        length = length or self.max_len
        _, _, _, heads, kvh, _ = self.cfg
        mk = lambda: torch.zeros(self.T, kvh, length, self.hd, device=self.dev, dtype=self.dtype)
        return {"k": [mk() for _ in self.layers], "v": [mk() for _ in self.layers],
                "valid": torch.zeros(self.T, length, dtype=torch.bool, device=self.dev)}

    # prefill: the HIP per-tenant RMSNorm (ONE launch).  Its block-per-row form is used up to this many rows and stock torch beyond (F.rms_norm +
    # the weight multiply = three launches, but faster per row on long prompts: 2048-row prefill 8.5 vs 13.1 us, profiles/r03_prefill_glue.txt);
    # since late in round 5 hidden sizes that are multiples of 2048 take the wave-per-row form at every size (rmsnorm_rows_kernel, bit-identical):
    # 6 tenants x 256 rows 10.7 us against 21.2 for the torch composition, 2048 rows 12.0 against 22.5 (tools/bench_norm.py; torch's rms_norm with
    # a FUSED weight -- one weight for all rows, not this loop's per-tenant weights -- is 10.1: bench_model keeps it).  A 6-tenant request
    # padded to 64 tokens (384 rows) spends 15.5 us per norm in the three torch kernels against ~5 us here (profiles/r05_mt_prefill_tiles.txt).
    HIP_NORM_MAX_ROWS = 1024

    def _norm(self, x, w):
        H = x.shape[-1]
        # (hidden sizes of 2048 / 4096 / 6144 / 8192: the wave-per-row kernel, any number of rows -- bd_srv_rmsnorm picks it from 64 rows on)
        if self.fast_glue and H % 8 == 0 and (x.shape[1] <= 16 or x.shape[0] * x.shape[1] <= self.HIP_NORM_MAX_ROWS or (H % 2048 == 0 and H <= 8192)):
            return ops.rmsnorm_tenant(x if x.is_contiguous() else x.contiguous(), w, self.eps)
        return F.rms_norm(x, (x.shape[-1],), None, self.eps) * w[:, None, :]

    def _hn(self, layer, which):
        """(nw / s, s) of a layer's norm for the hand-off (handoff_norm), computed once"""
        key = "_hn_" + which
        v = getattr(layer, key, None)
        if v is None:
            # s is read on the host and baked into captured launches (ssq_scale, eps / s^2): it is made in the warm-up step, never inside a capture
            assert not torch.cuda.is_current_stream_capturing(), "the hand-off norm cache is computed outside graph capture"
            v = handoff_norm(getattr(layer, which))
            setattr(layer, key, v)
        return v

    # ---------------------------------------------------------------- swapping one slot's fine-tune
    _DENSE = ("embed", "final_norm", "lm_head")
    _LINEARS = ("qkv", "o", "gate_up", "down")

    def tenant_state(self, t):
        """Slot t's fine-tune as load_tenant takes it: {"layers": [{"qkv" | "o" | "gate_up" | "down": (masks, coeffs), "norm1", "norm2"}, ...],
        "embed", "final_norm", "lm_head"} -- un-fused, de-interleaved sign words and coeffs per projection, the dense rows.  Views of this decoder's
        storage where the layout allows (copies for interleaved pairs): clone it to keep it across a later load into the same slot."""
        assert 0 <= t < self.T
        layers = []
        for layer in self.layers:
            d = {name: getattr(layer, name).tenant_signs(t) for name in self._LINEARS}
            d["norm1"], d["norm2"] = layer.norm1[t], layer.norm2[t]
            layers.append(d)
        return {"layers": layers, "embed": self.embed[t], "final_norm": self.final_norm[t], "lm_head": self.lm_head[t]}

    def _check_state(self, t, state):
        if not (isinstance(t, int) and 0 <= t < self.T):
            raise IndexError("tenant %r: this decoder holds slots 0 .. %d" % (t, self.T - 1))
        if len(state["layers"]) != len(self.layers):
            raise ValueError("%d layers in the state, %d in the decoder" % (len(state["layers"]), len(self.layers)))
        rows = [(getattr(self, n), state[n], n) for n in self._DENSE]
        for layer, d in zip(self.layers, state["layers"]):
            rows += [(layer.norm1, d["norm1"], "norm1"), (layer.norm2, d["norm2"], "norm2")]
            for name in self._LINEARS:
                getattr(layer, name).check_tenant(t, *d[name])
        for dst, src, name in rows:
            if dst.stride(0) == 0 and dst.shape[0] > 1:
                raise ValueError("%s is one row expanded over the tenants (shared_heads=True): a slot cannot be written alone" % name)
            if tuple(src.shape) != tuple(dst.shape[1:]) or src.dtype != dst.dtype:
                raise ValueError("%s: %s %s where the decoder holds %s %s" % (name, tuple(src.shape), src.dtype, tuple(dst.shape[1:]), dst.dtype))

    def _hn_peaks(self, t, state):
        """Host values the s rule needs, for every cached hand-off norm at once: {(layer index, which): max |new row t|}, and each entry's
        per-tenant maxima `_hnpeak_*` (kept on the host from then on).  ONE device reduction chain and ONE transfer per load, however many
        entries are cached; no transfer at all when nothing is cached, or when the maxima are known and the new rows are host tensors."""
        keys, parts, fresh = [], [], []
        for li, (layer, d) in enumerate(zip(self.layers, state["layers"])):
            for which in ("norm1", "norm2"):
                if getattr(layer, "_hn_" + which, None) is not None:
                    keys.append((li, which))
                    parts.append(d[which].detach().abs().max().reshape(1).float())
        for li, which in keys:
            if getattr(self.layers[li], "_hnpeak_" + which, None) is None:
                fresh.append((li, which))
                parts.append(getattr(self.layers[li], which).detach().abs().amax(dim=1).float())
        if not keys:
            return {}
        if any(p.is_cuda for p in parts):
            parts = [p.to(self.dev) for p in parts]
        host = torch.cat(parts).tolist()
        for i, (li, which) in enumerate(fresh):
            lo = len(keys) + i * self.T
            setattr(self.layers[li], "_hnpeak_" + which, host[lo:lo + self.T])
        return dict(zip(keys, host[:len(keys)]))

    def _reload_hn(self, layer, which, t, peak):
        """a cached hand-off norm (nw / s, s) after row t of the norm changed (peak = max |new row|, a host float): the row is rewritten in place
        while the power of two s over the new tenant set is the old one; otherwise the entry is rebuilt.  Returns True when s changed
        (captured launches baked the old one)."""
        v = getattr(layer, "_hn_" + which)
        nw = getattr(layer, which)
        peaks = getattr(layer, "_hnpeak_" + which)
        peaks[t] = peak
        m = max(peaks) if all(math.isfinite(p) for p in peaks) else float("nan")
        s = _pow2_scale(m)
        if s == v[1]:
            v[0][t].copy_((nw[t].float() / s).to(nw.dtype))
            return False
        setattr(layer, "_hn_" + which, ((nw.float() / s).to(nw.dtype), s))
        return True

    def tenant_tag(self, t):
        """Slot t's fine-tune tag: the hashable load_tenant(tag=) gave it, or the unique object it got at construction / at its last untagged load.
        Two slots -- or one slot at two times -- hold the same fine-tune, as far as the decoder can tell, exactly when their tags are equal.
        Nothing in this package reads the tag yet: it is bookkeeping for a caller that keeps data per fine-tune outside the decoder."""
        return self._tags[t]

    def tenant_rope(self, t):
        """Slot t's rotary embedding (a rope_spec record): what its q and k are rotated with, at construction or since its last load_tenant"""
        return self._rope[t]

    def _load_rope(self, t, rope):
        """the spec slot t carries after load_tenant(rope=): None is the decoder's default.  Every refusal happens here, before the first write: a
        record that is no spec or does not fit the head size, and -- on a decoder with ONE table for all tenants -- a spec other than the
        decoder's, which slot t could not have alone."""
        spec = self._rope_default if rope is None else rope
        rope_inv_freq(spec, self.hd)
        if not self.rope_per_tenant and spec != self._rope_default:
            raise ValueError("this decoder rotates every tenant with one table (%r): build it with a list of rope specs to give slot %d its own"
                             % (self._rope_default, t))
        return spec

    def _rope_rows(self, pos_idx):
        """the table rows of positions pos_idx as the stock-op attention takes them: [S, D], or per tenant [T, 1, S, D] (broadcast over the heads)"""
        if self.cos.dim() == 3:
            return self.cos[:, pos_idx].unsqueeze(1), self.sin[:, pos_idx].unsqueeze(1)
        return self.cos[pos_idx], self.sin[pos_idx]

    @torch.no_grad()
    def load_tenant(self, t, state, tag=None, rope=None):
        """Replace the fine-tune in slot t IN PLACE (state: see tenant_state): every delta Linear's sign words and scales through
        FusedDeltaLinear.load_tenant, the tenant's rows of the norms, the embedding and the lm_head by copies on the current stream.  Storage and
        pointers stay, so captured decode steps stay valid and the other tenants' rows are not touched.  The one thing a captured step bakes that
        depends on the whole tenant set is the hand-off norm's power-of-two scale s (handoff_norm): where a cached entry's s is still right
        the cached row is rewritten in place; where it moved, the entry is rebuilt and every captured graph of this decoder and of its live
        sessions is dropped (the next step captures again).  Host synchronisation: at most ONE device-to-host read per load -- the maxima of
        the new norm rows of every cached entry, reduced on the device and read back together (_hn_peaks); none when no hand-off norm is cached
        yet, or when the state's norm rows are host tensors.  That read waits for work already queued on the stream.  Refuses a decoder whose per-tenant tensors are one row expanded (shared_heads).
        The caller makes sure slot t is not generating (TenantSession.load_tenant checks).
        tag: the slot's fine-tune tag afterwards (tenant_tag).  None, the default, gives it a fresh unique object: nothing kept from before the
        load matches it.  A hashable (say the fine-tune's name) is the CALLER's statement that equal tags mean equal weights: after A -> B -> A in
        one slot the tag is A's again, and every slot loaded with tag A compares equal.  An unhashable tag is refused (TypeError) first, and
        every refusal leaves the tag as it was.  From the first write on the slot carries a fresh unique object, and the caller's tag is
        assigned after the last: a load that fails midway never leaves a tag that matches anything on partly new weights.
        rope: the slot's rotary embedding afterwards (rope_spec; tenant_rope); None, the default, is the decoder's default spec -- a load defines
        the whole slot, positional encoding included.  On a decoder with per-tenant tables the rows cos[t] / sin[t] are rebuilt on the device
        and copied in place on the current stream (no host read; storage, pointers and captured graphs stay valid).  On a decoder with one
        shared table a spec other than the decoder's is refused (ValueError) before the first write.  Keys of slot t that are still in a
        cache were rotated with the old table: they are not reusable (TenantSession.load_tenant forgets them)."""
        if tag is not None:
            hash(tag)
        self._check_state(t, state)
        spec = self._load_rope(t, rope)
        require_gpu(self.embed)
        assert not torch.cuda.is_current_stream_capturing(), "a load reads the hand-off scale on the host: not inside a graph capture"
        peaks = self._hn_peaks(t, state)                   # the load's one host read (none without a cached hand-off norm)
        rescaled = False
        self._tags[t] = object()                           # (every refusal is behind us; the first write follows)
        for li, (layer, d) in enumerate(zip(self.layers, state["layers"])):
            for name in self._LINEARS:
                getattr(layer, name).load_tenant(t, *d[name])
            for which in ("norm1", "norm2"):
                getattr(layer, which)[t].copy_(d[which])
                if (li, which) in peaks:
                    rescaled |= self._reload_hn(layer, which, t, peaks[(li, which)])
        for name in self._DENSE:
            getattr(self, name)[t].copy_(state[name])
        if spec != self._rope[t]:                          # (per-tenant tables only: _load_rope refused anything else)
            cos, sin = rope_tables(self.cos.shape[-2], self.hd, self.dev, self.dtype, spec)
            self.cos[t].copy_(cos)
            self.sin[t].copy_(sin)
            self._rope[t] = spec
        # The decoder's own one-tenant view is dropped and rebuilt on its next use.  That is enough: a view slices this storage and caches nothing
        # derived from tenant data (it only prefills, where no hand-off norm is made), so a view a caller still holds reads the new fine-tune too.
        self._tenant_views.pop(t, None)
        if tag is not None:
            self._tags[t] = tag
        if rescaled:
            for slot in self._static.values():
                slot["graph"] = None
            for sess in list(self._sessions):
                sess._graphs.clear()
        return rescaled

    def _layer(self, layer, x, cos, sin, cache, li, pos_idx, attn_mask, ssq_valid=False, next_layer=None, h_in=None, ragged=None):
        """one decoder layer; returns (x, ssq_valid): whether self._ssq / self._xw hold the partial sums of squares of the returned x and its
        copy pre-multiplied by the NEXT layer's input norm weight (next_layer; None after the last layer) -- both in handoff_norm's scaled form.
        h_in: norm1 of x when the previous layer's down projection already produced it (prefill, forward_residual_norm); the third return value is
        that tensor for the next layer (or None).  ragged: (pos [T], active [T]) of a TenantSession step -- one position per tenant; pos_idx is
        then not looked at."""
        T, S, hid = x.shape
        _, inter, _, heads, kvh, _ = self.cfg
        hd = self.hd
        fuse = S == 1 and self.fast_glue and self.fuse_glue and x.is_contiguous()
        handoff = fuse and self.norm_handoff and hid % 16 == 0
        if handoff and self._ssq is None:
            self._ssq = torch.empty(hid // 16, 16, dtype=torch.float32, device=x.device)
            self._xw = torch.empty(T, 1, hid, dtype=x.dtype, device=x.device)
        if handoff and ssq_valid:
            s1 = self._hn(layer, "norm1")[1]
            qkv = layer.qkv.forward_fused(self._xw, None, self.eps / (s1 * s1), ssq_in=self._ssq)    # rows already carry norm1's weight / s; s/rms in the epilogue
        elif fuse and self.fuse_qkv_norm and layer.qkv.fusable(x):
            qkv = layer.qkv.forward_fused(x, layer.norm1, self.eps)              # RMSNorm in the Linear's prologue: one launch
        else:
            qkv = layer.qkv(h_in if h_in is not None else self._norm(x, layer.norm1))
        ck, cv = cache["k"][li], cache["v"][li]
        short = S > 1 and self.fast_glue and self.short_prompt_fusions
        pairs = short and S <= 64 and T >= 2                                 # the request runs on pair tiles (two tenants per 128-row tile)
        pf = None
        if S == 1 and self.fast_glue and self.prefetch_o and layer.o.mask_packed is not None:
            # fork: the prefetch depends on nothing the layer computes; it is ordered behind the q|k|v launch only so that it runs next to attention
            if self._pf_stream is None:
                self._pf_stream = torch.cuda.Stream(device=x.device)
            pf, cur = self._pf_stream, torch.cuda.current_stream(x.device)
            pf.wait_stream(cur)
            with torch.cuda.stream(pf):
                w_o = layer.o.weight_tiled if (layer.o.weight_tiled is not None and layer.o.use_tiled) else layer.o.weight
                ops.cache_warm(w_o, layer.o.mask_packed)
        if ragged is not None:
            # a session's step: the same launch with each tenant at its own position; there is no stock-op form of it to fall to
            if not (S == 1 and self.fast_glue and ops.decode_attention_supported(heads, kvh, hd)):
                raise RuntimeError("a ragged decode step needs the HIP decode attention (fast_glue, head_dim 128, 1 / 4 / 8 query heads per kv head)")
            a = ops.decode_attention_ragged(qkv, self.cos, self.sin, ck, cv, cache["valid"], ragged[0], ragged[1], heads, kvh)
        elif (cache.get("chunk") is not None and self.fast_glue and self.hip_prefill_attention and hd == 128 and qkv.is_contiguous()
              and not layer.qkv.interleave8):
            # a chunk of S rows at positions q0 .. q0 + S - 1 behind cached keys (prefill_chunk): RoPE of q and k at those positions + both cache
            # writes, then flash-style attention of the chunk's queries over the cache rows kv_start[t] .. their own position.  With the switch
            # off the chunk takes the branches below (S > 1: rope + SDPA over the [T, 1, S, Lc] mask; S == 1: the decode launch at pos_idx)
            q0, kvs = cache["chunk"]
            nq, nk = heads * hd, kvh * hd
            if ck.is_contiguous() and cv.is_contiguous():
                ops.rope_kv_append_(qkv, self.cos, self.sin, ck, cv, heads, kvh, q0)
            else:
                ops.rope_(qkv[..., :nq + nk], self.cos, self.sin, heads + kvh, S, q0)
                ck[:, :, q0:q0 + S] = qkv[..., nq:nq + nk].view(T, S, kvh, hd).transpose(1, 2)
                cv[:, :, q0:q0 + S] = qkv[..., nq + nk:].view(T, S, kvh, hd).transpose(1, 2)
            a = ops.prefill_attention_cached(qkv[..., :nq].view(T, S, heads, hd), ck, cv, q0, kv_start=kvs)
        elif S == 1 and self.fast_glue and ops.decode_attention_supported(heads, kvh, hd):
            # decode: RoPE + cache append + attention over the valid keys in ONE launch (pos_idx is a one-element device tensor)
            a = ops.decode_attention(qkv, self.cos, self.sin, ck, cv, cache["valid"], pos_idx, heads, kvh)
        elif (S > 1 and self.fast_glue and cache.get("kv_start") is not None and hd == 128 and S % 64 == 0 and qkv.is_contiguous()
              and not layer.qkv.interleave8):
            # prefill from position 0: in-place RoPE on the q and k slices of the fused projection output, flash-style attention over the
            # left-padded prompts (keys kv_start[t] .. query position), then the K / V rows go into the cache
            nq, nk = heads * hd, kvh * hd
            qf, kf, vf = qkv[..., :nq], qkv[..., nq:nq + nk], qkv[..., nq + nk:]
            k4, v4 = kf.view(T, S, kvh, hd), vf.view(T, S, kvh, hd)
            if short and ck.is_contiguous() and cv.is_contiguous():
                ops.rope_kv_append_(qkv, self.cos, self.sin, ck, cv, heads, kvh, 0)       # RoPE of q and k + both cache writes: one launch
                a = ops.prefill_attention(qf.view(T, S, heads, hd), k4, v4, kv_start=cache["kv_start"], causal=True)
            else:
                ops.rope_(qkv[..., :nq + nk], self.cos, self.sin, heads + kvh, S, 0)      # q and k heads: one launch
                a = ops.prefill_attention(qf.view(T, S, heads, hd), k4, v4, kv_start=cache["kv_start"], causal=True)
                ck[:, :, :S] = k4.transpose(1, 2)
                cv[:, :, :S] = v4.transpose(1, 2)
        else:
            q, k, v = layer.qkv.split(qkv)
            if cos is None:                                                     # (forward() skips the gather when it expects the HIP attention)
                cos, sin = self._rope_rows(pos_idx)
            q = _rope(q.view(T, S, heads, hd).transpose(1, 2), cos, sin)
            k = _rope(k.view(T, S, kvh, hd).transpose(1, 2), cos, sin)
            v = v.view(T, S, kvh, hd).transpose(1, 2)
            ck.index_copy_(2, pos_idx, k)
            cv.index_copy_(2, pos_idx, v)
            a = F.scaled_dot_product_attention(q, ck, cv, attn_mask=attn_mask, enable_gqa=(kvh != heads))
            a = a.transpose(1, 2).reshape(T, S, heads * hd)
        if pf is not None:
            torch.cuda.current_stream(x.device).wait_stream(pf)           # join before the o projection
        o_hand = handoff and layer.o.handoff_producer_ok(a) and layer.gate_up.handoff_consumer_ok(x, swiglu=True)
        n2h, s2 = self._hn(layer, "norm2") if o_hand else (None, 1.0)
        h2 = None
        if pairs and layer.o.residual_norm_ok(a, x):
            x, h2 = layer.o.forward_residual_norm(a, x, layer.norm2, self.eps)    # o + residual, norm2 on its split-k reduce launch
        else:
            x = layer.o(a, residual=x, ssq_out=self._ssq if o_hand else None, next_norm=n2h, xw_out=self._xw if o_hand else None,
                        ssq_scale=1.0 / (s2 * s2))
        if h2 is not None:
            if self.swiglu_epilogue and layer.gate_up.swiglu_ok(h2):
                act = layer.gate_up.forward_swiglu(h2)                            # gate|up -> SwiGLU in the pair tile's epilogue (A/B: slower)
            else:
                act = ops.swiglu_interleaved8(layer.gate_up(h2)) if layer.gate_up.interleave8 else ops.swiglu(layer.gate_up(h2), inter)
        elif o_hand:
            act = layer.gate_up.forward_fused(self._xw, None, self.eps / (s2 * s2), swiglu=True, ssq_in=self._ssq)   # (RMSNorm by hand-off) gate|up -> SwiGLU
        elif fuse and self.fuse_gateup_norm and layer.gate_up.fusable(x, swiglu=True):
            act = layer.gate_up.forward_fused(x, layer.norm2, self.eps, swiglu=True)   # RMSNorm -> gate|up -> SwiGLU: one launch
        elif fuse and layer.gate_up.interleave8 and layer.gate_up._decode_ok(x):
            act = layer.gate_up.forward_fused(self._norm(x, layer.norm2), None, self.eps, swiglu=True)   # gate|up -> SwiGLU: one launch
        elif self.fast_glue and self.swiglu_epilogue and S >= 256 and layer.gate_up.swiglu_ok(x):
            act = layer.gate_up.forward_swiglu(self._norm(x, layer.norm2))       # prefill: gate|up -> SwiGLU in the GEMM's epilogue (A/B)
        else:
            gu = layer.gate_up(self._norm(x, layer.norm2))
            if self.fast_glue and inter % 8 == 0 and (S <= 16 or layer.gate_up.interleave8):
                # one elementwise pass on the projection output (any prompt length when the rows are interleaved in blocks of 8)
                act = ops.swiglu_interleaved8(gu) if layer.gate_up.interleave8 else ops.swiglu(gu, inter)
            else:
                g, u = layer.gate_up.split(gu)
                act = F.silu(g) * u
        d_hand = handoff and next_layer is not None and layer.down.handoff_producer_ok(act) and layer.qkv.handoff_consumer_ok(x)
        n1h, s1n = self._hn(next_layer, "norm1") if d_hand else (None, 1.0)
        if h2 is not None and next_layer is not None and layer.down.residual_norm_ok(act, x):
            x, h_next = layer.down.forward_residual_norm(act, x, next_layer.norm1, self.eps)   # down + residual, the NEXT layer's norm1 on its reduce
            return x, False, h_next
        x = layer.down(act, residual=x, ssq_out=self._ssq if d_hand else None, next_norm=n1h, xw_out=self._xw if d_hand else None,
                       ssq_scale=1.0 / (s1n * s1n))
        return x, d_hand, None

    @torch.no_grad()
    def forward(self, ids, pos_idx, cache, attn_mask, x=None, ragged=None):
        """ids [T, S]; pos_idx [S] (device, positions of these tokens in the cache); attn_mask [T, 1, S, L] bool.
        Returns the logits of the LAST position, [T, vocab].  x: the embedded tokens when the caller already has them (step_begin).
        ragged=(pos [T], active [T]): one decode token per tenant, each at its own position (TenantSession); pos_idx and attn_mask are unused."""
        x = self._hidden(ids, pos_idx, cache, attn_mask, x=x, ragged=ragged)
        last = self._norm(x[:, -1:, :], self.final_norm)
        return tenant_linear(last, self.lm_head)[:, 0, :]                     # per-tenant lm_head: one launch

    def _hidden(self, ids, pos_idx, cache, attn_mask, x=None, ragged=None):
        """forward's layers: the residual stream after the last layer, [T, S, hidden], before the final norm (every row: score reads them)"""
        T, S = ids.shape
        _, _, _, heads, kvh, _ = self.cfg
        assert ragged is None or S == 1
        # (the rows of the rotary tables are gathered only for the stock-op attention paths: the HIP kernels index the tables themselves)
        hip_attn = self.fast_glue and ((S == 1 and ops.decode_attention_supported(heads, kvh, self.hd)) or
                                       (S > 1 and cache.get("kv_start") is not None and self.hd == 128 and S % 64 == 0) or
                                       (cache.get("chunk") is not None and self.hip_prefill_attention and self.hd == 128))
        cos, sin = (None, None) if (hip_attn or ragged is not None) else self._rope_rows(pos_idx)
        if x is None:
            t_idx = torch.arange(T, device=ids.device).view(T, 1)
            x = self.embed[t_idx, ids]                                        # per-tenant embedding: one gather
        ssq_valid = False                                                     # (the embedding rows have no producer launch: layer 0 norms itself)
        h_in = None
        for li, layer in enumerate(self.layers):
            nxt = self.layers[li + 1] if li + 1 < len(self.layers) else None
            x, ssq_valid, h_in = self._layer(layer, x, cos, sin, cache, li, pos_idx, attn_mask, ssq_valid, nxt, h_in, ragged=ragged)
        return x

    # ---------------------------------------------------------------- request handling (demo_backend.py:261-315 + :190-258)
    def prepare(self, prompts):
        """Left-pad T prompts with token 0 to a power of two >= 64; returns (ids [T, L], attention mask [T, L]) on the device."""
        assert len(prompts) == self.T, "one prompt per tenant (batch row t is tenant t)"
        longest = max(len(p) for p in prompts)
        L = padded_length(longest)
        if L > MAX_PROMPT:
            raise ValueError("max_len too large, please reduce the input length")      # the reference's refusal, as an exception
        ids = torch.zeros(self.T, L, dtype=torch.long)
        am = torch.zeros(self.T, L, dtype=torch.bool)
        for t, p in enumerate(prompts):
            ids[t, L - len(p):] = torch.tensor(p, dtype=torch.long)
            am[t, L - len(p):] = True
        return ids.to(self.dev), am.to(self.dev)

    @torch.no_grad()
    def prefill(self, ids, attention_mask, cache, hidden=False):
        """hidden=True: every row of the residual stream after the last layer ([T, L, hidden], _hidden) instead of the last row's logits"""
        T, L = ids.shape
        pos_idx = torch.arange(L, device=self.dev)
        cache["valid"].zero_()
        cache["valid"][:, :L] = attention_mask
        Lc = cache["k"][0].shape[2]
        causal = torch.ones(L, Lc, dtype=torch.bool, device=self.dev).tril()                     # query i sees keys <= i
        mask = causal[None, None] & cache["valid"][:, None, None, :]
        # fully masked query rows (left pads) would be NaN in softmax: let a pad see itself; its output is never used
        mask = mask | torch.eye(L, Lc, dtype=torch.bool, device=self.dev)[None, None]
        # left-padded prompts (prepare() builds them so): the HIP prefill attention takes the first valid key of each tenant instead of
        # the [T, 1, L, Lc] mask; any other mask shape keeps the torch attention
        am = attention_mask.bool()
        left_padded = bool((am[:, 1:] | ~am[:, :-1]).all()) if L > 1 else True
        cache["kv_start"] = (L - am.sum(dim=1)).to(torch.int32) if (left_padded and self.hip_prefill_attention) else None
        try:
            return (self._hidden if hidden else self.forward)(ids, pos_idx, cache, mask)
        finally:
            cache["kv_start"] = None

    # ---------------------------------------------------------------- scoring (eval_ppl.py:61-83, for T fine-tunes in one pass over the base)
    def _score_args(self, seqs, targets_from):
        """score's argument checks, all on the host and before any launch: (token lists, first scored index per tenant, padded length)"""
        if torch.is_tensor(seqs):
            if seqs.dim() != 2 or seqs.dtype != torch.long:
                raise ValueError("a tensor of sequences is a [T, n] LongTensor")
            seqs = seqs.tolist()
        seqs = [[int(v) for v in s] for s in seqs]
        if len(seqs) != self.T:
            raise ValueError("one sequence per tenant: got %d for %d tenants" % (len(seqs), self.T))
        vocab = self.cfg[5]
        for s in seqs:
            if len(s) < 2:
                raise ValueError("a sequence needs at least 2 tokens to score one")
            if min(s) < 0 or max(s) >= vocab:
                raise ValueError("token id outside the vocabulary of %d" % vocab)
        if isinstance(targets_from, (list, tuple)):
            if len(targets_from) != self.T:
                raise ValueError("targets_from: one int, or one per tenant")
            first = [operator.index(v) for v in targets_from]
        else:
            first = [operator.index(targets_from)] * self.T
        if min(first) < 0:
            raise ValueError("targets_from is an index into the sequence: >= 0")
        L = -(-max(len(s) for s in seqs) // MIN_PAD) * MIN_PAD
        if L > self.max_len:
            raise ValueError("the sequences pad to %d tokens, beyond this decoder's max_len of %d" % (L, self.max_len))
        return seqs, [max(1, f) for f in first], L

    @torch.no_grad()
    def score(self, seqs, targets_from=0, row_chunk=512, hip_nll=True):
        """Teacher-forced token losses of T sequences, one per tenant (lengths >= 2, may differ; or a [T, n] LongTensor): a list of T float32
        device tensors, entry i of tensor t = -log p_t(seq_t[i] | seq_t[:i]) for i >= max(1, targets_from[t]) and exactly 0 before it.
        targets_from: an int, or one per tenant.  The sequences are left-padded with token 0 to a common multiple of 64 (prepare()'s power of two
        and MAX_PROMPT are the demo's request rules, not scoring's) and run through the batched prefill on a scratch KV cache of that length: the
        decoder's own cache, its captured graphs and live sessions are not touched.  Only the rows that predict a scored token go through the
        final norm and the lm_head, row_chunk rows per tenant at a time (torch.bmm: an M > 16 per-tenant Linear is the BLAS's), each chunk
        through serving_ops.token_nll -- the [T, L, vocab] logits never exist.  hip_nll=False: the stock tail, log_softmax(chunk.float()) + gather."""
        seqs, first, L = self._score_args(seqs, targets_from)
        row_chunk = operator.index(row_chunk)
        if row_chunk < 1:
            raise ValueError("row_chunk >= 1")
        T = self.T
        ids = torch.zeros(T, L, dtype=torch.long)
        am = torch.zeros(T, L, dtype=torch.bool)
        counts = [max(len(s) - f, 0) for s, f in zip(seqs, first)]           # scored tokens per tenant
        M = max(max(counts), 1)
        # row j of tenant t predicts the token at padded column rows[t, j] + 1.  Tenants with fewer scored tokens are filled with the last row and
        # the ignore label: those entries land in a spare column L of the result and are exactly 0
        rows = torch.full((T, M), L - 1, dtype=torch.long)
        labels = torch.full((T, M), -100, dtype=torch.long)
        for t, (s, f, c) in enumerate(zip(seqs, first, counts)):
            pad = L - len(s)
            ids[t, pad:] = torch.tensor(s, dtype=torch.long)
            am[t, pad:] = True
            if c:
                rows[t, :c] = torch.arange(pad + f - 1, L - 1)
                labels[t, :c] = ids[t, pad + f:]
        ids, am, rows, labels = ids.to(self.dev), am.to(self.dev), rows.to(self.dev), labels.to(self.dev)
        x = self.prefill(ids, am, self.new_cache(L), hidden=True)
        t_idx = torch.arange(T, device=self.dev).view(T, 1)
        h = self._norm(x[t_idx, rows], self.final_norm)                      # [T, M, hidden]: the predicting rows only
        head_t = self.lm_head.transpose(1, 2)
        vocab = self.lm_head.shape[1]
        out = torch.zeros(T, L + 1, dtype=torch.float32, device=self.dev)
        for c0 in range(0, M, row_chunk):
            c1 = min(c0 + row_chunk, M)
            logits = torch.bmm(h[:, c0:c1], head_t)                          # [T, c, vocab]
            lab = labels[:, c0:c1].reshape(-1)
            if hip_nll:
                nll = ops.token_nll(logits.view(-1, vocab), lab)
            else:
                lp = F.log_softmax(logits.view(-1, vocab).float(), dim=-1)
                keep = lab >= 0
                nll = torch.where(keep, -lp.gather(1, lab.clamp(min=0)[:, None])[:, 0], torch.zeros((), device=self.dev))
            out[t_idx, rows[:, c0:c1] + 1] = nll.view(T, c1 - c0)
        return [out[t, L - len(s):L] for t, s in enumerate(seqs)]

    @torch.no_grad()
    def prefill_chunk(self, ids, q0, cache, kv_start=None):
        """Prefill ids [T, n] (n >= 1, any value) at positions q0 .. q0 + n - 1 BEHIND the keys already in the cache -- the next turn of a
        conversation whose rows 0 .. q0 - 1 are cached, where the reference re-prefills the whole history (demo/demo_backend.py:261-315).
        Marks valid[:, q0 : q0 + n], writes those cache rows and returns the last row's logits [T, vocab].  kv_start: int32 [T] device tensor,
        each tenant's first valid key (its left pads; None = 0).  hip_prefill_attention picks the arm: bd_srv_prefill_attention_cached, or the
        stock ops (rope + SDPA over a [T, 1, n, Lc] mask made of the validity bytes)."""
        T, n = ids.shape
        q0 = int(q0)
        Lc = cache["k"][0].shape[2]
        if not (n >= 1 and 0 <= q0 and q0 + n <= Lc):
            raise ValueError("the chunk's rows %d .. %d do not lie in the KV cache (%d rows)" % (q0, q0 + n - 1, Lc))
        pos_idx = torch.arange(q0, q0 + n, device=self.dev)
        cache["valid"][:, q0:q0 + n] = True
        seen = torch.arange(Lc, device=self.dev)[None, :] <= pos_idx[:, None]                    # query i sees keys <= q0 + i
        mask = seen[None, None] & cache["valid"][:, None, None, :]
        cache["chunk"] = (q0, kv_start)
        try:
            return self.forward(ids, pos_idx, cache, mask)
        finally:
            cache["chunk"] = None

    def _decode_step(self, st):
        """one greedy step on static buffers: st['tok'] [T,1] -> logits -> argmax -> st['tok']; position / masks advance on device"""
        cache = st["cache"]
        if self.fast_glue and self.step_kernels and self.embed.shape[-1] % 8 == 0 and self.lm_head.shape[-2] % 8 == 0:
            # the two ends of the step as ONE launch each (serving_ops.step_begin / step_end): mask extension + embedding, then argmax + the
            # token / output / stop-flag / position updates
            if "ticket" not in st:
                st["ticket"] = torch.zeros(1, dtype=torch.int32, device=self.dev)      # (first call = outside any graph capture)
            x = ops.step_begin(self.embed, st["tok"], cache["valid"], st["pos"])
            logits = self.forward(st["tok"], st["pos"], cache, cache["valid"][:, None, None, :], x=x)
            if logits.stride(1) == 1 and logits.stride(0) % 8 == 0 and logits.data_ptr() % 16 == 0:
                ops.step_end(logits, st["tok"], st["out"], st["step"], st["pos"], st["stop_ids"], st["stopped"], st["ticket"])
                return
        else:
            cache["valid"].index_fill_(1, st["pos"], True)
            mask = cache["valid"][:, None, None, :]
            logits = self.forward(st["tok"], st["pos"], cache, mask)
        nxt = torch.argmax(logits, dim=-1)
        st["tok"].copy_(nxt[:, None])
        st["out"].index_copy_(1, st["step"], nxt[:, None])
        st["stopped"] |= (nxt[:, None] == st["stop_ids"]).any(dim=1)
        st["pos"] += 1
        st["step"] += 1

    @torch.no_grad()
    def generate(self, prompts, max_new_tokens=16, stop_token_ids=None, use_graph=True, check_every=1):
        """Greedy decoding of T prompts (one per tenant).  Returns (new_tokens [T, n] on the CPU, n_steps).
        stop_token_ids: per-tenant lists of token ids; generation ends when every tenant has produced one (or at max_new_tokens),
        exactly like the reference's loop; tokens after a tenant's stop token are still generated (the reference does the same and
        hides them in its response formatting)."""
        ids, am = self.prepare(prompts)
        T, L = ids.shape
        assert L + max_new_tokens <= self.max_len
        nstop = max((len(s) for s in stop_token_ids), default=0) if stop_token_ids else 0
        # Static request state, reused by every generate() call: ONE KV cache per decoder (it does not depend on the request), feedback
        # buffers sized to fixed maxima (`out` holds max_len tokens, the stop table MIN_STOP_WIDTH ids or the next power of two), so
        # the captured hipGraph of the decode step is keyed by the stop-table width and the glue switches only -- not by caller-chosen
        # max_new_tokens (every new key used to allocate a full KV cache + a graph and nothing was ever evicted).  The
        # few slots that can exist are kept in a small LRU; an evicted slot's graph and buffers are released.
        # Stale keys of an earlier request are masked by cache["valid"].
        width = max(self.MIN_STOP_WIDTH, 1 << max(nstop - 1, 0).bit_length())
        key = (width, self.fast_glue, self.fuse_glue, self.fuse_qkv_norm, self.fuse_gateup_norm, self.norm_handoff, FusedDeltaLinear.use_tiled,
               self.prefetch_o, self.step_kernels)
        if self._kv_cache is None:
            self._kv_cache = self.new_cache()
        slot = self._static.pop(key, None)
        if slot is None:
            slot = {"st": {
                "cache": self._kv_cache, "tok": torch.zeros(T, 1, dtype=torch.long, device=self.dev),
                "pos": torch.zeros(1, dtype=torch.long, device=self.dev), "step": torch.zeros(1, dtype=torch.long, device=self.dev),
                "stop_ids": torch.full((T, width), -1, dtype=torch.long, device=self.dev),
                "out": torch.zeros(T, self.max_len + 1, dtype=torch.long, device=self.dev),
                "stopped": torch.zeros(T, dtype=torch.bool, device=self.dev)}, "graph": None}
        self._static[key] = slot                              # (re-)inserted last: dict order is the LRU order
        while len(self._static) > self.MAX_STATIC_SLOTS:
            old = self._static.pop(next(iter(self._static)))
            old["graph"] = None                               # drops the captured graph (and with it the references to the buffers)
            old["st"].clear()
        st = slot["st"]
        cache = st["cache"]
        logits = self.prefill(ids, am, cache)
        st["stop_ids"].fill_(-1)
        if stop_token_ids:
            for t, s_ in enumerate(stop_token_ids):
                if len(s_):
                    st["stop_ids"][t, :len(s_)] = torch.tensor(sorted(s_), dtype=torch.long, device=self.dev)
        first = torch.argmax(logits, dim=-1)
        st["tok"].copy_(first[:, None])
        st["pos"].fill_(L)
        st["step"].fill_(1)
        st["out"].zero_()
        st["out"][:, 0] = first
        st["stopped"].copy_((first[:, None] == st["stop_ids"]).any(dim=1))
        n = 1
        if use_graph and max_new_tokens > 1:
            if slot["graph"] is None:
                slot["graph"] = self._graph_runner(st)
            runner = slot["graph"]
        else:
            runner = lambda: self._decode_step(st)
        while n < max_new_tokens:
            if (n - 1) % check_every == 0 and bool(st["stopped"].all()):
                break
            runner()
            n += 1
        return st["out"][:, :n].cpu(), n

    # ---------------------------------------------------------------- per-tenant requests
    _SWITCHES = ("fast_glue", "swiglu_epilogue", "short_prompt_fusions", "hip_prefill_attention", "fuse_glue")

    def tenant_view(self, t):
        """A one-tenant TenantDecoder over tenant t's slices of THIS decoder's tensors -- sign words, scales, embedding, norms, lm_head; the base
        weights whole -- for prefilling one tenant alone.  Nothing is copied: every tensor of the view is the parent's storage, offset by the
        tenant.  It carries no decode copies (packed sign words, tile-major weights): it is a prefill-only user."""
        assert 0 <= t < self.T
        views = self._tenant_views
        v = views.get(t)
        if v is None:
            v = TenantDecoder(self.cfg, 1, self.dev, self.dtype, max_len=self.max_len, eps=self.eps, base_int8=self.base_int8, base_gptq4=self.base_gptq4,
                              rope=self._rope[t])
            # the parent's table, or the tenant's rows of it: a slice of the storage load_tenant(rope=) rewrites in place
            v.cos, v.sin = (self.cos[t], self.sin[t]) if self.rope_per_tenant else (self.cos, self.sin)
            for layer in self.layers:
                lv = nn.Module()
                for name in ("qkv", "o", "gate_up", "down"):
                    setattr(lv, name, getattr(layer, name).tenant_view(t))
                lv.norm1, lv.norm2 = layer.norm1[t:t + 1], layer.norm2[t:t + 1]
                v.layers.append(lv)
            v.embed, v.final_norm, v.lm_head = self.embed[t:t + 1], self.final_norm[t:t + 1], self.lm_head[t:t + 1]
            views[t] = v
        for name in self._SWITCHES:
            setattr(v, name, getattr(self, name))
        return v

    def cache_view(self, cache, t):
        """tenant t's slices of a KV cache of this decoder (views, no copy): what tenant_view(t) prefills into"""
        return {"k": [k[t:t + 1] for k in cache["k"]], "v": [v[t:t + 1] for v in cache["v"]], "valid": cache["valid"][t:t + 1]}

    def session(self, max_stop_ids=8, sampling=False, logprobs=None, penalties=False, max_logit_bias=16, constraints=False,
                max_constraint_states=256, max_constraint_edges=4096, stop_sequences=False, max_stop_sequences=4, max_stop_sequence_len=8, bans=False, max_bad_words=16,
                max_bad_word_len=8, truncation=False):
        """A TenantSession on this decoder's KV cache: per-tenant admission and retirement around the same decode step.  sampling=True: every
        request carries its own temperature / top_k / top_p / seed (TenantSession); the default session is greedy and takes none of them.
        logprobs=k (0 .. 20): the session also keeps every emitted token's log-probability and its k most probable alternatives
        (TenantSession.result_logprobs); None, the default, keeps nothing and adds no launch.
        penalties=True: every request also carries repetition_penalty / presence_penalty / frequency_penalty / logit_bias (penalty_params; at
        most max_logit_bias <= 64 bias entries per request); independent of sampling and logprobs.  The default session takes none of them,
        allocates nothing for them and runs the step it ran before.
        constraints=True: every request may also carry constraint= a TokenAutomaton (constraint.py) of at most max_constraint_states states and
        max_constraint_edges edges, which restricts what the request may emit; independent of the other three.  The default session refuses
        one, allocates nothing for it and runs the step it ran before.
        stop_sequences=True: every request may also carry stop_sequences= a list of token-id lists (at most max_stop_sequences <= 16 of at most
        max_stop_sequence_len <= 32 ids each) and retires, with reason 16, in the step that completes one of them (TenantSession.stop_match,
        streamable); independent of the other four.  The default session refuses them, allocates nothing for them and runs the step it ran
        before.
        bans=True: every request may also carry no_repeat_ngram_size= / bad_words= / min_new_tokens= (ban_params; at most max_bad_words <= 64
        sequences of at most max_bad_word_len <= 32 ids each): tokens its own history forbids are never chosen; independent of the other
        five.  The default session refuses them, allocates nothing for them and runs the step it ran before.
        truncation=True (needs sampling=True, ValueError otherwise): every request may also carry min_p= / typical_p= / epsilon_cutoff= /
        eta_cutoff= (truncation_params): the tail of its distribution is cut by the row's own statistics before top-k / top-p.  The default
        session refuses them, allocates nothing for them and runs the step it ran before."""
        return TenantSession(self, max_stop_ids, sampling=sampling, logprobs=logprobs, penalties=penalties, max_logit_bias=max_logit_bias,
                             constraints=constraints, max_constraint_states=max_constraint_states, max_constraint_edges=max_constraint_edges,
                             stop_sequences=stop_sequences, max_stop_sequences=max_stop_sequences, max_stop_sequence_len=max_stop_sequence_len,
                             bans=bans, max_bad_words=max_bad_words, max_bad_word_len=max_bad_word_len, truncation=truncation)

    def _graph_runner(self, st):
        """Capture one decode step as a hipGraph on the request's static buffers and return a replay callable.  The launch-bound
        step (4 Linear launches + ~20 small torch ops per layer) replays without per-op host overhead."""
        # ONE capture stream per decoder: the library's scratch is keyed by (device, stream), so the warm-up step below allocates it on
        # the very stream the capture then runs on (nothing is allocated or memset inside the graph), and later captures reuse it
        if self._capture_stream is None:
            self._capture_stream = torch.cuda.Stream(device=self.dev)
        side = self._capture_stream
        snap = {k: v.clone() for k, v in st.items() if torch.is_tensor(v)}
        snap_valid = st["cache"]["valid"].clone()
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):                     # warm-up outside capture (allocations, workspace, lazy init)
            self._decode_step(st)
        torch.cuda.current_stream(self.dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            self._decode_step(st)
        torch.cuda.synchronize(self.dev)
        for k, v in snap.items():                         # undo the two trial steps: replay starts from the request's real state
            st[k].copy_(v)
        st["cache"]["valid"].copy_(snap_valid)
        return g.replay


def extend_plan(pos, kv_start, done, n_tokens, Lc, active=False):
    """Geometry and refusals of TenantSession.extend, host integers only: a retired tenant at position `pos` (its cache rows hold the conversation
    up to, not including, its last emitted token) whose conversation starts at row kv_start (the left pads of its first prompt; None = never
    submitted, or its fine-tune was replaced since) takes n_tokens more tokens.  Returns (P, n): the chunk [last emitted token] + tokens has
    n = 1 + n_tokens rows and goes to cache rows P .. P + n - 1.  Raises, in this order: RuntimeError for an active tenant, for one without a
    cached conversation, and for one whose cache rows are full (done & 4); ValueError when the chunk does not fit the Lc cache rows, and when the
    conversation's real length, padded as a request of that length would be, passes MAX_PROMPT (the reference's refusal)."""
    if active:
        raise RuntimeError("the tenant is still generating")
    if kv_start is None:
        raise RuntimeError("the tenant has no cached conversation to extend (never submitted, or its fine-tune was replaced)")
    if int(done) & 4:
        raise RuntimeError("the tenant's cache rows are full")
    P, n = int(pos), 1 + int(n_tokens)
    if not (0 <= int(kv_start) <= P and n_tokens >= 0):
        raise ValueError("position %d / first key %d / %d new tokens: not a conversation's state" % (P, kv_start, n_tokens))
    if P + n > Lc:
        raise ValueError("the conversation does not fit the KV cache")
    if padded_length(P - int(kv_start) + n) > MAX_PROMPT:
        raise ValueError("max_len too large, please reduce the input length")
    return P, n


def sampling_params(temperature=0.0, top_k=0, top_p=1.0, seed=0):
    """The sampling parameters of one request, validated on the host: (temperature, top_k, top_p, seed) as (float, int, float, int).
    temperature: finite and >= 0 (0 = greedy); top_k: an integer >= 0 (0 = off); top_p: 0 < top_p <= 1 (1 = off); seed: an integer in
    [0, 2^64).  Anything else raises ValueError.  The defaults are greedy decoding."""
    def integer(v, what):
        try:
            if isinstance(v, bool):
                raise TypeError
            return operator.index(v)
        except TypeError:
            raise ValueError("%s = %r: an integer is required" % (what, v))
    try:
        tau, p = float(temperature), float(top_p)
    except (TypeError, ValueError):
        raise ValueError("temperature = %r, top_p = %r: numbers are required" % (temperature, top_p))
    if not (math.isfinite(tau) and tau >= 0.0):
        raise ValueError("temperature = %r: a finite value >= 0 is required (0 = greedy)" % (temperature,))
    k = integer(top_k, "top_k")
    if k < 0:
        raise ValueError("top_k = %r: an integer >= 0 is required (0 = off)" % (top_k,))
    if not (0.0 < p <= 1.0):
        raise ValueError("top_p = %r: 0 < top_p <= 1 is required (1 = off)" % (top_p,))
    s_ = integer(seed, "seed")
    if not (0 <= s_ < 1 << 64):
        raise ValueError("seed = %r: 0 <= seed < 2^64 is required" % (seed,))
    return tau, k, p, s_


GREEDY = sampling_params()


def penalty_params(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, *, vocab=None,
                   max_logit_bias=ops.LOGIT_BIAS_MAX):
    """The penalty parameters of one request, validated on the host: (repetition_penalty, presence_penalty, frequency_penalty, bias) as
    (float, float, float, ((id, value), ...)) with the bias sorted by id -- the canonical form: two requests that mean the same compare equal.
    repetition_penalty: finite and > 0 (1 = off; HF's rule); presence_penalty / frequency_penalty: finite (0 = off; OpenAI's rule on the tokens
    generated in this turn); logit_bias: None or a mapping {token id: value} -- integer ids (no bools) in [0, vocab) when the vocabulary size is
    given, values finite with |value| <= 100, or -inf (the token is banned), at most max_logit_bias entries.  Anything else raises ValueError.
    The defaults change nothing (NEUTRAL)."""
    try:
        r, pres, freq = float(repetition_penalty), float(presence_penalty), float(frequency_penalty)
    except (TypeError, ValueError):
        raise ValueError("repetition_penalty = %r, presence_penalty = %r, frequency_penalty = %r: numbers are required"
                         % (repetition_penalty, presence_penalty, frequency_penalty))
    if any(isinstance(v, bool) for v in (repetition_penalty, presence_penalty, frequency_penalty)):
        raise ValueError("a penalty is a number, not a bool")
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError("repetition_penalty = %r: a finite value > 0 is required (1 = off)" % (repetition_penalty,))
    if not (math.isfinite(pres) and math.isfinite(freq)):
        raise ValueError("presence_penalty = %r, frequency_penalty = %r: finite values are required (0 = off)"
                         % (presence_penalty, frequency_penalty))
    bias = []
    if logit_bias is not None:
        if not isinstance(logit_bias, collections.abc.Mapping):
            raise ValueError("logit_bias = %r: a mapping {token id: value} is required" % (logit_bias,))
        if len(logit_bias) > max_logit_bias:
            raise ValueError("logit_bias holds %d entries: at most %d are kept per request" % (len(logit_bias), max_logit_bias))
        for k, v in logit_bias.items():
            try:
                if isinstance(k, bool) or isinstance(v, bool):
                    raise TypeError
                i, b = operator.index(k), float(v)
            except (TypeError, ValueError):
                raise ValueError("logit_bias[%r] = %r: an integer token id and a number are required" % (k, v))
            if i < 0 or (vocab is not None and i >= vocab):
                raise ValueError("logit_bias: token id %d is outside the vocabulary" % i)
            if not (b == -math.inf or (math.isfinite(b) and abs(b) <= 100.0)):
                raise ValueError("logit_bias[%d] = %r: a finite value with |value| <= 100, or -inf (a ban), is required" % (i, v))
            bias.append((i, b))
        bias.sort()
    return r, pres, freq, tuple(bias)


NEUTRAL = penalty_params()


def penalty_row(pp):
    """the four floats the kernel reads for penalty_params' tuple pp: (r, float32(1 / r) from the fp64 quotient, presence, frequency)"""
    return [pp[0], 1.0 / pp[0], pp[1], pp[2]]


def fold_history(hist):
    """TenantSession.extend's fold of a history row (int16, any shape; a new tensor): every non-zero element becomes bit 15 alone.  What the
    earlier turns held or generated is context of the next turn, and the counts restart with the turn, as result() does -- the history a submit
    of the whole conversation would have written."""
    return torch.where(hist != 0, torch.full_like(hist, -32768), torch.zeros_like(hist))


def logprobs_count(logprobs):
    """The logprobs= argument of a session, validated on the host: None (nothing is kept) or an integer 0 <= k <= 20 (0: the chosen token's
    log-probability only; k: the k most probable alternatives with it).  A bool, a non-integer or a value outside the range raises ValueError."""
    if logprobs is None:
        return None
    try:
        if isinstance(logprobs, bool):
            raise TypeError
        k = operator.index(logprobs)
    except TypeError:
        raise ValueError("logprobs = %r: None or an integer is required" % (logprobs,))
    if not (0 <= k <= ops.LOGPROBS_MAX):
        raise ValueError("logprobs = %r: 0 <= logprobs <= %d is required" % (logprobs, ops.LOGPROBS_MAX))
    return k


def logprobs_slot(n, lp_n, cap):
    """serving_ops.step_logprobs' rule for one tenant on host integers: its token count n against the launch's own counter lp_n and the cap entries
    of its buffers.  Returns (j, lp_n'): the entry written (None: nothing) and the counter afterwards.  A tenant whose count did not move is not
    touched; otherwise the entry is that of the token just stored at out[t, n - 1], kept when it lies inside the buffers, and the counter follows
    n -- so the entries 0 .. min(n, cap) - 1 that result_logprobs reports are exactly the ones written, entry j with token j."""
    if n == lp_n:
        return None, lp_n
    j = n - 1
    return (j if 0 <= j < cap else None), n


def stop_sequence_table(seqs, Q, W, vocab=None):
    """The stop sequences of one request, validated on the host, as the rows the device table takes: (tok, lens) with tok Q lists of W ints --
    sequence q in tok[q][:lens[q]], padded with -1 -- and lens Q ints, 0 for an unused slot.  The caller's order is kept: hit is an index into
    it.  seqs: None or a list / tuple of token-id sequences (lists / tuples), each of 1 .. W integer ids (no bools) in [0, vocab) when the
    vocabulary size is given, at most Q of them.  Anything else -- an empty sequence, an id that is no integer or lies outside the vocabulary,
    too many sequences, a sequence that is too long -- raises ValueError."""
    if seqs is None:
        seqs = ()
    if not isinstance(seqs, (list, tuple)):
        raise ValueError("stop_sequences = %r: a list of token-id lists is required" % (seqs,))
    if len(seqs) > Q:
        raise ValueError("%d stop sequences: at most %d are kept per request" % (len(seqs), Q))
    tok, lens = [], []
    for s_ in seqs:
        if not isinstance(s_, (list, tuple)):
            raise ValueError("stop sequence %r: a list of token ids is required" % (s_,))
        if len(s_) == 0:
            raise ValueError("an empty stop sequence")
        if len(s_) > W:
            raise ValueError("a stop sequence of %d tokens: at most %d are kept" % (len(s_), W))
        row = []
        for i in s_:
            try:
                if isinstance(i, bool):
                    raise TypeError
                i = operator.index(i)
            except TypeError:
                raise ValueError("stop sequence %r: integer token ids are required" % (s_,))
            if i < 0 or i > 2 ** 31 - 1 or (vocab is not None and i >= vocab):
                raise ValueError("stop sequence %r: token id %d is outside the vocabulary" % (s_, i))
            row.append(i)
        tok.append(row + [-1] * (W - len(row)))
        lens.append(len(row))
    pad = Q - len(tok)
    return tok + [[-1] * W for _ in range(pad)], lens + [0] * pad


def stop_sequence_scan(tokens, seqs):
    """include/bitdelta_hip.h's rule (bd_srv_step_stop_sequences) for one tenant on host integers: tokens = this turn's tokens so far (the prompt
    and earlier turns never take part), seqs = the request's sequences in the caller's order.  Returns (hit, hold): the lowest index of a
    sequence the tokens END with, or -1; and the largest k such that the last k tokens are the first k of a sequence longer than k -- the
    trailing tokens a streaming caller must not show yet -- which is 0 on a hit.  Admission uses it for the first token, which comes from the
    prefill and not from a step."""
    y, n = list(tokens), len(tokens)
    for q, s_ in enumerate(seqs):
        s_ = list(s_)
        if 1 <= len(s_) <= n and y[n - len(s_):] == s_:
            return q, 0
    hold = 0
    for s_ in seqs:
        s_ = list(s_)
        for k in range(min(len(s_) - 1, n), hold, -1):
            if y[n - k:] == s_[:k]:
                hold = k
                break
    return -1, hold


def ban_params(no_repeat_ngram_size=0, bad_words=(), min_new_tokens=0, *, vocab=None, max_bad_words=ops.BAN_WORDS_MAX,
               max_bad_word_len=ops.BAN_WORD_LEN_MAX):
    """The hard bans of one request, validated on the host: (no_repeat_ngram_size, bad_words, min_new_tokens) as (int, tuple of tuples of ints,
    int) -- the canonical form: two requests that mean the same compare equal.  include/bitdelta_hip.h (bd_srv_ban_rows) defines what they
    ban.  no_repeat_ngram_size: an integer 0 .. 8 (0 = off; HF's NoRepeatNGramLogitsProcessor); bad_words: None or a list / tuple of token-id
    sequences (lists / tuples), each of 1 .. max_bad_word_len integer ids in [0, vocab) when the vocabulary size is given, at most
    max_bad_words of them, kept in the caller's order (HF's bad_words_ids); min_new_tokens: an integer >= 0 (0 = off; HF's
    MinNewTokensLengthLogitsProcessor; values past 2^31 - 1 mean the same as that).  Anything else -- a bool or a non-integer where an integer is
    required, a negative size, an empty sequence, an id outside the vocabulary, too many or too long sequences -- raises ValueError.  The
    defaults ban nothing (NO_BANS)."""
    def integer(v, what):
        try:
            if isinstance(v, bool):
                raise TypeError
            return operator.index(v)
        except TypeError:
            raise ValueError("%s = %r: an integer is required" % (what, v))
    g = integer(no_repeat_ngram_size, "no_repeat_ngram_size")
    if not (0 <= g <= ops.BAN_NGRAM_MAX):
        raise ValueError("no_repeat_ngram_size = %r: an integer 0 .. %d is required (0 = off)" % (no_repeat_ngram_size, ops.BAN_NGRAM_MAX))
    lo = integer(min_new_tokens, "min_new_tokens")
    if lo < 0:
        raise ValueError("min_new_tokens = %r: an integer >= 0 is required (0 = off)" % (min_new_tokens,))
    if bad_words is None:
        bad_words = ()
    if not isinstance(bad_words, (list, tuple)):
        raise ValueError("bad_words = %r: a list of token-id lists is required" % (bad_words,))
    if len(bad_words) > max_bad_words:
        raise ValueError("%d bad words: at most %d are kept per request" % (len(bad_words), max_bad_words))
    words = []
    for w in bad_words:
        if not isinstance(w, (list, tuple)):
            raise ValueError("bad word %r: a list of token ids is required" % (w,))
        if len(w) == 0:
            raise ValueError("an empty bad word")
        if len(w) > max_bad_word_len:
            raise ValueError("a bad word of %d tokens: at most %d are kept" % (len(w), max_bad_word_len))
        row = []
        for i in w:
            i = integer(i, "bad word %r: token id" % (w,))
            if i < 0 or i > 2 ** 31 - 1 or (vocab is not None and i >= vocab):
                raise ValueError("bad word %r: token id %d is outside the vocabulary" % (w, i))
            row.append(i)
        words.append(tuple(row))
    return g, tuple(words), min(lo, 2 ** 31 - 1)


NO_BANS = ban_params()


def ban_word_table(words, Q, W):
    """ban_params' bad words as the rows the device table takes: (tok, lens) with tok Q lists of W ints -- word q in tok[q][:lens[q]], padded with
    -1 -- and lens Q ints, 0 for an unused slot.  ValueError when the words do not fit Q rows of W ids."""
    if len(words) > Q or any(not 1 <= len(w) <= W for w in words):
        raise ValueError("the bad words do not fit a table of %d words of %d ids" % (Q, W))
    pad = Q - len(words)
    return [list(w) + [-1] * (W - len(w)) for w in words] + [[-1] * W for _ in range(pad)], [len(w) for w in words] + [0] * pad


def truncation_params(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """The tail truncation of one request, validated on the host: (min_p, typical_p, epsilon_cutoff, eta_cutoff) as four floats -- the canonical
    form: two requests that mean the same compare equal.  include/bitdelta_hip.h (bd_srv_truncate_rows) defines what they drop.  min_p in
    [0, 1] (0 = off; HF's MinPLogitsWarper); typical_p in (0, 1] (1 = off; TypicalLogitsWarper); epsilon_cutoff in [0, 1) (0 = off;
    EpsilonLogitsWarper); eta_cutoff in [0, 1) (0 = off; EtaLogitsWarper).  Anything else -- a value outside its range, a NaN, an infinity, a
    bool or something that is no number -- raises ValueError.  The defaults drop nothing (NO_TRUNCATION)."""
    def number(v, what):
        try:
            if isinstance(v, bool):
                raise TypeError
            x = float(v)
        except (TypeError, ValueError):
            raise ValueError("%s = %r: a number is required" % (what, v))
        if not math.isfinite(x):
            raise ValueError("%s = %r: a finite value is required" % (what, v))
        return x + 0.0                                 # (-0.0 -> 0.0: one canonical zero)
    mp, ty = number(min_p, "min_p"), number(typical_p, "typical_p")
    ep, et = number(epsilon_cutoff, "epsilon_cutoff"), number(eta_cutoff, "eta_cutoff")
    if not (0.0 <= mp <= 1.0):
        raise ValueError("min_p = %r: 0 <= min_p <= 1 is required (0 = off)" % (min_p,))
    if not (0.0 < ty <= 1.0):
        raise ValueError("typical_p = %r: 0 < typical_p <= 1 is required (1 = off)" % (typical_p,))
    if not (0.0 <= ep < 1.0):
        raise ValueError("epsilon_cutoff = %r: 0 <= epsilon_cutoff < 1 is required (0 = off)" % (epsilon_cutoff,))
    if not (0.0 <= et < 1.0):
        raise ValueError("eta_cutoff = %r: 0 <= eta_cutoff < 1 is required (0 = off)" % (eta_cutoff,))
    return mp, ty, ep, et


NO_TRUNCATION = truncation_params()


class TenantSession:
    """Per-tenant requests on one TenantDecoder: a tenant is admitted when its request arrives (`submit`) and retires at its own stop token, its
    own max_new_tokens or the end of its cache rows, while the other tenants keep generating.  The decode step is the decoder's -- the same
    Linear launches over the same T rows -- with the three launches that knew a shared position replaced by their ragged forms
    (serving_ops.step_begin_ragged / decode_attention_ragged / step_end_ragged): every tenant has its own pos / n / limit / active / done on the
    device.  An inactive tenant's row runs through the step as zeros and none of its state, cache rows or validity bytes is touched.

    sampling=True: a request carries temperature / top_k / top_p / seed (sampling_params; include/bitdelta_hip.h, bd_srv_sample_rows, defines the
    token).  They are per-tenant device arrays next to pos / n / limit, written at admission and read by the launch that ends the step
    (serving_ops.step_end_sample) -- never baked into the captured graph, so a tenant changes them from request to request without a new capture.
    The draw index of a token is the cache row it will occupy: it rises through a conversation, extend included, so the same seed replays the same
    conversation and no turn reuses the draws of the turn before; a caller who wants fresh randomness passes a new seed.  Without sampling=True the
    session is greedy and refuses non-default sampling arguments (ValueError).

    logprobs=k (0 .. 20; logprobs_count): the session keeps, per emitted token, its log-probability and the k most probable tokens of its step
    with theirs (result_logprobs; include/bitdelta_hip.h, bd_srv_token_logprobs, defines an entry) -- the model's own distribution, softmax of
    the logits at temperature 1 before top-k / top-p, whatever the request sampled with.  One more launch ends the step
    (serving_ops.step_logprobs, behind the step-end launch) and writes the entry of every tenant whose token count moved; the first token's
    entry comes from the prefill's logits on the device.  The count is the session's: it sizes the buffers and the captured graph.  None keeps
    nothing and launches nothing.

    penalties=True: a request carries repetition_penalty / presence_penalty / frequency_penalty / logit_bias (penalty_params;
    include/bitdelta_hip.h, bd_srv_penalize_rows, defines the penalised row).  The session keeps a token history per tenant (hist [T, V] int16:
    bit 15 = in the context of this turn, bits 0 .. 14 = times generated in this turn), the parameters and the bias list as device arrays, and
    one more launch (serving_ops.step_penalize) between the lm_head and the step-end launch counts the token fed in and writes the penalised
    logits the step end then reads; the first token is chosen from the penalised prefill logits.  Nothing is baked into the captured graph.
    result_logprobs keeps reporting the RAW logits' distribution.  Without penalties=True the session refuses non-neutral values (ValueError),
    allocates none of this and launches nothing more.

    constraints=True: a request may carry constraint= a TokenAutomaton (constraint.py; include/bitdelta_hip.h, bd_srv_constrain_rows, defines the
    masked row), and every token it emits follows the automaton from its start state.  The session keeps, per tenant, the automaton at fixed
    sizes (c_off [T, S + 1], c_tok / c_next [T, E], c_acc [T, S]; S = max_constraint_states, E = max_constraint_edges), the current state
    (c_state [T] int32, -1 = no constraint) and the advance launch's own counter (c_n [T]) as device arrays written at admission, and the step
    gains two launches: serving_ops.step_constrain between the lm_head (or step_penalize, whose row it then reads) and the step end writes
    clogits [T, V] -- -inf wherever the tenant's state does not allow the token, the same bits elsewhere -- which the step end reads;
    serving_ops.step_constrain_advance behind the step end (and step_logprobs) follows the chosen token, and a tenant that reaches a FINAL state
    (accepting, no edges) retires in that same step with reason 8.  In an accepting state the request's own stop ids are allowed too, and
    emitting one is reason 1 as ever.  The first token is chosen from serving_ops.constrain_rows of the (penalised) prefill logits in the start
    state, and the state is advanced once on the host with that token, which admission reads anyway.  extend constrains the new turn only.
    Nothing is baked into the captured graph.  result_logprobs keeps reporting the RAW logits' distribution.  Without constraints=True the
    session refuses a constraint (ValueError), allocates none of this and launches nothing more.

    stop_sequences=True: a request may carry stop_sequences= a list of token-id lists (stop_sequence_table; include/bitdelta_hip.h,
    bd_srv_step_stop_sequences, defines a match) -- OpenAI's `stop`, on token ids: the project has no tokenizer, so the caller turns a stop string
    into the one or several token sequences that spell it and passes them all.  The session keeps, per tenant, the table at fixed sizes (ss_tok
    [T, Q, W] int32, ss_len [T, Q]; Q = max_stop_sequences, W = max_stop_sequence_len), the launch's own counter (ss_n [T]) and its two results
    (hit [T] int32: the index of the matched sequence or -1; hold [T]: how many trailing tokens are a proper prefix of a sequence) as device
    arrays written at admission, and ONE more launch ends the step (serving_ops.step_stop_sequences, behind the step end, step_logprobs and
    step_constrain_advance): a tenant whose turn now ends with one of its sequences retires in that very step with reason 16 -- OR-ed to the
    reasons 1 / 2 / 4 when the step end retired it on the same token.  Only this turn's tokens are compared: a sequence that straddles the
    prompt (or an earlier turn) and the output does not match.  The matched tokens stay in result(t), as a stop token does; stop_match(t) says
    which sequence matched and how long it is, streamable(t) how many leading tokens of result(t) are safe to show (n - hold).  The first
    token comes from the prefill, so admission applies the same rule on the host (stop_sequence_scan): a one-token sequence equal to it
    retires the tenant at admission.  extend matches the new turn only.  A constraint and stop sequences are independent: the automaton is
    not taught to allow the sequences, and a sequence it never lets through never matches -- the two are the caller's to keep consistent.
    Nothing is baked into the captured graph.  Without stop_sequences=True the session refuses them (ValueError), allocates none of this and
    launches nothing more.

    bans=True: a request may carry no_repeat_ngram_size= / bad_words= / min_new_tokens= (ban_params; include/bitdelta_hip.h, bd_srv_ban_rows,
    defines the banned set) -- Hugging Face's NoRepeatNGramLogitsProcessor, bad_words_ids and MinNewTokensLengthLogitsProcessor, hard bans that
    depend on what the request has already written.  The session keeps, per tenant, the conversation's real tokens (ctx [T, Lc] int32 with
    ctx_len [T]; the host keeps the list and extend appends the earlier turn's emitted tokens and the new ones), the n-gram size (ban_ngram
    [T]), the bad-word table at fixed sizes (ban_tok [T, Q, W] int32, ban_len [T, Q]; Q = max_bad_words, W = max_bad_word_len) and the
    minimum turn length (ban_min [T]) as device arrays written at admission, and ONE more launch (serving_ops.step_ban) sits between the
    lm_head -- behind step_penalize and step_constrain, whose row it then reads -- and the step end: it writes blogits [T, V], -inf at every
    token the tenant's history (ctx, then out[t, :n]) forbids and the same bits elsewhere, which the step end reads.  The order makes a ban
    win over a positive logit_bias and over a constraint's edge.  The launch keeps no counter: it is a pure function of the row, ctx, out, n
    and the tables.  The first token is chosen from serving_ops.ban_rows of the (penalised, constrained) prefill logits.  min_new_tokens holds
    back the request's stop IDS while the turn is shorter: not its stop sequences (reason 16) and not a constraint's final state (reason 8).
    Below the longest bad word's length the rule deviates from HF on purpose: a bad word's prefix is matched as soon as the history holds it,
    so a two-token bad word right behind a one-token prompt is banned.  A request whose bans, alone or with a constraint, leave no finite
    logit is the caller's error, as a -inf bias on every token is.  Nothing is baked into the captured graph.  result_logprobs keeps reporting
    the RAW logits' distribution.  Without bans=True the session refuses non-default values (ValueError), allocates none of this and launches
    nothing more.

    truncation=True (a sampling session only): a request may carry min_p= / typical_p= / epsilon_cutoff= / eta_cutoff= (truncation_params;
    include/bitdelta_hip.h, bd_srv_truncate_rows, defines the kept set) -- Hugging Face's MinPLogitsWarper, TypicalLogitsWarper,
    EpsilonLogitsWarper and EtaLogitsWarper, the filters that cut the tail by the row's own statistics at the request's temperature.  The
    session keeps the four numbers per tenant (trunc [T, 4] float32, written at admission) and ONE more launch (serving_ops.step_truncate)
    sits behind step_penalize, step_constrain and step_ban -- the last of the masks, judged on the row they leave -- and in front of
    step_end_sample, which reads its output tlogits [T, V], applies top-k / top-p to the survivors and draws.  With one filter set and top-k /
    top-p off this is the Hugging Face warper of that name; with several set the kept set is the INTERSECTION of the sets each filter keeps on
    the same row (HF applies them one after another on renormalised survivors), and typical_p is ignored on a row where its set does not meet
    the thresholds' set.  typical_p may drop the most probable token.  A greedy request (temperature 0) is not touched.  The launch keeps no
    counter: it is a pure function of the row and the five numbers.  The first token is chosen from serving_ops.truncate_rows of the
    (penalised, constrained, banned) prefill logits.  Nothing is baked into the captured graph.  result_logprobs keeps reporting the RAW
    logits' distribution.  Without truncation=True the session refuses non-neutral values (ValueError), allocates none of this and launches
    nothing more.

    One sequence per tenant, the decoder's ONE KV cache.  `generate` is the lockstep loop of the reference and is not changed by this:
    it runs every tenant until all have stopped, a session stops each tenant at ITS stop token.
    reason (result(t)[1], bits): 1 = stop token, 2 = max_new_tokens reached, 4 = the cache is full, 8 = the constraint is complete (a final state
    of the request's automaton was reached), 16 = the turn ends with one of the request's stop sequences; 0 = still active or never submitted."""

    def __init__(self, dec, max_stop_ids=8, sampling=False, logprobs=None, penalties=False, max_logit_bias=16, constraints=False,
                 max_constraint_states=256, max_constraint_edges=4096, stop_sequences=False, max_stop_sequences=4, max_stop_sequence_len=8,
                 bans=False, max_bad_words=16, max_bad_word_len=8, truncation=False):
        self.logprobs = logprobs_count(logprobs)
        self.truncation = bool(truncation)
        if self.truncation and not sampling:
            raise ValueError("truncation=True cuts the tail of a sampled distribution: make the session with sampling=True as well")
        self.penalties = bool(penalties)
        self.constraints = bool(constraints)
        self.stop_sequences = bool(stop_sequences)
        if self.stop_sequences:
            for v, what, top in ((max_stop_sequences, "max_stop_sequences", ops.STOP_SEQ_MAX),
                                 (max_stop_sequence_len, "max_stop_sequence_len", ops.STOP_SEQ_LEN_MAX)):
                if not (isinstance(v, int) and not isinstance(v, bool) and 1 <= v <= top):
                    raise ValueError("%s = %r: an integer 1 .. %d is required" % (what, v, top))
        self.bans = bool(bans)
        if self.bans:
            for v, what, top in ((max_bad_words, "max_bad_words", ops.BAN_WORDS_MAX), (max_bad_word_len, "max_bad_word_len", ops.BAN_WORD_LEN_MAX)):
                if not (isinstance(v, int) and not isinstance(v, bool) and 1 <= v <= top):
                    raise ValueError("%s = %r: an integer 1 .. %d is required" % (what, v, top))
            if max(int(max_stop_ids), 1) > ops.BAN_STOP_MAX:
                raise ValueError("a session with bans holds at most %d stop ids per request" % ops.BAN_STOP_MAX)
        if self.constraints:
            for v, what, top in ((max_constraint_states, "max_constraint_states", ops.CONSTRAINT_STATES_MAX),
                                 (max_constraint_edges, "max_constraint_edges", ops.CONSTRAINT_EDGES_MAX)):
                if not (isinstance(v, int) and not isinstance(v, bool) and 1 <= v <= top):
                    raise ValueError("%s = %r: an integer 1 .. %d is required" % (what, v, top))
            if max(int(max_stop_ids), 1) > ops.CONSTRAINT_STOP_MAX:
                raise ValueError("a session with constraints holds at most %d stop ids per request" % ops.CONSTRAINT_STOP_MAX)
        if self.penalties and not (isinstance(max_logit_bias, int) and not isinstance(max_logit_bias, bool)
                                   and 0 <= max_logit_bias <= ops.LOGIT_BIAS_MAX):
            raise ValueError("max_logit_bias = %r: an integer 0 .. %d is required" % (max_logit_bias, ops.LOGIT_BIAS_MAX))
        _, _, _, heads, kvh, _ = dec.cfg
        if not (dec.fast_glue and dec.step_kernels):
            raise ValueError("a session runs on the HIP glue and step kernels (fast_glue, step_kernels); there is no stock-op ragged step")
        if not ops.decode_attention_supported(heads, kvh, dec.hd):
            raise ValueError("a session needs the HIP decode attention: head_dim 128 and 1, 4 or 8 query heads per kv head")
        if dec.embed.shape[-1] % 8 or dec.lm_head.shape[-2] % 8:
            raise ValueError("a session needs hidden and vocabulary sizes that are multiples of 8 (the step kernels' 16-byte rows)")
        if dec.prefetch_o:
            raise ValueError("a session does not take prefetch_o=True (a side branch in the captured step)")
        self.dec, self.T, dev = dec, dec.T, dec.dev
        if dec._kv_cache is None:
            dec._kv_cache = dec.new_cache()
        self.cache = dec._kv_cache
        self.Lc = self.cache["valid"].shape[1]
        T = self.T
        self.tok = torch.zeros(T, 1, dtype=torch.long, device=dev)
        self.pos = torch.zeros(T, dtype=torch.long, device=dev)
        self.n = torch.zeros(T, dtype=torch.long, device=dev)
        self.limit = torch.zeros(T, dtype=torch.long, device=dev)
        self.active_flags = torch.zeros(T, dtype=torch.bool, device=dev)
        self.done = torch.zeros(T, dtype=torch.uint8, device=dev)
        self.stop_ids = torch.full((T, max(int(max_stop_ids), 1)), -1, dtype=torch.long, device=dev)
        self.out = torch.zeros(T, dec.max_len, dtype=torch.long, device=dev)      # (a caller may swap in a strided view BEFORE the first step)
        self.sampling = bool(sampling)
        if self.sampling:
            self.temperature = torch.zeros(T, dtype=torch.float32, device=dev)
            self.top_k = torch.zeros(T, dtype=torch.int32, device=dev)
            self.top_p = torch.ones(T, dtype=torch.float32, device=dev)
            self.seed = torch.zeros(T, dtype=torch.long, device=dev)          # the seed's 64 bits
        if self.logprobs is not None:                 # entry [t, j] belongs to out[t, j]; entries at or past n[t] are unspecified
            cap, k = self.out.shape[1], self.logprobs
            self.lp_n = torch.zeros(T, dtype=torch.long, device=dev)          # step_logprobs' own counter: follows n
            self.lp = torch.zeros(T, cap, dtype=torch.float32, device=dev)
            self.top_id = torch.zeros(T, cap, k, dtype=torch.int32, device=dev)
            self.top_lp = torch.zeros(T, cap, k, dtype=torch.float32, device=dev)
        if self.penalties:                            # per tenant: token history, (r, 1 / r, presence, frequency), the bias list, the penalised row
            V = dec.lm_head.shape[-2]
            self.hist = torch.zeros(T, V, dtype=torch.int16, device=dev)
            self.pen = torch.tensor([penalty_row(NEUTRAL)] * T, dtype=torch.float32).to(dev)
            self.bias_id = torch.full((T, max_logit_bias), -1, dtype=torch.int32, device=dev)
            self.bias_val = torch.zeros(T, max_logit_bias, dtype=torch.float32, device=dev)
            self.plogits = torch.zeros(T, V, dtype=dec.lm_head.dtype, device=dev)
        if self.constraints:                          # per tenant: the automaton at the session's sizes, its state, the advance launch's counter, the masked row
            V, S, E = dec.lm_head.shape[-2], max_constraint_states, max_constraint_edges
            self.c_state = torch.full((T,), -1, dtype=torch.int32, device=dev)
            self.c_n = torch.zeros(T, dtype=torch.long, device=dev)           # step_constrain_advance's own counter: follows n
            self.c_off = torch.zeros(T, S + 1, dtype=torch.int32, device=dev)
            self.c_tok = torch.zeros(T, E, dtype=torch.int32, device=dev)
            self.c_next = torch.zeros(T, E, dtype=torch.int32, device=dev)
            self.c_acc = torch.zeros(T, S, dtype=torch.uint8, device=dev)
            self.clogits = torch.zeros(T, V, dtype=dec.lm_head.dtype, device=dev)
        if self.stop_sequences:                       # per tenant: the table at the session's sizes, the launch's counter, its two results
            Q, W = max_stop_sequences, max_stop_sequence_len
            self.ss_tok = torch.full((T, Q, W), -1, dtype=torch.int32, device=dev)
            self.ss_len = torch.zeros(T, Q, dtype=torch.int32, device=dev)
            self.ss_n = torch.zeros(T, dtype=torch.long, device=dev)          # step_stop_sequences' own counter: follows n
            self.hit = torch.full((T,), -1, dtype=torch.int32, device=dev)
            self.hold = torch.zeros(T, dtype=torch.int32, device=dev)
        if self.bans:                                 # per tenant: the conversation's real tokens, the three parameters at the session's sizes, the masked row
            V, Q, W = dec.lm_head.shape[-2], max_bad_words, max_bad_word_len
            self.ctx = torch.zeros(T, self.Lc, dtype=torch.int32, device=dev)
            self.ctx_len = torch.zeros(T, dtype=torch.int32, device=dev)
            self.ban_ngram = torch.zeros(T, dtype=torch.int32, device=dev)
            self.ban_tok = torch.full((T, Q, W), -1, dtype=torch.int32, device=dev)
            self.ban_len = torch.zeros(T, Q, dtype=torch.int32, device=dev)
            self.ban_min = torch.zeros(T, dtype=torch.int32, device=dev)
            self.blogits = torch.zeros(T, V, dtype=dec.lm_head.dtype, device=dev)
            self._ctx_tokens = [[] for _ in range(T)]  # the host's copy of ctx[t, :ctx_len[t]]: extend appends to it
        if self.truncation:                           # per tenant: (min_p, typical_p, epsilon_cutoff, eta_cutoff), and the truncated row
            self.trunc = torch.tensor([NO_TRUNCATION] * T, dtype=torch.float32).to(dev)
            self.tlogits = torch.zeros(T, dec.lm_head.shape[-2], dtype=dec.lm_head.dtype, device=dev)
        self._first_lp = None           # the first tokens' entries between _first_tokens and _admit (device tensors)
        self._graphs = {}
        self._kv_start = [None] * T     # per tenant: the first cache row of its conversation (left pads of its first prompt); None = nothing to extend
        dec._sessions.add(self)

    # ------------------------------------------------------------ admission
    @torch.no_grad()
    def load_tenant(self, t, state, tag=None, rope=None):
        """Put another fine-tune into slot t (TenantDecoder.load_tenant) while the other tenants keep generating: refused (RuntimeError) while
        tenant t is active.  Runs on the current stream, i.e. ordered between the replays around it; tenant t's validity bytes, stop reason, token
        count and output row are cleared, nobody else's state, cache rows or validity bytes are touched.  Host reads: tenant t's own activity
        flag (as in submit) and, where a hand-off norm is cached, the decoder's one read of the new norm rows' maxima.
        tag: the slot's fine-tune tag afterwards (TenantDecoder.load_tenant, tenant_tag); a refused load leaves the tag as it was.
        rope: the slot's rotary embedding afterwards (rope_spec; None = the decoder's default), as TenantDecoder.load_tenant takes it: on per-tenant
        tables the slot's rows are rewritten in place, so the session's captured graphs stay; a shared-table decoder refuses another spec before
        anything is written.  The slot's cached keys were rotated with the old table: extend() after a load refuses, as before."""
        if not (isinstance(t, int) and 0 <= t < self.T):
            raise IndexError("tenant %r: this session holds slots 0 .. %d" % (t, self.T - 1))
        if tag is not None:
            hash(tag)
        if bool(self.active_flags[t]):
            raise RuntimeError("tenant %d is still generating" % t)
        rescaled = self.dec.load_tenant(t, state, tag=tag, rope=rope)
        self._kv_start[t] = None                      # the cache rows belong to the fine-tune that left: nothing to extend
        self.cache["valid"][t].zero_()
        self.done[t] = 0
        self.n[t] = 0
        self.out[t].zero_()
        if self.logprobs is not None:
            self.lp_n[t] = 0
        if self.sampling:
            self._write_params(t, GREEDY)
        if self.penalties:
            self.hist[t].zero_()
            self._write_penalties(t, NEUTRAL)
        if self.constraints:
            self.c_state[t] = -1
            self.c_n[t] = 0
        if self.stop_sequences:
            self._write_stop_sequences(t, self._stop_sequences_arg(()), -1, 0, 0)
        if self.bans:
            self._write_bans(t, NO_BANS, [], [])
        if self.truncation:
            self._write_truncation(t, NO_TRUNCATION)
        return rescaled

    def _params(self, temperature, top_k, top_p, seed):
        """one request's validated parameters; a session made without sampling=True takes the defaults only"""
        sp = sampling_params(temperature, top_k, top_p, seed)
        if not self.sampling and sp != GREEDY:
            raise ValueError("this session is greedy: make it with session(sampling=True) to pass temperature / top_k / top_p / seed")
        return sp

    def _penalty_params(self, repetition_penalty, presence_penalty, frequency_penalty, logit_bias):
        """one request's validated penalty parameters; a session made without penalties=True takes the neutral values only"""
        pp = penalty_params(repetition_penalty, presence_penalty, frequency_penalty, logit_bias, vocab=self.dec.lm_head.shape[-2],
                            max_logit_bias=self.bias_id.shape[1] if self.penalties else ops.LOGIT_BIAS_MAX)
        if not self.penalties and pp != NEUTRAL:
            raise ValueError("this session takes no penalties: make it with session(penalties=True) to pass repetition_penalty / "
                             "presence_penalty / frequency_penalty / logit_bias")
        return pp

    def _constraint_arg(self, constraint):
        """a request's constraint= argument: None or a TokenAutomaton; a session made without constraints=True takes None only"""
        if constraint is None:
            return None
        if not self.constraints:
            raise ValueError("this session takes no constraint: make it with session(constraints=True) to pass constraint=")
        if not isinstance(constraint, TokenAutomaton):
            raise ValueError("constraint = %r: None or a TokenAutomaton is required" % (constraint,))
        return constraint

    def _stop_sequences_arg(self, seqs):
        """a request's stop_sequences= argument, validated before anything is touched: None for a session made without stop_sequences=True (which
        takes an empty value only), otherwise (seqs as lists of ints, in the caller's order; stop_sequence_table's rows)"""
        if not self.stop_sequences:
            if seqs is None or (isinstance(seqs, (list, tuple)) and len(seqs) == 0):
                return None
            raise ValueError("this session takes no stop sequences: make it with session(stop_sequences=True) to pass stop_sequences=")
        Q, W = self.ss_tok.shape[1], self.ss_tok.shape[2]
        tok, lens = stop_sequence_table(seqs, Q, W, self.dec.lm_head.shape[-2])
        return [row[:l] for row, l in zip(tok, lens) if l], (tok, lens)

    def _ban_params(self, no_repeat_ngram_size, bad_words, min_new_tokens):
        """one request's validated bans, before anything is touched; a session made without bans=True takes the defaults only"""
        if not self.bans:
            bp = ban_params(no_repeat_ngram_size, bad_words, min_new_tokens)
            if bp != NO_BANS:
                raise ValueError("this session takes no bans: make it with session(bans=True) to pass no_repeat_ngram_size / bad_words / "
                                 "min_new_tokens")
            return bp
        return ban_params(no_repeat_ngram_size, bad_words, min_new_tokens, vocab=self.dec.lm_head.shape[-2], max_bad_words=self.ban_tok.shape[1],
                          max_bad_word_len=self.ban_tok.shape[2])

    def _truncation_params(self, min_p, typical_p, epsilon_cutoff, eta_cutoff):
        """one request's validated truncation, before anything is touched; a session made without truncation=True takes the neutral values only"""
        tp = truncation_params(min_p, typical_p, epsilon_cutoff, eta_cutoff)
        if not self.truncation and tp != NO_TRUNCATION:
            raise ValueError("this session truncates nothing: make it with session(sampling=True, truncation=True) to pass min_p / typical_p / "
                             "epsilon_cutoff / eta_cutoff")
        return tp

    def _write_truncation(self, t, tp):
        """a truncation session, before the first token is chosen: tenant t's four numbers.  One torch op on the current stream, no host read."""
        if self.truncation:
            self.trunc[t] = torch.tensor(tp, dtype=torch.float32).to(self.dec.dev)

    def _per_tenant_bad_words(self, v):
        """submit_all's bad_words=: one list of token-id lists for all tenants, or a list with one such list per tenant, told apart by depth as
        _per_tenant_stop_sequences tells stop sequences apart"""
        return self._per_tenant_stop_sequences(v)

    def _check_conversation(self, tokens):
        """a ban session keeps the conversation's real tokens as int32, at most one per cache row"""
        if self.bans and not (len(tokens) <= self.Lc and all(-2 ** 31 <= int(i) < 2 ** 31 for i in tokens)):
            raise ValueError("the conversation does not fit the ban history (%d tokens, int32 ids)" % self.Lc)

    def _write_bans(self, t, bp, tokens, stops):
        """a ban session, before the first token is chosen: tenant t's conversation so far (`tokens`: ALL its real tokens up to this turn; the
        host keeps the list), its three parameters, and the stop ids min_new_tokens holds back.  Torch ops on the current stream, no host
        read."""
        if not self.bans:
            return
        dev = self.dec.dev
        tokens = [int(i) for i in tokens]
        self._ctx_tokens[t] = tokens
        if tokens:
            self.ctx[t, :len(tokens)] = torch.tensor(tokens, dtype=torch.int32).to(dev)
        self.ctx_len[t] = len(tokens)
        g, words, lo = bp
        tok, lens = ban_word_table(words, self.ban_tok.shape[1], self.ban_tok.shape[2])
        self.ban_ngram[t] = g
        self.ban_tok[t] = torch.tensor(tok, dtype=torch.int32).to(dev)
        self.ban_len[t] = torch.tensor(lens, dtype=torch.int32).to(dev)
        self.ban_min[t] = lo
        self.stop_ids[t].fill_(-1)                    # (_admit writes the same values again)
        if stops:
            self.stop_ids[t, :len(stops)] = torch.tensor(stops, dtype=torch.long).to(dev)

    def _per_tenant_stop_sequences(self, v):
        """submit_all's stop_sequences=: one list of token-id lists for all tenants, or a list with one such list per tenant.  The two are told
        apart by depth: the value is PER TENANT when it is not empty and none of its elements holds a token id directly -- every element is
        itself a (possibly empty) list / tuple of lists / tuples, e.g. [[[5, 6]], [], [[7], [8, 9]], []] -- and must then have one element per
        tenant (_per_tenant's rule: ValueError otherwise).  [[5, 6], [7]] is one list of two sequences for all, [] / None is none for all, and
        [[], []] reads as two tenants without sequences (an empty sequence is never valid, so nothing is lost)."""
        seq = (list, tuple)
        if isinstance(v, seq) and len(v) and all(isinstance(e, seq) and all(isinstance(x, seq) for x in e) for e in v):
            if len(v) != self.T:
                raise ValueError("%d values for %d tenants" % (len(v), self.T))
            return list(v)
        return [v] * self.T

    def _write_stop_sequences(self, t, ss, hit, hold, n):
        """a stop-sequence session: tenant t's table rows (_stop_sequences_arg's), results and counter.  Torch ops on the current stream, no host
        read."""
        dev = self.dec.dev
        tok, lens = ss[1]
        self.ss_tok[t] = torch.tensor(tok, dtype=torch.int32).to(dev)
        self.ss_len[t] = torch.tensor(lens, dtype=torch.int32).to(dev)
        self.hit[t] = hit
        self.hold[t] = hold
        self.ss_n[t] = n

    def _check_constraint(self, con, stops):
        """the checks that need the session's sizes and the request's stop ids (TokenAutomaton.check), before anything is touched"""
        if con is not None:
            con.check(self.dec.lm_head.shape[-2], self.c_acc.shape[1], self.c_tok.shape[1], bool(stops))
        return con

    def _write_constraint(self, t, con, stops):
        """a constraint session, before the first token is chosen: the automaton into tenant t's slices (the rest of them is never indexed: every
        offset and target lies inside what is written), the start state or -1, and the stop ids the start state may allow.  Torch ops on the
        current stream, no host read."""
        if not self.constraints:
            return
        dev = self.dec.dev
        self.stop_ids[t].fill_(-1)                    # (_admit writes the same values again)
        if stops:
            self.stop_ids[t, :len(stops)] = torch.tensor(stops, dtype=torch.long).to(dev)
        if con is None:
            self.c_state[t] = -1
            return
        S, E = con.n_states, con.n_edges
        self.c_off[t, :S + 1] = torch.tensor(con.off, dtype=torch.int32).to(dev)
        if E:
            self.c_tok[t, :E] = torch.tensor(con.edge_tok, dtype=torch.int32).to(dev)
            self.c_next[t, :E] = torch.tensor(con.edge_next, dtype=torch.int32).to(dev)
        self.c_acc[t, :S] = torch.tensor(con.accepting, dtype=torch.uint8).to(dev)
        self.c_state[t] = 0

    def _write_penalties(self, t, pp):
        cap = self.bias_id.shape[1]
        self.pen[t] = torch.tensor(penalty_row(pp), dtype=torch.float32).to(self.dec.dev)
        if cap:
            bias = pp[3]
            self.bias_id[t] = torch.tensor([b[0] for b in bias] + [-1] * (cap - len(bias)), dtype=torch.int32).to(self.dec.dev)
            self.bias_val[t] = torch.tensor([b[1] for b in bias] + [0.0] * (cap - len(bias)), dtype=torch.float32).to(self.dec.dev)

    def _context(self, t, tokens, pp, fold=False):
        """a penalty session, before the first token is chosen: tenant t's parameters, and its history -- cleared (submit) or folded (extend:
        fold_history), then bit 15 set at `tokens`, the real tokens this admission adds to the context.  Torch ops on the current stream, no
        host read."""
        if not self.penalties:
            return
        self._write_penalties(t, pp)
        if fold:
            self.hist[t] = fold_history(self.hist[t])
        else:
            self.hist[t].zero_()
        self.hist[t].index_fill_(0, torch.tensor(tokens, dtype=torch.long).to(self.dec.dev), -32768)

    def _check_tokens(self, tokens):
        """a penalty session indexes its history with the request's tokens: ids outside the vocabulary are refused on the host"""
        if self.penalties and not all(0 <= int(i) < self.hist.shape[1] for i in tokens):
            raise ValueError("a token id is outside the vocabulary")

    def _per_tenant(self, v):
        if isinstance(v, torch.Tensor):
            v = v.tolist()
        if isinstance(v, (list, tuple)):
            if len(v) != self.T:
                raise ValueError("%d values for %d tenants" % (len(v), self.T))
            return list(v)
        return [v] * self.T

    def _write_params(self, t, sp):
        tau, k, p, s_ = sp
        self.temperature[t] = tau
        self.top_k[t] = min(k, 2 ** 31 - 1)
        self.top_p[t] = p
        self.seed[t] = s_ - (1 << 64) if s_ >= 1 << 63 else s_

    def _first_tokens(self, logits, sps, d, rows=slice(None)):
        """the first token of each row of the prefill's logits [R, V] (they stay on the device) under its request's parameters, draw index d: the
        cache row the token will occupy.  One host read, the one admission makes anyway.  rows: the tenants the R rows belong to; a penalty
        session chooses from their penalised rows (serving_ops.penalize_rows on the history and parameters _context has just written), a
        constraint session from those rows masked by the start states _write_constraint has just written (serving_ops.constrain_rows), and
        the log-probabilities are still the raw rows'."""
        raw = logits
        if self.penalties:
            logits = ops.penalize_rows(logits, self.hist[rows], self.pen[rows], self.bias_id[rows], self.bias_val[rows])
        if self.constraints:
            logits = ops.constrain_rows(logits, self.c_state[rows].contiguous(), self.c_off[rows].contiguous(), self.c_tok[rows].contiguous(),
                                        self.c_acc[rows].contiguous(), self.stop_ids[rows].contiguous())
        if self.bans:                                 # n absent: the turn has no token yet, so min_new_tokens > 0 holds back the stop ids here too
            logits = ops.ban_rows(logits, self.ctx[rows].contiguous(), self.ctx_len[rows].contiguous(), self.ban_ngram[rows].contiguous(),
                                  self.ban_tok[rows].contiguous(), self.ban_len[rows].contiguous(), self.ban_min[rows].contiguous(),
                                  self.stop_ids[rows].contiguous())
        if not self.sampling:
            tok = torch.argmax(logits, dim=-1)
            self._keep_first_logprobs(raw, tok)
            return tok.tolist()
        dev = self.dec.dev
        if self.truncation:                           # the last of the masks, at the request's own temperature (_admit writes it to the device later)
            logits = ops.truncate_rows(logits, torch.tensor([sp[0] for sp in sps], dtype=torch.float32).to(dev), self.trunc[rows].contiguous())
        if not (logits.stride(1) == 1 and logits.stride(0) % 8 == 0 and logits.data_ptr() % 16 == 0):
            logits = logits.contiguous()
        tok = ops.sample_rows(logits, torch.tensor([sp[0] for sp in sps], dtype=torch.float32).to(dev),
                              torch.tensor([min(sp[1], 2 ** 31 - 1) for sp in sps], dtype=torch.int32).to(dev),
                              torch.tensor([sp[2] for sp in sps], dtype=torch.float32).to(dev),
                              torch.tensor([sp[3] - (1 << 64) if sp[3] >= 1 << 63 else sp[3] for sp in sps], dtype=torch.long).to(dev),
                              torch.full((len(sps),), int(d), dtype=torch.long).to(dev))
        self._keep_first_logprobs(raw, tok)
        return tok.tolist()

    def _keep_first_logprobs(self, logits, tok):
        """a logprob session: the first tokens' entries from the prefill's logits [R, V] and the tokens just chosen, both still on the device;
        _admit copies row r into the tenant's entry 0.  No host read."""
        if self.logprobs is not None:
            self._first_lp = ops.token_logprobs(logits, tok.view(-1), self.logprobs)

    def _stops(self, stop_token_ids):
        s_ = sorted(int(i) for i in (stop_token_ids or ()))
        if len(s_) > self.stop_ids.shape[1]:
            raise ValueError("more stop ids than session(max_stop_ids=%d) holds" % self.stop_ids.shape[1])
        return s_

    def _admit(self, t, first, L, max_new_tokens, stops, sp=GREEDY, row=0, con=None, ss=None):
        """tenant t's state after its prefill: the first token is the prefill's (argmax, or _first_tokens' draw); row: its row of that prefill;
        con: the request's automaton, advanced here once, on the host, with that first token; ss: _stop_sequences_arg's value, matched here
        once, on the host, against that first token"""
        if self.sampling:
            self._write_params(t, sp)
        if self.logprobs is not None:                 # the turn's entries restart with it, as result() does
            lp, top_id, top_lp = self._first_lp
            self.lp[t, 0] = lp[row]
            self.top_id[t, 0] = top_id[row]
            self.top_lp[t, 0] = top_lp[row]
            self.lp_n[t] = 1
        reason = (1 if first in stops else 0) | (2 if max_new_tokens <= 1 else 0) | (4 if L >= self.Lc else 0)
        if self.constraints:
            self.c_n[t] = 1
            if con is not None:
                s_ = con.step(0, first)
                self.c_state[t] = s_
                reason |= 8 if con.is_final(s_) else 0
        if self.stop_sequences:                       # the rule of the launch for n = 1: a one-token sequence equal to the first token is a hit
            hit, hold = stop_sequence_scan([first], ss[0])
            self._write_stop_sequences(t, ss, hit, hold, 1)
            reason |= 16 if hit >= 0 else 0
        self.stop_ids[t].fill_(-1)
        if stops:
            self.stop_ids[t, :len(stops)] = torch.tensor(stops, dtype=torch.long, device=self.dec.dev)
        self.out[t].zero_()
        self.out[t, 0] = first
        self.tok[t, 0] = first
        self.n[t] = 1
        self.pos[t] = L
        self.limit[t] = int(max_new_tokens)
        self.done[t] = reason
        self.active_flags[t] = reason == 0

    @torch.no_grad()
    def submit(self, t, prompt, max_new_tokens=16, stop_token_ids=(), temperature=0.0, top_k=0, top_p=1.0, seed=0, repetition_penalty=1.0,
               presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, constraint=None, stop_sequences=(), no_repeat_ngram_size=0,
               bad_words=(), min_new_tokens=0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
        """Admit one request for tenant t; the other tenants' state, cache rows and validity bytes are not touched.  The prompt is left-padded to
        padded_length(len(prompt)) and refused beyond MAX_PROMPT (the reference's per-request rules, per tenant), prefilled for this tenant
        alone through tenant_view(t), and the tenant starts at its own position.  temperature / top_k / top_p / seed: sampling_params, in a
        session(sampling=True); the first token's draw index is the padded length L.  repetition_penalty / presence_penalty /
        frequency_penalty / logit_bias: penalty_params, in a session(penalties=True); the context of the turn is the prompt's real tokens.
        constraint: None or a TokenAutomaton, in a session(constraints=True): every token of the turn follows it from its start state; refused
        (ValueError, before anything is touched) when it does not fit the session's sizes or the vocabulary (TokenAutomaton.check).
        stop_sequences: a list of token-id lists, in a session(stop_sequences=True): the tenant retires with reason 16 in the step after which
        this turn's tokens end with one of them (stop_sequence_table's refusals: ValueError, before anything is touched).
        no_repeat_ngram_size / bad_words / min_new_tokens: ban_params, in a session(bans=True); the history they look at is the prompt's real
        tokens followed by the turn's own, and the first token obeys them too.
        min_p / typical_p / epsilon_cutoff / eta_cutoff: truncation_params, in a session(sampling=True, truncation=True); they cut the row the
        token is sampled from, behind every other mask and in front of top-k / top-p, and the first token obeys them too."""
        dec = self.dec
        assert 0 <= t < self.T and len(prompt) >= 1 and max_new_tokens >= 1
        sp = self._params(temperature, top_k, top_p, seed)
        pp = self._penalty_params(repetition_penalty, presence_penalty, frequency_penalty, logit_bias)
        con = self._constraint_arg(constraint)
        ss = self._stop_sequences_arg(stop_sequences)
        bp = self._ban_params(no_repeat_ngram_size, bad_words, min_new_tokens)
        tp = self._truncation_params(min_p, typical_p, epsilon_cutoff, eta_cutoff)
        self._check_tokens(prompt)
        self._check_conversation(prompt)
        if bool(self.active_flags[t]):
            raise RuntimeError("tenant %d is still generating" % t)
        L = padded_length(len(prompt))
        if L > MAX_PROMPT:
            raise ValueError("max_len too large, please reduce the input length")
        if L > self.Lc:
            raise ValueError("the padded prompt does not fit the KV cache")
        stops = self._stops(stop_token_ids)
        self._check_constraint(con, stops)
        ids = torch.zeros(1, L, dtype=torch.long)
        am = torch.zeros(1, L, dtype=torch.bool)
        ids[0, L - len(prompt):] = torch.tensor(prompt, dtype=torch.long)
        am[0, L - len(prompt):] = True
        logits = dec.tenant_view(t).prefill(ids.to(dec.dev), am.to(dec.dev), dec.cache_view(self.cache, t))      # clears valid[t], writes rows [0, L)
        self._context(t, prompt, pp)
        self._write_constraint(t, con, stops)
        self._write_bans(t, bp, prompt, stops)
        self._write_truncation(t, tp)
        self._admit(t, int(self._first_tokens(logits, [sp], L, slice(t, t + 1))[0]), L, max_new_tokens, stops, sp, con=con, ss=ss)
        self._kv_start[t] = L - len(prompt)

    @torch.no_grad()
    def extend(self, t, tokens, max_new_tokens=16, stop_token_ids=(), temperature=0.0, top_k=0, top_p=1.0, seed=0, repetition_penalty=1.0,
               presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, constraint=None, stop_sequences=(), no_repeat_ngram_size=0,
               bad_words=(), min_new_tokens=0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
        """The next turn of tenant t's conversation FROM ITS CACHED KEYS: `tokens` (the new user turn; may be empty) follow what the tenant was
        submitted and has generated so far, and only they are prefilled -- the reference re-sends and re-prefills the whole history with every
        request (demo/demo_backend.py:261-315).  The cache of a retired tenant holds its conversation up to, not including, its last emitted
        token, so the chunk is [that token] + tokens at rows P .. P + n - 1, P = pos[t]; it runs through tenant_view(t).prefill_chunk, and the
        tenant is admitted as after a submit of P + n rows: result(t) restarts with this turn's tokens.  Refusals (extend_plan), all raised
        before any state or cache row is touched: an active tenant, one never submitted or whose fine-tune was replaced since (RuntimeError), one
        whose cache rows are full (RuntimeError), a chunk that does not fit the cache, a conversation whose padded real length passes MAX_PROMPT
        (ValueError).  Nobody else's state, cache rows or validity bytes are touched, and the captured step is reused.  One host read before the
        prefill (tenant t's activity flag, position, stop reason and last token together) and, as in submit, one of the first token after it.
        The conversation is the decoder's cache rows: a generate() on the decoder ends it
        without the session knowing.  temperature / top_k / top_p / seed as in submit (this turn's own; invalid ones raise ValueError before
        anything is touched); the first token's draw index is P + n.  The penalty arguments as in submit (this turn's own); the turn's context is
        everything the conversation held before it plus [last emitted token] + tokens, and its counts start at zero (fold_history).
        constraint as in submit: it constrains THIS turn's tokens only, from its start state; None leaves the turn free.
        stop_sequences as in submit: they replace the turn before's, and matching restarts with the turn, as result() does -- tokens of earlier
        turns never take part.  A tenant retired by reason 16 is extended like one retired by a stop token: its last token, the one that
        completed the sequence, is the one not yet in the cache.
        no_repeat_ngram_size / bad_words / min_new_tokens as in submit (this turn's own).  The history they look at is the WHOLE conversation:
        what the tenant was submitted, every earlier turn's emitted tokens and new tokens, then `tokens`, then this turn's own -- an n-gram seen
        only in turn one is banned in turn two; min_new_tokens counts this turn's tokens.  A ban session reads the earlier turn's tokens back
        (one more host read) to keep that history.
        min_p / typical_p / epsilon_cutoff / eta_cutoff as in submit (this turn's own; they replace the turn before's)."""
        dec = self.dec
        if not (isinstance(t, int) and 0 <= t < self.T):
            raise IndexError("tenant %r: this session holds slots 0 .. %d" % (t, self.T - 1))
        assert max_new_tokens >= 1
        tokens = [int(i) for i in tokens]
        stops = self._stops(stop_token_ids)
        sp = self._params(temperature, top_k, top_p, seed)
        pp = self._penalty_params(repetition_penalty, presence_penalty, frequency_penalty, logit_bias)
        con = self._check_constraint(self._constraint_arg(constraint), stops)
        ss = self._stop_sequences_arg(stop_sequences)
        bp = self._ban_params(no_repeat_ngram_size, bad_words, min_new_tokens)
        tp = self._truncation_params(min_p, typical_p, epsilon_cutoff, eta_cutoff)
        self._check_tokens(tokens)
        active, pos, done, last = torch.stack([self.active_flags[t].long(), self.pos[t], self.done[t].long(), self.tok[t, 0]]).tolist()
        P, n = extend_plan(pos, self._kv_start[t], done, len(tokens), self.Lc, active=bool(active))
        conv = None
        if self.bans:                                 # the conversation so far: what it held, the turn before's tokens, the new ones
            conv = self._ctx_tokens[t] + self.result(t)[0].tolist() + tokens
            self._check_conversation(conv)
        ids = torch.tensor([[last] + tokens], dtype=torch.long).to(dec.dev)
        kvs = torch.tensor([self._kv_start[t]], dtype=torch.int32).to(dec.dev)
        logits = dec.tenant_view(t).prefill_chunk(ids, P, dec.cache_view(self.cache, t), kvs)      # marks valid[t, P : P + n], writes those rows
        self._context(t, [last] + tokens, pp, fold=True)
        self._write_constraint(t, con, stops)
        self._write_bans(t, bp, conv, stops)
        self._write_truncation(t, tp)
        self._admit(t, int(self._first_tokens(logits, [sp], P + n, slice(t, t + 1))[0]), P + n, max_new_tokens, stops, sp, con=con, ss=ss)

    @torch.no_grad()
    def submit_all(self, prompts, max_new_tokens=16, stop_token_ids=None, temperature=0.0, top_k=0, top_p=1.0, seed=0, repetition_penalty=1.0,
                   presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, constraint=None, stop_sequences=(), no_repeat_ngram_size=0,
                   bad_words=(), min_new_tokens=0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
        """The reference's request shape: one prompt per tenant, one batched prepare + prefill exactly as generate does, every tenant at the
        common padded length.  temperature / top_k / top_p / seed and the four penalty arguments: each one value for all (a logit_bias mapping
        is one value) or a list with one value per tenant.  constraint: None or one TokenAutomaton for all, or a list with one (or None) per
        tenant.  stop_sequences: one list of token-id lists for all, or a list with one such list per tenant; the two are told apart by depth
        (_per_tenant_stop_sequences).  no_repeat_ngram_size / min_new_tokens: one value for all or a list with one per tenant; bad_words: one list
        of token-id lists for all or a list with one such list per tenant, told apart as stop_sequences are.  min_p / typical_p / epsilon_cutoff /
        eta_cutoff: each one value for all or a list with one per tenant."""
        dec = self.dec
        assert max_new_tokens >= 1
        bps = [self._ban_params(*a) for a in zip(self._per_tenant(no_repeat_ngram_size), self._per_tenant_bad_words(bad_words),
                                                 self._per_tenant(min_new_tokens))]
        tps = [self._truncation_params(*a) for a in zip(self._per_tenant(min_p), self._per_tenant(typical_p), self._per_tenant(epsilon_cutoff),
                                                        self._per_tenant(eta_cutoff))]
        sps = [self._params(*a) for a in zip(self._per_tenant(temperature), self._per_tenant(top_k), self._per_tenant(top_p),
                                             self._per_tenant(seed))]
        pps = [self._penalty_params(*a) for a in zip(self._per_tenant(repetition_penalty), self._per_tenant(presence_penalty),
                                                     self._per_tenant(frequency_penalty), self._per_tenant(logit_bias))]
        cons = [self._constraint_arg(c) for c in self._per_tenant(constraint)]
        sss = [self._stop_sequences_arg(v) for v in self._per_tenant_stop_sequences(stop_sequences)]
        for p_ in prompts:
            self._check_tokens(p_)
            self._check_conversation(p_)
        if bool(self.active_flags.any()):
            raise RuntimeError("a tenant is still generating")
        stops = [self._stops(stop_token_ids[t]) if stop_token_ids else [] for t in range(self.T)]
        for t in range(self.T):
            self._check_constraint(cons[t], stops[t])
        ids, am = dec.prepare(prompts)
        L = ids.shape[1]
        if L > self.Lc:
            raise ValueError("the padded prompts do not fit the KV cache")
        logits = dec.prefill(ids, am, self.cache)
        for t in range(self.T):
            self._context(t, prompts[t], pps[t])
            self._write_constraint(t, cons[t], stops[t])
            self._write_bans(t, bps[t], prompts[t], stops[t])
            self._write_truncation(t, tps[t])
        first = self._first_tokens(logits, sps, L)
        for t in range(self.T):
            self._admit(t, first[t], L, max_new_tokens, stops[t], sps[t], row=t, con=cons[t], ss=sss[t])
            self._kv_start[t] = L - len(prompts[t])

    # ------------------------------------------------------------ stepping
    def _step_once(self):
        dec = self.dec
        x = ops.step_begin_ragged(dec.embed, self.tok, self.cache["valid"], self.pos, self.active_flags)
        logits = dec.forward(self.tok, None, self.cache, None, x=x, ragged=(self.pos, self.active_flags))
        if not (logits.stride(1) == 1 and logits.stride(0) % 8 == 0 and logits.data_ptr() % 16 == 0):
            raise RuntimeError("the lm_head output is not laid out for the step kernel (16-byte aligned rows)")
        raw = logits                                  # (step_logprobs keeps reading the model's own row)
        if self.penalties:                            # counts the token fed in, writes the row the step end chooses from
            logits = ops.step_penalize(raw, self.plogits, self.hist, self.tok, self.active_flags, self.pen, self.bias_id, self.bias_val)
        if self.constraints:                          # masks the (penalised) row by each tenant's automaton state; the state itself moves below
            logits = ops.step_constrain(logits, self.clogits, self.c_state, self.c_off, self.c_tok, self.c_acc, self.stop_ids, self.active_flags)
        if self.bans:                                 # masks what the tenant's own history forbids; wins over a positive bias and a constraint's edge
            logits = ops.step_ban(logits, self.blogits, self.ctx, self.ctx_len, self.out, self.n, self.ban_ngram, self.ban_tok, self.ban_len,
                                  self.ban_min, self.stop_ids, self.active_flags)
        if self.truncation:                           # the last of the masks: cuts the tail of the row the others leave, at the tenant's temperature
            logits = ops.step_truncate(logits, self.tlogits, self.temperature, self.trunc, self.active_flags)
        if self.sampling:
            ops.step_end_sample(logits, self.tok, self.out, self.n, self.pos, self.limit, self.stop_ids, self.active_flags, self.done, self.Lc,
                                self.temperature, self.top_k, self.top_p, self.seed)
        else:
            ops.step_end_ragged(logits, self.tok, self.out, self.n, self.pos, self.limit, self.stop_ids, self.active_flags, self.done, self.Lc)
        if self.logprobs is not None:
            ops.step_logprobs(raw, self.tok, self.n, self.lp_n, self.lp, self.top_id, self.top_lp)
        if self.constraints:                          # follows the token just chosen; a tenant that reaches a final state retires here (reason 8)
            ops.step_constrain_advance(self.tok, self.n, self.c_n, self.c_state, self.c_off, self.c_tok, self.c_next, self.c_acc,
                                       self.active_flags, self.done)
        if self.stop_sequences:                       # LAST: a turn that now ends with one of its sequences retires here (reason 16, OR-ed)
            ops.step_stop_sequences(self.out, self.n, self.ss_n, self.ss_tok, self.ss_len, self.hit, self.hold, self.active_flags, self.done)

    def _state(self):
        st = [self.tok, self.pos, self.n, self.limit, self.active_flags, self.done, self.stop_ids, self.out, self.cache["valid"]]
        if self.logprobs is not None:
            st = st + [self.lp_n]
        if self.penalties:                            # (the warm-up and the capture step would count their token twice otherwise)
            st = st + [self.hist]
        if self.constraints:                          # (... and would advance twice)
            st = st + [self.c_state, self.c_n]
        if self.stop_sequences:                       # (... and would leave a hit of the trial steps behind)
            st = st + [self.ss_n, self.hit, self.hold]
        return st

    def _runner(self):
        """The step as a captured hipGraph on the decoder's capture stream (TenantDecoder._graph_runner's discipline: a warm-up step on that
        stream, the capture, then every state tensor put back).  All request state is device data, so the graph is keyed by the glue switches
        and the kind of session (greedy or sampling: another last launch; its logprobs count: one more launch on its own buffers; penalties:
        one more launch in front of the last; constraints: one more in front of the last and one behind it; stop sequences: one more at the very end, on a table of the
        session's two sizes; bans: one more in front of the step end, on a table of the session's two sizes; truncation: one more in front of the
        step end) alone."""
        dec = self.dec
        key = (dec.fuse_glue, dec.fuse_qkv_norm, dec.fuse_gateup_norm, dec.norm_handoff, FusedDeltaLinear.use_tiled, self.out.data_ptr(),
               self.sampling, self.logprobs, self.penalties, self.constraints)
        if self.stop_sequences:                       # (a session without them keeps the key it had)
            key = key + (True, self.ss_tok.shape[1], self.ss_tok.shape[2])
        if self.bans:                                 # (likewise; the launch keeps no counter, so _state() gains nothing)
            key = key + ("bans", self.ban_tok.shape[1], self.ban_tok.shape[2])
        if self.truncation:                           # (likewise)
            key = key + ("truncation",)
        g = self._graphs.get(key)
        if g is None:
            if dec._capture_stream is None:
                dec._capture_stream = torch.cuda.Stream(device=dec.dev)
            side = dec._capture_stream
            snap = [v.clone() for v in self._state()]
            side.wait_stream(torch.cuda.current_stream(dec.dev))
            with torch.cuda.stream(side):
                self._step_once()
            torch.cuda.current_stream(dec.dev).wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                self._step_once()
            torch.cuda.synchronize(dec.dev)
            for v, s_ in zip(self._state(), snap):
                v.copy_(s_)
            self._graphs[key] = g
        return g.replay

    @torch.no_grad()
    def step(self, k=1, use_graph=True):
        """k ragged steps: every active tenant produces one token per step, at its own position"""
        if k <= 0:
            return
        if not (self.dec.fast_glue and self.dec.step_kernels) or self.dec.prefetch_o:
            raise RuntimeError("fast_glue / step_kernels / prefetch_o were switched after the session was made")
        runner = self._runner() if use_graph else self._step_once
        for _ in range(k):
            runner()

    def run(self, check_every=1, use_graph=True):
        """step until no tenant is active; the host polls the activity flags every check_every steps"""
        while bool(self.active_flags.any()):
            self.step(check_every, use_graph=use_graph)

    def active(self):
        """the activity flags on the host: a list of T bools"""
        return self.active_flags.tolist()

    def result(self, t):
        """(tokens, reason): tenant t's new tokens so far as a 1-D CPU tensor, and why it stopped (0 while it is active)"""
        n = min(int(self.n[t]), self.out.shape[1])
        return self.out[t, :n].cpu(), int(self.done[t])

    def _need_stop_sequences(self):
        if not self.stop_sequences:
            raise ValueError("this session keeps no stop sequences: make it with session(stop_sequences=True)")

    def stop_match(self, t):
        """(index, length) of the stop sequence tenant t's turn ends with -- the index into the request's stop_sequences, the lowest when several
        match, and the number of trailing tokens of result(t) that spell it -- or None when none matched (yet).  ValueError in a session made
        without stop_sequences."""
        self._need_stop_sequences()
        q = int(self.hit[t])
        return None if q < 0 else (q, int(self.ss_len[t, q]))

    def streamable(self, t):
        """n - hold: how many leading tokens of result(t) are safe to show -- the trailing `hold` tokens are the beginning of one of the
        request's stop sequences and may yet be completed.  After a hit hold is 0: whether the matched tokens are shown is the caller's choice
        (stop_match gives their number).  ValueError in a session made without stop_sequences."""
        self._need_stop_sequences()
        n, hold = torch.stack([self.n[t], self.hold[t].long()]).tolist()
        return min(n, self.out.shape[1]) - hold

    def result_logprobs(self, t):
        """(token_logprobs [n], top_ids [n, k], top_logprobs [n, k]) as CPU tensors (float32, int32, float32) for the n tokens result(t) returns:
        entry j is token j's log-probability under the model's own distribution -- softmax of the step's logits at temperature 1, before top-k /
        top-p, whatever the request sampled with -- and the k = session(logprobs=k) most probable tokens of that step with theirs, in descending
        order (include/bitdelta_hip.h, bd_srv_token_logprobs).  In a session(penalties=True) too the entries are computed from the RAW logits of
        the step, not from the penalised row the token was chosen from: a banned token keeps its model probability, and a token forced by a bias
        is reported with the probability the model gave it.  The same holds in a session(constraints=True): the entries describe the RAW row,
        not the masked one, so a token the automaton forbids appears in the lists with its model probability and the chosen token is reported
        with the probability the model gave it, not renormalised over the allowed set.  ValueError in a session made without logprobs."""
        if self.logprobs is None:
            raise ValueError("this session keeps no log-probabilities: make it with session(logprobs=k), 0 <= k <= %d" % ops.LOGPROBS_MAX)
        n = min(int(self.n[t]), self.out.shape[1])
        return self.lp[t, :n].cpu(), self.top_id[t, :n].cpu(), self.top_lp[t, :n].cpu()
