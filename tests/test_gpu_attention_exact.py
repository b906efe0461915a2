"""Exact tests of the two attention kernels: which keys does each attention row see?

prefill_attn_kernel (csrc/bd_attn_prefill.h) and decode_attn_kernel (csrc/bd_serving.h), both through bitdelta_amd.serving_ops, i.e. through
ctypes and the C ABI, both 16-bit dtypes.  The reference is plain fp64 attention written here (scores materialised, boolean mask, torch.softmax
in fp64, matmul) on the same 16-bit inputs; for decode the q heads and the new k are rotated with serving_loop._rope / _rope_tables (the cache-
append check pins that the kernel's RoPE equals that composition bit for bit).  Nothing in the reference uses the kernels' helpers or the oracle.

The randn-based attention tests elsewhere compare one global number; with diffuse softmax weights one key wrongly seen or dropped moves a row by
|v| / n, far under their gates.  Three input classes here make such an error visible:

1. UNIFORM WEIGHTS, INDEX-CODED V.  Q = 0, so every score is exactly 0, every probability exactly 1 and the denominator the exact count of
   visible keys (K is large finite noise: a kernel that did not multiply by Q = 0 would show).  V holds 0 / 1: dims 0..63 one-hot of key % 64,
   dims 64..127 one-hot of (key // 64) % 64, so every accumulator is an exact integer < 2^24 and the output is count_in_bin / count_visible: one
   fp32 quotient and one rounding.  Gate: 1 ulp of the output dtype against the fp64 quotient rounded to that dtype (derived: nothing inexact
   happens before the quotient).  One key too many or too few changes a bin by 1 = at least 64 / n relative; the two codes name the key.
2. NEEDLES.  One visible key per (row, head) scores >= 60 nats above every other visible key, so the output row must EQUAL V[needle] bit for bit
   (every other contribution is below half an fp32 ulp of the accumulator; the needle's own probability differs from 1 by the fp32 rounding of
   score * c, ~1e-5 at <= 200 nats, far below half a 16-bit ulp).  The test first checks ON ITS fp64 REFERENCE that the non-needle weight times
   max |V| is at most 2^-30 of the smallest non-zero |V[needle]|, that the needle scores <= 200 nats and that the margin is >= 60 nats.
   Needles sit at the first / last visible key, next to the diagonal, on both sides of every 32-key boundary (64-key tile edges, 32-key halves,
   32-row ring iterations), of every decode split boundary and right after kv_start; MASKED needles (a higher score and a distinctive V where
   nothing may be seen: query + 1, below kv_start, valid = 0 holes, cache rows past pos) must change no bit.
   Prefill keys are code vectors (7 groups of 17 dims, digit t of key j = (a + b t + c t^2) mod 17 for j = a + 17 b + 289 c, value 16): two
   different keys share at most 2 of 7 groups, so |k|^2 = 1792, own score 158.4 nats, every other key <= 45.3 nats, a masked needle
   (x 1.125) 178.2 nats -- deterministic margins, no luck of a random draw.
3. SCORE RANGE.  randn-based inputs outside the comfortable range -- every score of a row near +150 / -150 nats, scores that rise / fall by 2 nats
   per 64-key tile over the whole length (the rescale runs on every tile), and the diffuse case for contrast -- compared PER ELEMENT:
       |got - ref| <= c * 2u * (P_ref . |V|) + tiny
   (u = 2^-11 fp16 / 2^-8 bf16: one u for the 16-bit probabilities of the PV product, one for the output rounding; tiny = the smallest subnormal).
   This class is NOT meant to catch one-key errors -- at n = 2048 in bf16 one key moves a row by |v| / n ~ 5e-4, a tenth of 2u P|V| -- classes 1
   and 2 catch those.  c covers fp32 accumulation order and the hardware exp2: RANGE_C below, from the measured ratios
   max |err| / (2u P|V|) of stock F.scaled_dot_product_attention with 50 % headroom, never below 1 and never above 4.

Measured on an MI355X, max |err| / (2u P|V|) as "shipped kernel / stock SDPA" (SDPA ran every case, with a boolean attn_mask), fp16 | bf16:
    prefill S = 2048 causal      +150: 0.73 / 0.54 | 0.72 / 0.49    -150: 0.71 / 0.55 | 0.67 / 0.49    rising: 0.76 / 0.49 | 0.65 / 0.50
                                 falling: 0.73 / 0.49 | 0.75 / 0.49    diffuse: 0.88 / 0.50 | 0.84 / 0.49    diffuse S = 4096: 0.68 / 0.48 | 0.73 / 0.48
    prefill S = 2048 not causal  +150: 0.10 / 0.09 | 0.12 / 0.10    -150: 0.12 / 0.12 | 0.13 / 0.13    rising: 0.39 / 0.39 | 0.45 / 0.36
                                 falling: 0.42 / 0.38 | 0.41 / 0.37
    decode (largest of the three geometries)
                                 +150: 0.32 / 0.35 | 0.29 / 0.33    -150: 0.30 / 0.32 | 0.31 / 0.33    rising: 0.30 / 0.42 | 0.30 / 0.30
                                 falling: 0.34 / 0.36 | 0.32 / 0.35    diffuse: 0.32 / 0.32 | 0.30 / 0.40
The largest SDPA ratio is 0.55, so c = max(1, 1.5 x 0.55) = 1 everywhere (RANGE_C); the prefill kernel's own largest ratio is 0.88 (above
SDPA on causal rows, within the bound), the decode kernel (fp32 probabilities) sits with SDPA.
Wall time of the module on an MI355X: 10 s for its 160 cases (12 s with interpreter start; the fp64 references are built on the device).

Every decode case asserts the kernel instantiation it was built to reach through bd_last_attention_form() (nsplit | DEPTH << 8 | MAXS << 16 |
G << 24); the last test asserts that the module's geometries cover all twelve {G} x {DEPTH} x {MAXS} forms and the unsplit launch per dtype.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HD = 128
DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
DT_ID = {torch.float16: "f16", torch.bfloat16: "bf16"}
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}

# class 3 bound c: the largest stock-SDPA ratio measured is 0.55 (table in the module docstring), so clamp(1.5 * ratio, 1, 4) = 1 for both kernels and
# both dtypes: the shipped kernels must stay within 2u P|V| + tiny themselves
RANGE_C = {("prefill", torch.float16): 1.0, ("prefill", torch.bfloat16): 1.0, ("decode", torch.float16): 1.0, ("decode", torch.bfloat16): 1.0}


@pytest.fixture(scope="module")
def bd():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import bitdelta_amd
    from bitdelta_amd import _lib
    _lib.lib()
    return bitdelta_amd


# ------------------------------------------------------------------------------------------------------------------------ helpers
def bits(x):
    return x.contiguous().view(torch.int16)


def ulp_distance(a, b):
    """distance in units of the last place between two finite 16-bit tensors of one dtype (sign-magnitude bits -> monotonic integers)"""
    def mono(x):
        i = bits(x).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (mono(a) - mono(b)).abs()


def first_true(mask):
    return tuple(mask.nonzero()[0].tolist())


def nonzero_randn(shape, dev, g, dtype, scale=1.0):
    v = (torch.randn(shape, device=dev, generator=g) * scale).to(dtype)
    return torch.where(v == 0, torch.ones_like(v), v)


def index_coded_v(n, dev, dtype):
    """[n, 128] of 0 / 1: dims 0..63 one-hot of key % 64, dims 64..127 one-hot of (key // 64) % 64"""
    key = torch.arange(n, device=dev)
    v = torch.zeros(n, HD, device=dev)
    v[key, key % 64] = 1
    v[key, 64 + (key // 64) % 64] = 1
    return v.to(dtype)


def code_vectors(n, dev):
    """[n, 128] fp32 needle codes (module docstring): two different keys below 4913 share at most 2 of their 7 non-zero dims"""
    assert n <= 17 ** 3
    j = torch.arange(n, device=dev)
    a, b, c = j % 17, (j // 17) % 17, (j // 289) % 17
    out = torch.zeros(n, HD, device=dev)
    for t in range(7):
        out[j, 17 * t + (a + b * t + c * t * t) % 17] = 16.0
    return out


def check_needles(sc, ok, p, vd, needle, checked, what):
    """The derivation of class 2, checked on the fp64 reference.  sc / p [heads, rows, keys] scores (nats) and probabilities, ok [rows, keys] or
    [heads, rows, keys] visibility, vd [heads, keys, 128], needle [rows] key index, checked [rows] bool."""
    if not bool(checked.any()):
        return
    idx = needle.view(1, -1, 1).expand(sc.shape[0], -1, 1)
    s_n = sc.gather(2, idx)[..., 0][:, checked]
    assert bool(ok.expand_as(sc).gather(2, idx)[..., 0][:, checked].all()), f"{what}: a needle is not visible in the reference"
    assert float(s_n.max()) <= 200.0, f"{what}: needle score {float(s_n.max())} nats"
    rest = sc.masked_fill(~ok, float("-inf")).scatter(2, idx, float("-inf")).amax(2)[:, checked]
    assert float((s_n - rest).min()) >= 60.0, f"{what}: needle margin {float((s_n - rest).min())} nats"
    w_rest = p.scatter(2, idx, 0.0).sum(2)[:, checked]
    v_n = vd.gather(1, needle.view(1, -1, 1).expand(vd.shape[0], -1, HD)).abs()[:, checked]
    v_min = torch.where(v_n > 0, v_n, torch.full_like(v_n, float("inf"))).amin(2)
    assert bool((w_rest * vd.abs().max() <= 2.0 ** -30 * v_min).all()), f"{what}: non-needle weight too large for bit equality"


def prefill_ref(q, k, v, kv_start, causal, needle=None, checked=None, want_absv=False, what=""):
    """fp64 attention on [B, S, heads, 128] views, one batch entry at a time (the scores of S = 4096 x 8 heads are 1 GB).  kv_start: list of ints or
    None.  Rows without a visible key -> 0.  Returns out [B, S, heads * 128] fp64 (and P . |V| alike)."""
    B, S, H, _ = q.shape
    G = H // k.shape[2]
    keys = torch.arange(S, device=q.device)
    outs, absv = [], []
    for b in range(B):
        qd = q[b].double().transpose(0, 1)
        kd = k[b].double().transpose(0, 1).repeat_interleave(G, dim=0)
        vd = v[b].double().transpose(0, 1).repeat_interleave(G, dim=0)
        sc = qd @ kd.transpose(1, 2) * HD ** -0.5                                       # [H, S, S]
        ok = torch.ones(S, S, dtype=torch.bool, device=q.device)
        if causal:
            ok &= keys[None, :] <= keys[:, None]
        if kv_start is not None:
            ok &= keys[None, :] >= int(kv_start[b])
        p = torch.softmax(sc.masked_fill(~ok, float("-inf")), dim=-1)
        p = torch.where(ok.any(1)[None, :, None], p, torch.zeros_like(p))
        if needle is not None:
            check_needles(sc, ok, p, vd, needle[b], checked[b], f"{what} batch {b}")
        outs.append((p @ vd).transpose(0, 1).reshape(S, H * HD))
        if want_absv:
            absv.append((p @ vd.abs()).transpose(0, 1).reshape(S, H * HD))
        del sc, p
    out = torch.stack(outs)
    return (out, torch.stack(absv)) if want_absv else out


def alloc_qkv(B, S, H, KVH, dtype, layout, dev):
    """q / k / v views [B, S, heads, 128]: the three slices of one fused buffer, or three separately strided tensors"""
    if layout == "fused":
        buf = torch.zeros(B, S, (H + 2 * KVH) * HD, device=dev, dtype=dtype)
        return (buf[..., :H * HD].view(B, S, H, HD), buf[..., H * HD:(H + KVH) * HD].view(B, S, KVH, HD),
                buf[..., (H + KVH) * HD:].view(B, S, KVH, HD))
    q = torch.zeros(B, S, H * HD + 64, device=dev, dtype=dtype)[..., :H * HD].view(B, S, H, HD)
    k = torch.zeros(B, S, KVH * HD, device=dev, dtype=dtype).view(B, S, KVH, HD)
    v = torch.zeros(B, S + 3, KVH * HD, device=dev, dtype=dtype)[:, :S].view(B, S, KVH, HD)
    return q, k, v


def kv_starts(S):
    out = []
    for x in (0, 1, 31, 32, 63, 64, 65, 127, 128, S // 2 - 1, S // 2 + 1, S - 1, S):
        if 0 <= x <= S and x not in out:
            out.append(x)
    return out


HEADS = [(2, 2), (8, 2), (8, 1)]            # heads / kv heads = 1, 4, 8


def run_prefill(q, k, v, ks, causal):
    from bitdelta_amd import serving_ops as ops
    assert ops.prefill_attention_supported(q, k, v)
    kv = None if ks is None else torch.tensor(ks, dtype=torch.int32, device=q.device)
    out = ops.prefill_attention(q, k, v, kv_start=kv, causal=causal)
    B, S, H, _ = q.shape
    assert out.shape == (B, S, H * HD) and out.dtype == q.dtype
    return out


def zero_rows(S, ks, causal, dev):
    """[B, S] bool: query rows without any visible key"""
    i = torch.arange(S, device=dev)
    return torch.stack([(i < x) if causal else torch.full((S,), x >= S, device=dev) for x in ks])


# ------------------------------------------------------------------------------------------------------- class 1, prefill
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("S", [64, 128, 192, 1024, 2048, 4096])
def test_prefill_uniform_weights_index_coded_v(bd, S, causal, dtype):
    """Q = 0, V = index code: every output element is count_in_bin / count_visible within 1 ulp, for EVERY query row -- the first row of a
    128-row workgroup, of a 32-row wave and of a 64-key tile and the row before each are what this test exists for -- and every kv_start of
    kv_starts(S) in one batch (and no kv_start at all); rows without a visible key are exactly zero."""
    dev = DEV
    g = torch.Generator(device=dev).manual_seed(S + 7 * causal)
    for hi, (H, KVH) in enumerate(HEADS):
        layouts = ("fused", "separate") if S <= 192 else (("fused", "separate")[(hi + S // 1024 + causal) % 2],)
        for layout in layouts:
            for ks in (kv_starts(S), None):
                B = len(ks) if ks is not None else 2
                q, k, v = alloc_qkv(B, S, H, KVH, dtype, layout, dev)
                k.copy_((torch.randn(B, S, KVH, HD, device=dev, generator=g) * 200).to(dtype))
                v.copy_(index_coded_v(S, dev, dtype)[None, :, None, :].expand(B, S, KVH, HD))
                out = run_prefill(q, k, v, ks, causal)
                ref = prefill_ref(q, k, v, ks, causal).to(dtype)
                tag = f"S={S} causal={causal} {DT_ID[dtype]} H={H} KVH={KVH} {layout} kv_start={ks}"
                assert bool(torch.isfinite(out).all()), tag
                bad = ulp_distance(out, ref) > 1
                if bool(bad.any()):
                    b, r, c = first_true(bad)
                    raise AssertionError(f"{tag}: batch {b} row {r} head {c // HD} dim {c % HD}: got {float(out[b, r, c])}, "
                                         f"want {float(ref[b, r, c])} (dims < 64: key % 64, dims >= 64: (key // 64) % 64)")
                if ks is not None:
                    z = zero_rows(S, ks, causal, dev)
                    assert bool((bits(out)[z] == 0).all()), f"{tag}: rows without a visible key must be exactly zero"


# ------------------------------------------------------------------------------------------------------- class 2, prefill
def needle_map(place, S, ks, causal):
    """needle key of every query row of one batch entry (numpy int64 [S]) and which rows are checked (bool [S])"""
    i = np.arange(S)
    if causal:
        vis, last = i >= ks, i
    else:
        vis, last = np.full(S, ks < S), np.full(S, S - 1)
    if place == "first":                                   # the first visible key = the first key after kv_start: the maximum is set at the start
        n = np.full(S, min(ks, S - 1))
    elif place == "last":                                  # the last visible key (causal: the diagonal): the maximum jumps at the very end
        n = last
    elif place == "prev":                                  # the key before the last visible one: at a tile edge, the last key of the previous tile
        n = np.maximum(last - 1, min(ks, S - 1))
    elif place == "edges":                                 # both sides of every 32-key boundary, and kv_start / kv_start + 1, spread over the rows
        cand = sorted({x for m in range(S // 32 + 1) for x in (32 * m - 1, 32 * m) if 0 <= x < S} | {x for x in (ks, ks + 1) if x < S})
        c = np.array(cand, dtype=np.int64)
        lo, hi = np.searchsorted(c, ks, "left"), np.searchsorted(c, last, "right")
        cnt = hi - lo
        n = np.where(cnt > 0, c[np.minimum(lo + (i * 37) % np.maximum(cnt, 1), len(c) - 1)], last)
    else:
        raise ValueError(place)
    return n.astype(np.int64), vis


PREFILL_NEEDLE_VARIANTS = ["first", "last", "prev", "edges", "first+poison_below_kv_start", "last+poison_at_query+1:even", "last+poison_at_query+1:odd"]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("S", [64, 128, 192, 1024, 2048, 4096])
def test_prefill_needles_return_their_v_row_bit_for_bit(bd, S, causal, dtype):
    dev = DEV
    g = torch.Generator(device=dev).manual_seed(1000 + S + causal)
    codes = code_vectors(S, dev)
    ks = kv_starts(S)
    B = len(ks)
    for vi, variant in enumerate(PREFILL_NEEDLE_VARIANTS):
        place, _, poison = variant.partition("+")
        if poison.startswith("poison_at_query+1") and not causal:
            continue
        H, KVH = HEADS[(vi + S // 64) % 3]
        layout = ("fused", "separate")[(vi + causal) % 2]
        for kv in ((ks, None) if variant == "last" else (ks,)):
            ksl = ks if kv is not None else [0] * B
            maps = [needle_map(place, S, x, causal) for x in ksl]
            needle = torch.tensor(np.stack([m[0] for m in maps]), device=dev)
            checked = torch.tensor(np.stack([m[1] for m in maps]), device=dev)
            q, k, v = alloc_qkv(B, S, H, KVH, dtype, layout, dev)
            K = codes[None, :, None, :].repeat(B, 1, KVH, 1)
            V = nonzero_randn((B, S, KVH, HD), dev, g, dtype)
            if poison == "poison_below_kv_start":          # every key below kv_start scores above the needle and carries a loud V
                for b, x in enumerate(ksl):
                    K[b, :x] = 1.125 * codes[min(x, S - 1)]
                    V[b, :x] = (500 + 4 * torch.randn(x, KVH, HD, device=dev, generator=g)).to(dtype)
            elif poison:                                   # rows of one parity: key row + 1 scores above the row's own (diagonal) needle
                par = 0 if poison.endswith("even") else 1
                rows = torch.arange(par, S - 1, 2, device=dev)
                K[:, rows + 1] = 1.125 * codes[rows][None, :, None, :]
                V[:, rows + 1] = (500 + 4 * torch.randn(B, rows.numel(), KVH, HD, device=dev, generator=g)).to(dtype)
                checked &= (torch.arange(S, device=dev) % 2 == par)[None]
            k.copy_(K.to(dtype))
            v.copy_(V)
            q.copy_(codes[needle][:, :, None, :].expand(B, S, H, HD).to(dtype))
            tag = f"S={S} causal={causal} {DT_ID[dtype]} H={H} KVH={KVH} {layout} {variant} kv_start={kv}"
            ref = prefill_ref(q, k, v, kv, causal, needle=needle, checked=checked, what=tag)
            out = run_prefill(q, k, v, kv, causal).view(B, S, H, HD)
            want = torch.gather(v, 1, needle.view(B, S, 1, 1).expand(B, S, KVH, HD)).repeat_interleave(H // KVH, dim=2)
            chk = checked[:, :, None, None].expand(B, S, H, HD)
            assert bool(((bits(ref.view(B, S, H, HD).to(dtype)) == bits(want)) | ~chk).all()), f"{tag}: the fp64 reference itself does not return V[needle]"
            bad = (bits(out) != bits(want)) & chk
            if bool(bad.any()):
                b, r, h, d = first_true(bad)
                raise AssertionError(f"{tag}: batch {b} (kv_start {ksl[b]}) row {r} head {h} dim {d}: got {float(out[b, r, h, d])}, "
                                     f"V[needle = key {int(needle[b, r])}] = {float(want[b, r, h, d])}")
            z = zero_rows(S, ksl, causal, dev)
            assert bool((bits(out)[z] == 0).all()), f"{tag}: rows without a visible key must be exactly zero"


# ------------------------------------------------------------------------------------------------------- decode: geometry and reference
# name -> (tenants, heads, kv heads, cache length, the instantiation the geometry is built to reach: (DEPTH, MAXS, split?))
#   DEPTH = 4 needs Lc > 2048; MAXS = 16 needs nsplit > 4, so few (tenant, kv head) pairs; the unsplit launch needs Lc < 256
DECODE_GEOMS = {}
for _g, (_h1, _k1, _h16, _k16) in {1: (3, 3, 1, 1), 4: (12, 3, 4, 1), 8: (24, 3, 8, 1)}.items():
    DECODE_GEOMS[f"unsplit-G{_g}"] = (3, _h16 * 2, _k16 * 2, 160, (2, 4, False))
    DECODE_GEOMS[f"depth2-maxs4-G{_g}"] = (6, _h1, _k1, 640, (2, 4, True))
    DECODE_GEOMS[f"depth2-maxs16-G{_g}"] = (6, _h16, _k16, 1024, (2, 16, True))
    DECODE_GEOMS[f"depth4-maxs4-G{_g}"] = (6, _h1, _k1, 2304, (4, 4, True))
    DECODE_GEOMS[f"depth4-maxs16-G{_g}"] = (6, _h16, _k16, 2304, (4, 16, True))

_FORMS_SEEN = {dt: set() for dt in DTYPES}


def split_count(T, kvh, Lc, cus):
    """attn_splits() of csrc/bd_api.hip restated: 4 splits, doubled up to 16 while the launch covers at most a quarter of the CUs"""
    if Lc < 256:
        return 1
    ns = 4
    while ns * 2 <= 16 and T * kvh * ns * 4 <= cus and ns * 2 * 32 <= Lc:
        ns *= 2
    return ns


def per_split(pos, ns):
    """key rows per split (bd_serving.h): whole iterations of 32 rows"""
    return ((pos + 1 + ns - 1) // ns + 31) // 32 * 32


def expected_form(name):
    T, heads, kvh, Lc, (depth, maxs, split) = DECODE_GEOMS[name]
    ns = split_count(T, kvh, Lc, torch.cuda.get_device_properties(0).multi_processor_count)
    assert (ns > 1) == split and (4 if ns <= 4 else 16) == maxs and (2 if Lc <= 2048 else 4) == depth, f"{name}: geometry does not reach its form"
    return ns, ns | depth << 8 | maxs << 16 | (heads // kvh) << 24


def run_decode(name, qkv, cos, sin, kc, vc, valid, pos, dtype):
    """the launch on clones of the caches; asserts the instantiation; returns out and the updated caches / mask"""
    from bitdelta_amd import _lib, serving_ops as ops
    T, heads, kvh, Lc, _ = DECODE_GEOMS[name]
    kc, vc, valid = kc.clone(), vc.clone(), valid.clone()
    pidx = torch.tensor([pos], device=qkv.device)
    out = ops.decode_attention(qkv, cos, sin, kc, vc, valid, pidx, heads, kvh)
    form, (_, want) = _lib.lib().bd_last_attention_form(), expected_form(name)
    assert form == want, f"{name}: bd_last_attention_form() = {form:#x}, built to reach {want:#x}"
    _FORMS_SEEN[dtype].add(form)
    return out, kc, vc, valid


def decode_ref(qkv, cos, sin, kc, vc, valid, pos, heads, kvh):
    """fp64 single-token attention: RoPE of the q heads and the new k by serving_loop._rope, cache append, mask = valid (with valid[:, pos] set),
    softmax, matmul.  Returns out [T, 1, heads * 128] fp64, the updated caches and mask, scores and probabilities [T, heads, 1, Lc], P . |V|."""
    from bitdelta_amd.serving_loop import _rope
    T = qkv.shape[0]
    pidx = torch.tensor([pos], device=qkv.device)
    q, k, v = qkv.split([heads * HD, kvh * HD, kvh * HD], dim=-1)
    q = _rope(q.view(T, 1, heads, HD).transpose(1, 2), cos[pidx], sin[pidx])
    k = _rope(k.view(T, 1, kvh, HD).transpose(1, 2), cos[pidx], sin[pidx])
    kr, vr, vm = kc.clone(), vc.clone(), valid.clone()
    kr.index_copy_(2, pidx, k)
    vr.index_copy_(2, pidx, v.view(T, 1, kvh, HD).transpose(1, 2))
    vm[:, pos] = True
    G = heads // kvh
    vd = vr.double().repeat_interleave(G, dim=1)
    sc = (q.double() @ kr.double().repeat_interleave(G, dim=1).transpose(2, 3)) / math.sqrt(HD)
    ok = vm[:, None, None, :].expand_as(sc)
    p = torch.softmax(sc.masked_fill(~ok, float("-inf")), dim=-1)
    flat = lambda x: x.transpose(1, 2).reshape(T, 1, heads * HD)
    return flat(p @ vd), kr, vr, vm, sc, p, flat(p @ vd.abs())


def decode_positions(ns, Lc):
    """pos in {0, 1, 31, 32, 33, Lc - 1} and, for every split boundary c * per_split(pos), the largest pos just below / at / just above it"""
    out = {0, 1, 31, 32, 33, Lc - 1}
    if ns > 1:
        best = {}
        for pos in range(Lc):
            per = per_split(pos, ns)
            c, r = divmod(pos, per)
            if r == per - 1 and c < ns - 1:
                best[(c + 1, "below")] = pos
            if c >= 1 and r in (0, 1):
                best[(c, "at" if r == 0 else "above")] = pos
        out |= set(best.values())
    return sorted(out)


def padded_valid(T, Lc, pos, ns, dev):
    """valid [T, Lc] before the launch (rows >= pos are 0) with a different left padding per tenant: none; pos itself (only the new token is
    visible); short + pseudo-random isolated holes; ending exactly on a split boundary; longer than a whole split (a block contributes
    nothing); holes on every 32-row boundary and at pos - 1"""
    per = per_split(pos, ns)
    c = pos // per
    l = torch.arange(Lc, device=dev)
    valid = torch.zeros(T, Lc, dtype=torch.bool, device=dev)
    for t in range(T):
        kind = t % 6
        pad = (0, pos, min(5, pos), per * max(1, c // 2) if per <= pos else pos // 2,
               per * c + (pos - per * c) // 2 if c >= 1 else min(pos, 40), min(1, pos))[kind]
        row = (l >= pad) & (l < pos)
        if kind == 2:
            row &= ((l * 2654435761) >> 16) % 4 != 0
        if kind == 5:
            row &= (l % 32 != 0) & (l != pos - 1)
        valid[t] = row
    return valid


# ------------------------------------------------------------------------------------------------------- class 1, decode
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("name", list(DECODE_GEOMS))
def test_decode_uniform_weights_index_coded_v(bd, name, dtype):
    """q heads = 0 (RoPE of 0 is 0), V = index code of the cache row (the new token's v carries the code of pos; rows past pos and rows with
    valid = 0 carry theirs, so they show if read): count_in_bin / count_visible within 1 ulp; caches and valid[:, pos] updated bit-exactly"""
    from bitdelta_amd.serving_loop import _rope_tables
    dev = DEV
    T, heads, kvh, Lc, _ = DECODE_GEOMS[name]
    ns, _ = expected_form(name)
    g = torch.Generator(device=dev).manual_seed(Lc + heads)
    cos, sin = _rope_tables(Lc, HD, dev, dtype)
    kc = (torch.randn(T, kvh, Lc, HD, device=dev, generator=g) * 50).to(dtype)
    code = index_coded_v(Lc, dev, dtype)
    vc = code[None, None].expand(T, kvh, Lc, HD).contiguous()
    for pos in decode_positions(ns, Lc):
        valid = padded_valid(T, Lc, pos, ns, dev)
        qkv = torch.zeros(T, 1, (heads + 2 * kvh) * HD, device=dev, dtype=dtype)
        qkv[:, 0, heads * HD:(heads + kvh) * HD] = (torch.randn(T, kvh * HD, device=dev, generator=g) * 50).to(dtype)
        qkv[:, 0, (heads + kvh) * HD:] = code[pos].repeat(kvh)
        out, k1, v1, m1 = run_decode(name, qkv, cos, sin, kc, vc, valid, pos, dtype)
        ref, kr, vr, vm, _, _, _ = decode_ref(qkv, cos, sin, kc, vc, valid, pos, heads, kvh)
        ref = ref.to(dtype)
        tag = f"{name} {DT_ID[dtype]} pos={pos} nsplit={ns} per_split={per_split(pos, ns)}"
        assert torch.equal(bits(k1), bits(kr)) and torch.equal(bits(v1), bits(vr)) and torch.equal(m1, vm), f"{tag}: cache append"
        bad = ulp_distance(out, ref) > 1
        if bool(bad.any()):
            t, _, c = first_true(bad)
            raise AssertionError(f"{tag}: tenant {t} head {c // HD} dim {c % HD}: got {float(out[t, 0, c])}, want {float(ref[t, 0, c])} "
                                 f"(dims < 64: row % 64, dims >= 64: (row // 64) % 64; {int(vm[t].sum())} visible rows)")


# ------------------------------------------------------------------------------------------------------- class 2, decode
def needle_rows(pos, ns):
    """candidate needle rows: first and last cache row, the new token, both sides of every split boundary and of every 32-row ring iteration"""
    per = per_split(pos, ns)
    cand = {0, pos, pos - 1}
    cand |= {x for c in range(1, ns) for x in (c * per - 1, c * per)}
    cand |= {x for m in range(1, pos // 32 + 1) for x in (32 * m - 1, 32 * m)}
    return sorted(x for x in cand if 0 <= x <= pos)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("name", list(DECODE_GEOMS))
def test_decode_needles_return_their_v_row_bit_for_bit(bd, name, dtype):
    """The heads of a group share q (|q|^2 = 1500: 133 nats), the needle row holds the rotated q itself (the new token: k = q in qkv), every
    other row is small.  Every launch also carries MASKED needles (1.125 x the rotated q, V ~ 1000): the row below the left padding and row
    0, valid = 0 holes next to the needle and 32 rows from it, row pos + 1 and the last cache row.  In every other launch the left padding ends
    at the needle (the needle is the first visible key; at needle = pos only the new token is visible)."""
    from bitdelta_amd.serving_loop import _rope, _rope_tables
    dev = DEV
    T, heads, kvh, Lc, _ = DECODE_GEOMS[name]
    G = heads // kvh
    ns, _ = expected_form(name)
    g = torch.Generator(device=dev).manual_seed(2 * Lc + heads)
    cos, sin = _rope_tables(Lc, HD, dev, dtype)
    kc0 = (torch.randn(T, kvh, Lc, HD, device=dev, generator=g) * 0.05).to(dtype)
    vc0 = nonzero_randn((T, kvh, Lc, HD), dev, g, dtype)
    positions = [Lc - 1, 33]
    if ns > 1:
        positions.insert(1, max((p for p in range(Lc) if p % per_split(p, ns) == 0 and p // per_split(p, ns) == ns // 2), default=Lc // 2))
    for pos in positions:
        cand = needle_rows(pos, ns)
        pidx = torch.tensor([pos], device=dev)
        for launch in range((len(cand) + T - 1) // T):
            nd = [cand[(launch * T + t) % len(cand)] for t in range(T)]
            qraw = torch.randn(T, kvh, HD, device=dev, generator=g)
            qraw = (qraw * (1500 ** 0.5 / qraw.norm(dim=-1, keepdim=True))).to(dtype)
            qrot = _rope(qraw.view(T, 1, kvh, HD).transpose(1, 2), cos[pidx], sin[pidx])[:, :, 0]           # [T, kvh, 128], 16-bit
            qkv = torch.empty(T, 1, (heads + 2 * kvh) * HD, device=dev, dtype=dtype)
            qkv[:, 0, :heads * HD] = qraw.repeat_interleave(G, dim=1).reshape(T, heads * HD)
            knew = (torch.randn(T, kvh, HD, device=dev, generator=g) * 0.05).to(dtype)
            qkv[:, 0, (heads + kvh) * HD:] = nonzero_randn((T, kvh * HD), dev, g, dtype)
            kc, vc = kc0.clone(), vc0.clone()
            valid = torch.zeros(T, Lc, dtype=torch.bool, device=dev)
            poison_rows = []
            for t in range(T):
                pad = nd[t] if (launch + t) % 2 else 0
                valid[t, pad:pos] = True
                masked = {pad - 1, 0} if pad > 0 else set()
                masked |= {x for x in (pos + 1, Lc - 1) if pos < x < Lc}
                holes = [x for x in (nd[t] + 1, nd[t] - 1) if pad <= x < pos][:1] + [x for x in (nd[t] + 32, nd[t] - 32) if pad <= x < pos][:1]
                for x in holes:
                    valid[t, x] = False
                masked |= set(holes)
                poison_rows.append(sorted(masked))
                if nd[t] == pos:
                    knew[t] = qraw[t]
                else:
                    kc[t, :, nd[t]] = qrot[t]
                for x in masked:
                    kc[t, :, x] = (1.125 * qrot[t].float()).to(dtype)
                    vc[t, :, x] = (1000 + 8 * torch.randn(kvh, HD, device=dev, generator=g)).to(dtype)
            qkv[:, 0, heads * HD:(heads + kvh) * HD] = knew.reshape(T, kvh * HD)
            tag = f"{name} {DT_ID[dtype]} pos={pos} nsplit={ns} per_split={per_split(pos, ns)} needles={nd} masked needles={poison_rows}"
            ref, kr, vr, vm, sc, p, _ = decode_ref(qkv, cos, sin, kc, vc, valid, pos, heads, kvh)
            needle = torch.tensor(nd, device=dev)
            for t in range(T):
                check_needles(sc[t], vm[t][None, None, :].expand(heads, 1, Lc), p[t], vr[t].double().repeat_interleave(G, dim=0), needle[t:t + 1],
                              torch.ones(1, dtype=torch.bool, device=dev), f"{tag} tenant {t}")
            want = torch.stack([vr[t, :, nd[t]] for t in range(T)]).repeat_interleave(G, dim=1).reshape(T, 1, heads * HD)
            assert torch.equal(bits(ref.to(dtype)), bits(want)), f"{tag}: the fp64 reference itself does not return V[needle]"
            out, k1, v1, m1 = run_decode(name, qkv, cos, sin, kc, vc, valid, pos, dtype)
            assert torch.equal(bits(k1), bits(kr)) and torch.equal(bits(v1), bits(vr)) and torch.equal(m1, vm), f"{tag}: cache append"
            bad = bits(out) != bits(want)
            if bool(bad.any()):
                t, _, c = first_true(bad)
                raise AssertionError(f"{tag}: tenant {t} head {c // HD} dim {c % HD}: got {float(out[t, 0, c])}, V[needle] = {float(want[t, 0, c])}")


# ------------------------------------------------------------------------------------------------------- class 3
RANGE_CASES = ["plus150", "minus150", "rising", "falling", "diffuse"]


def range_ratio(got, ref, absv, dtype):
    """max over the elements of (|got - ref| - tiny) / (2u P|V|); elements nothing contributes to must be exactly zero"""
    err = (got.double() - ref).abs()
    dead = absv == 0
    assert bool((err[dead] == 0).all())
    r = ((err - TINY[dtype]).clamp_min(0) / (2 * UNIT[dtype] * absv.clamp_min(1e-300)))[~dead]
    return float(r.max()) if r.numel() else 0.0


def shift_column(case, n, dev):
    """(a, b[n]): with q[0] = a and k_j[0] = b_j (no noise in that dim) every score moves by a * b_j / sqrt(128) nats: +-150.4, or +-2 per 64 keys"""
    j = torch.arange(n, device=dev)
    if case == "plus150":
        return 41.25, torch.full((n,), 41.25, device=dev)
    if case == "minus150":
        return 41.25, torch.full((n,), -41.25, device=dev)
    if case == "rising":
        return 16.0, (j // 64).float() * (2 * math.sqrt(HD) / 16)
    if case == "falling":
        return 16.0, (j // 64).float() * (-2 * math.sqrt(HD) / 16)
    return None, None


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("case,S,causal", [(c, 2048, True) for c in RANGE_CASES] + [(c, 2048, False) for c in RANGE_CASES[:4]] + [("diffuse", 4096, True)])
def test_prefill_score_range_per_element(bd, case, S, causal, dtype):
    import torch.nn.functional as F
    dev = DEV
    B, H, KVH = 2, 8, 2
    ks = [0, 333]
    g = torch.Generator(device=dev).manual_seed(S + RANGE_CASES.index(case))
    q, k, v = alloc_qkv(B, S, H, KVH, dtype, "fused", dev)
    Q, K = torch.randn(B, S, H, HD, device=dev, generator=g), torch.randn(B, S, KVH, HD, device=dev, generator=g)
    a, col = shift_column(case, S, dev)
    if a is not None:
        Q[..., 0] = a
        K[..., 0] = col[None, :, None]
    q.copy_(Q.to(dtype)); k.copy_(K.to(dtype)); v.copy_(torch.randn(B, S, KVH, HD, device=dev, generator=g).to(dtype))
    ref, absv = prefill_ref(q, k, v, ks, causal, want_absv=True)
    out = run_prefill(q, k, v, ks, causal)
    assert bool(torch.isfinite(out).all())
    ratio = range_ratio(out, ref, absv, dtype)
    ratio_sdpa = None
    try:
        keys = torch.arange(S, device=dev)
        ok = keys[None, None, :] >= torch.tensor(ks, device=dev)[:, None, None]
        if causal:
            ok = ok & (keys[None, :] <= keys[:, None])[None]
        sd = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), attn_mask=ok[:, None].expand(B, 1, S, S),
                                            enable_gqa=True).transpose(1, 2).reshape(B, S, H * HD)
        live = ok.any(-1).expand(B, S)[:, :, None].expand_as(sd)           # SDPA returns NaN for rows without a visible key
        ratio_sdpa = range_ratio(torch.where(live, sd, torch.zeros_like(sd)), ref, absv, dtype)
    except RuntimeError as e:                                                # stock SDPA cannot run the case: nothing to compare with
        print(f"SDPA did not run prefill/{case}: {e}")
    print(f"RANGE prefill {case} S={S} causal={causal} {DT_ID[dtype]}: kernel {ratio:.3f} sdpa {ratio_sdpa}")
    assert ratio <= RANGE_C[("prefill", dtype)], (case, S, causal, dtype, ratio, ratio_sdpa)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("name", ["depth4-maxs4-G4", "depth2-maxs16-G8", "depth4-maxs16-G1"])
@pytest.mark.parametrize("case", RANGE_CASES)
def test_decode_score_range_per_element(bd, case, name, dtype):
    """The shift column lives in the ROTATED space: raw dims (0, 64) of the q heads and of the new k are (a cos, -a sin) of the position's first
    RoPE angle, which RoPE turns into (a, ~0); the cache rows hold (b_l, noise)."""
    import torch.nn.functional as F
    from bitdelta_amd.serving_loop import _rope_tables
    dev = DEV
    T, heads, kvh, Lc, _ = DECODE_GEOMS[name]
    pos = Lc - 1
    ns, _ = expected_form(name)
    g = torch.Generator(device=dev).manual_seed(Lc + heads + RANGE_CASES.index(case))
    cos, sin = _rope_tables(Lc, HD, dev, dtype)
    kc = torch.randn(T, kvh, Lc, HD, device=dev, generator=g)
    qkv = torch.randn(T, heads + 2 * kvh, HD, device=dev, generator=g)
    a, col = shift_column(case, Lc, dev)
    if a is not None:
        kc[..., 0] = col
        th = float(pos)                                                       # angle of dims (0, 64): pos * base^0
        qkv[:, :heads, 0], qkv[:, :heads, 64] = a * math.cos(th), -a * math.sin(th)
        qkv[:, heads:heads + kvh, 0], qkv[:, heads:heads + kvh, 64] = float(col[pos]) * math.cos(th), -float(col[pos]) * math.sin(th)
    kc = kc.to(dtype)
    vc = torch.randn(T, kvh, Lc, HD, device=dev, generator=g).to(dtype)
    qkv = qkv.to(dtype).view(T, 1, (heads + 2 * kvh) * HD)
    valid = padded_valid(T, Lc, pos, ns, dev)
    valid[1] = valid[0]                                                       # (tenant 1 of padded_valid sees the new token only)
    ref, kr, vr, vm, sc, _, absv = decode_ref(qkv, cos, sin, kc, vc, valid, pos, heads, kvh)
    out, k1, v1, m1 = run_decode(name, qkv, cos, sin, kc, vc, valid, pos, dtype)
    assert torch.equal(bits(k1), bits(kr)) and torch.equal(bits(v1), bits(vr)) and torch.equal(m1, vm)
    assert bool(torch.isfinite(out).all())
    ratio = range_ratio(out, ref, absv, dtype)
    ratio_sdpa = None
    try:
        from bitdelta_amd.serving_loop import _rope
        pidx = torch.tensor([pos], device=dev)
        qr = _rope(qkv[..., :heads * HD].view(T, 1, heads, HD).transpose(1, 2), cos[pidx], sin[pidx])
        G = heads // kvh
        sd = F.scaled_dot_product_attention(qr, kr.repeat_interleave(G, dim=1), vr.repeat_interleave(G, dim=1),
                                            attn_mask=vm[:, None, None, :]).transpose(1, 2).reshape(T, 1, heads * HD)
        ratio_sdpa = range_ratio(sd, ref, absv, dtype)
    except RuntimeError as e:
        print(f"SDPA did not run decode/{case}: {e}")
    vis = sc.masked_fill(~vm[:, None, None, :], float("nan"))
    print(f"RANGE decode {case} {name} {DT_ID[dtype]}: kernel {ratio:.3f} sdpa {ratio_sdpa} (scores {float(vis.nan_to_num(1e9).min()):.1f} .. "
          f"{float(vis.nan_to_num(-1e9).max()):.1f} nats)")
    assert ratio <= RANGE_C[("decode", dtype)], (case, name, dtype, ratio, ratio_sdpa)


# ------------------------------------------------------------------------------------------------------- class 4
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_decode_geometries_cover_every_instantiation(bd, dtype):
    """One launch per geometry of DECODE_GEOMS (so the test stands alone), together with what the cases above recorded: all twelve
    {G 1, 4, 8} x {DEPTH 2, 4} x {MAXS 4, 16} split forms and the unsplit launch of every G ran, and nothing else did"""
    from bitdelta_amd.serving_loop import _rope_tables
    dev = DEV
    for name, (T, heads, kvh, Lc, _) in DECODE_GEOMS.items():
        cos, sin = _rope_tables(Lc, HD, dev, dtype)
        kc = torch.randn(T, kvh, Lc, HD, device=dev).to(dtype)
        valid = torch.zeros(T, Lc, dtype=torch.bool, device=dev)
        valid[:, :Lc - 1] = True
        qkv = torch.randn(T, 1, (heads + 2 * kvh) * HD, device=dev).to(dtype)
        run_decode(name, qkv, cos, sin, kc, kc, valid, Lc - 1, dtype)            # asserts its form and records it
    seen = {(f >> 24, (f >> 8) & 0xFF, (f >> 16) & 0xFF, (f & 0xFF) > 1) for f in _FORMS_SEEN[dtype]}
    want = {(G, d, m, True) for G in (1, 4, 8) for d in (2, 4) for m in (4, 16)} | {(G, 2, 4, False) for G in (1, 4, 8)}
    assert seen == want, (sorted(want - seen), sorted(seen - want))
