"""fp64 models of the decode-step glue arithmetic of csrc/bd_serving.h -- RMSNorm (per-tenant weight), residual add + RMSNorm, SwiGLU, RoPE --
and the ONE acceptance rule the tests of these kernels share (tests/test_glue_ref_host.py without a GPU, tests/test_gpu_glue_exact.py with one).

A model states the rounding points the kernels document (`w * round16(x * rs)`, `round16(silu(g)) * u`, `round16(round16(x cos) + x' sin)`: the
order of the HF modules they replace) and computes everything else exactly: float64 sums of squares, float64 exp, one rounding per documented
point and straight from float64 to the 16-bit format (never through float32: `tensor.double().to(torch.bfloat16)` rounds twice).  A kernel that
computes the same thing in fp32 lands on the model's 16-bit value except where its fp32 result sits within an fp32 ulp of a 16-bit rounding
boundary, so nearly every element is bit-equal and the rest is one or two ulps off; a kernel that rounds at other points, drops eps, or divides
by the wrong H is a few ulps off on a LARGE share of the elements.  accept() therefore asks for both: a per-element ulp limit and a minimum share
of bit-equal elements.

numpy float64 throughout; 16-bit tensors cross over with to64() / bits16()."""
import collections

import numpy as np
import torch

#            mantissa bits, smallest normal exponent, largest exponent
_FORMAT = {torch.float16: (10, -14, 15), torch.bfloat16: (7, -126, 127)}


def to64(t):
    """a torch tensor (any float dtype, any device) as a numpy float64 array -- exact"""
    return t.detach().cpu().double().numpy()


def from_bits(bits, dtype):
    """16-bit patterns (any integer array) -> torch tensor of `dtype`"""
    return torch.from_numpy(np.asarray(bits).astype(np.uint16).view(np.int16).copy()).view(dtype)


def _quantum_and_exponent(a, dtype):
    """for |values| a (finite, >= 0): the format's spacing at a (the subnormal quantum below the smallest normal) and the clamped exponent"""
    mbits, emin, _ = _FORMAT[dtype]
    _, e = np.frexp(a)                                      # a = m * 2^e, m in [0.5, 1)  ->  a in [2^(e-1), 2^e)
    eq = np.where(a == 0, emin, np.maximum(e.astype(np.int64) - 1, emin))
    return np.ldexp(1.0, (eq - mbits).astype(np.int64)), eq


def _round16_bits(v64, dtype):
    mbits, emin, emax = _FORMAT[dtype]
    v = np.asarray(v64, dtype=np.float64)
    nan, inf = np.isnan(v), np.isinf(v)
    a = np.where(nan | inf, 0.0, np.abs(v))
    q, eq = _quantum_and_exponent(a, dtype)
    r = np.rint(a / q)                                      # a / q is exact (a power-of-two scaling below 2^(mbits + 1)); rint = nearest, ties to even
    # r in [2^mbits, 2^(mbits+1)] for a normal result, below 2^mbits for a subnormal one: the pattern is the exponent field's base plus r, and
    # a carry out of the mantissa (r = 2^(mbits+1), or a subnormal rounding up to the smallest normal) lands in the next exponent by itself
    bits = (eq - emin) * (1 << mbits) + r.astype(np.int64)
    inf_bits = (emax - emin + 2) << mbits
    bits = np.where(inf, inf_bits, np.minimum(bits, inf_bits))          # past the largest finite value: inf
    bits = np.where(nan, inf_bits | (1 << (mbits - 1)), bits)
    return (bits | np.where(np.signbit(v) & ~nan, 0x8000, 0)).astype(np.uint16)


def _decode_bits(bits, dtype):
    mbits, emin, emax = _FORMAT[dtype]
    b = np.asarray(bits).astype(np.int64)
    field, man = (b & 0x7fff) >> mbits, b & ((1 << mbits) - 1)
    mag = np.where(field == 0, np.ldexp(man.astype(np.float64), emin - mbits),
                   np.ldexp((man + (1 << mbits)).astype(np.float64), (field - 1 + emin - mbits).astype(np.int64)))
    with np.errstate(invalid="ignore"):
        mag = np.where(field == emax - emin + 2, np.where(man == 0, np.inf, np.nan), mag)
    return np.where(b & 0x8000, -mag, mag)


def round16(v64, dtype):
    """float64 -> nearest fp16 / bf16 value (ties to even, subnormals of the format kept, overflow to inf), returned as float64"""
    return _decode_bits(_round16_bits(v64, dtype), dtype)


def bits16(v64, dtype):
    """the 16-bit pattern of round16(v64) (of v64 itself where it already is a value of the format); NaN -> the quiet NaN"""
    return _round16_bits(v64, dtype)


def ulp16(v64, dtype):
    """spacing of the format at |v|: 2^(e - mantissa bits), the subnormal quantum below the smallest normal; the top binade's for inf; NaN for NaN"""
    mbits, _, emax = _FORMAT[dtype]
    v = np.asarray(v64, dtype=np.float64)
    nan, inf = np.isnan(v), np.isinf(v)
    q, _ = _quantum_and_exponent(np.where(nan | inf, 0.0, np.abs(v)), dtype)
    return np.where(nan, np.nan, np.where(inf, np.ldexp(1.0, emax - mbits), q))


# ------------------------------------------------------------------------------------------------------------------------ models
def rmsnorm(x, w, eps, rows_per_tenant, dtype):
    """x [rows, H], w [T, H] (values of `dtype` as float64) -> (y, a):  rs = 1 / sqrt(sum(x^2) / H + eps), a = round16(x rs),
    y = round16(a w[row // rows_per_tenant]).  eps is the fp32 number the kernel is handed."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    rows, H = x.shape
    with np.errstate(all="ignore"):
        rs = 1.0 / np.sqrt((x * x).sum(-1, keepdims=True) / H + float(np.float32(eps)))
        a = round16(x * rs, dtype)
        wr = w[np.arange(rows) // rows_per_tenant]
        return round16(a * wr, dtype), a


def add_rmsnorm(resid, y32, w, eps, rows_per_tenant, dtype):
    """x = round16(resid + round16(y32)), then rmsnorm(x) -> (x, h, a)"""
    with np.errstate(all="ignore"):
        x = round16(np.asarray(resid, np.float64) + round16(y32, dtype), dtype)
    h, a = rmsnorm(x, w, eps, rows_per_tenant, dtype)
    return x, h, a


def swiglu(g, u, dtype):
    """a = round16(g / (1 + exp(-g))), y = round16(a u) -> (y, a)"""
    g, u = np.asarray(g, np.float64), np.asarray(u, np.float64)
    with np.errstate(all="ignore"):
        a = round16(g / (1.0 + np.exp(-g)), dtype)
        return round16(a * u, dtype), a


def rope_tables(length, base=10000.0, dim=128):
    """HF rotary tables from first principles, unrounded float64 [length, dim]: angle(p, i) = p * base^(-2 i / dim) for the pair (i, i + dim/2);
    cos(angle) in both halves; the rotate-half sign written out: -sin(angle) for dims 0 .. dim/2 - 1, +sin(angle) for dims dim/2 .. dim - 1.
    Returns (cos, sin_signed, angle)."""
    i = np.arange(dim // 2, dtype=np.float64)
    ang = np.arange(length, dtype=np.float64)[:, None] * base ** (-2.0 * i / dim)[None, :]
    return (np.concatenate([np.cos(ang), np.cos(ang)], -1), np.concatenate([-np.sin(ang), np.sin(ang)], -1), np.concatenate([ang, ang], -1))


def rope(x, cos16, sin16, pos, dtype):
    """x [rows, heads, 128]; cos16 / sin16 [L, 128]: the 16-bit tables as given (sign folded into sin); pos [rows] ->
    (out, inter):  inter = round16(x[d] cos[d]),  out[d] = round16(inter + x[d +- 64] sin[d])"""
    x = np.asarray(x, np.float64)
    c, s = np.asarray(cos16, np.float64)[np.asarray(pos)][:, None, :], np.asarray(sin16, np.float64)[np.asarray(pos)][:, None, :]
    rot = np.concatenate([x[..., 64:], x[..., :64]], -1)
    with np.errstate(all="ignore"):
        inter = round16(x * c, dtype)
        return round16(inter + rot * s, dtype), inter


# ------------------------------------------------------------------------------------------------------------------------ the acceptance rule
NORM_LIMITS = (2, 0.99)         # one ulp in a = round16(x rs) is up to 2^-10 (fp16) / 2^-7 (bf16) relative: up to two ulps of y
SWIGLU_LIMITS = (2, 0.99)       # the same structure: one ulp in round16(silu(g)), times u
ROPE_LIMITS = (1, 0.999)        # products exact in fp32; only the final sum is rounded twice (fp32, then 16 bits)

Verdict = collections.namedtuple("Verdict", "ok worst_ulp equal_share first_bad n_bad worst_ulp_normal")


def _ordered(bits):
    """sign-magnitude pattern -> monotonic integer (tests/test_gpu_parity.ulp_diff's mapping; -0 and +0 both 0)"""
    b = np.asarray(bits).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7fff), b & 0x7fff)


def accept(got16, model64, inter64, mult64, dtype, max_ulp, min_equal):
    """got16: the kernel's output (torch tensor of `dtype`); model64 / inter64 / mult64: the model's output, its rounded intermediate and what
    that intermediate is multiplied by (arrays broadcastable to got16's shape; mult64 = 1 where it is added to).

    An element passes when it is within max_ulp ulps of the model (distance of the monotonic integers), OR within
    ulp16(inter) |mult| + ulp16(model) of it: the intermediate one ulp away, carried through the multiplication, plus one ulp of the result --
    wider than max_ulp ulps only where the intermediate is subnormal (its ulp is no longer 2^-mantissa of it).  NaN passes against NaN only;
    -0 equals +0.  Over the whole tensor the share of bit-equal elements must reach min_equal.
    Returns Verdict(ok, worst ulp distance, bit-equal share, flat index of the first failing element or -1, number of failing elements, worst
    ulp distance over the elements whose intermediate is a normal number -- where the band admits nothing the ulp limit would not)."""
    got = to64(got16)
    gb = got16.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.int64) & 0xffff
    model = np.broadcast_to(np.asarray(model64, np.float64), got.shape)
    inter = np.broadcast_to(np.asarray(inter64, np.float64), got.shape)
    mult = np.broadcast_to(np.asarray(mult64, np.float64), got.shape)
    gn, mn = np.isnan(got), np.isnan(model)
    d = np.abs(_ordered(gb) - _ordered(bits16(model, dtype)))
    d = np.where(gn | mn, 0, d)
    with np.errstate(all="ignore"):
        band = ulp16(inter, dtype) * np.abs(mult) + ulp16(model, dtype)
        in_band = np.abs(got - model) <= band                              # (False wherever a NaN or inf - inf is involved)
    good = np.where(gn | mn, gn & mn, (d <= max_ulp) | in_band)
    equal = np.where(gn | mn, gn & mn, d == 0)
    share = float(equal.mean()) if equal.size else 1.0
    bad = np.flatnonzero(~good.ravel())
    worst = int(d.max()) if d.size else 0
    normal = np.abs(inter) >= np.ldexp(1.0, _FORMAT[dtype][1])
    worst_normal = int(d[normal].max()) if normal.any() else 0
    return Verdict(bool(bad.size == 0 and share >= min_equal), worst, share, int(bad[0]) if bad.size else -1, int(bad.size), worst_normal)


# ------------------------------------------------------------------------------------------------------------------------ shared inputs
NORM_EPS = (1e-6, 1e-5, 1e-2)          # 1e-2 makes eps visible in every row class
NORM_TENANTS = 3
NAN_ROW, INF_ROW, ZERO_ROW = "f", "g", "d"
# bd_srv_rmsnorm's block-per-row kernel (fewer than 64 rows; 256 threads x 8 elements per pass): one thread; 33 threads; exactly one pass; thread 0
# alone in a second pass; four passes; a fifth pass.  3 tenants x 7 rows.
NORM_BLOCK_H, NORM_BLOCK_ROWS = (8, 264, 2048, 2056, 8192, 8200), 21
# its wave-per-row kernel (from 64 rows on, H = 2048 NCH): all four NCH instantiations.  3 tenants x 22 rows: at the 64-row switch, not a multiple
# of the 4 rows of a block (idle waves in the last one), and a block straddles two tenants.
NORM_WAVE_H, NORM_WAVE_ROWS = (2048, 4096, 6144, 8192), 66


def norm_row_classes(dtype):
    """the cycle of row classes: the NaN row (f) and the inf row (g) sit BETWEEN ordinary rows"""
    return ["a", "f", "b", "g", "c", "d"] + (["e"] if dtype == torch.float16 else [])


def norm_inputs(dtype, H, rows, seed=0):
    """(x [rows, H], w [3, H], classes [rows]) as CPU tensors of `dtype`.  Row r is of class norm_row_classes(dtype)[r % len]:
    a  randn;   b  randn * 2^-10 (mean square ~1e-6: eps dominates);   c  randn * 1e3 (bf16) / 100 (fp16) with one element 60 x larger;
    d  all zero;   e  (fp16) every element an fp16 subnormal (see below for which);   f  randn with one NaN;   g  randn with one +inf.
    Weights: tenant 0  1 + 0.1 randn;  tenant 1  magnitudes spread over 0.02 .. 5, a third of them negative, one exact 0;  tenant 2  all 1."""
    g = torch.Generator().manual_seed(1000 * H + rows + (7 if dtype == torch.float16 else 0) + seed)
    cyc = norm_row_classes(dtype)
    classes = [cyc[r % len(cyc)] for r in range(rows)]
    x = torch.randn(rows, H, generator=g)
    for r, c in enumerate(classes):
        col = int(torch.randint(0, H, (1,), generator=g))
        if c == "b":
            x[r] *= 2.0 ** -10
        elif c == "c":
            x[r] *= 1e3 if dtype == torch.bfloat16 else 100.0
            x[r, col] = (60e3 if dtype == torch.bfloat16 else 6e3) * (1 if r % 2 else -1)
        elif c == "d":
            x[r] = 0
        elif c == "e":
            # k * 2^-24 with k < 205 (every low bit pattern) or k a multiple of 8 up to 1016.  NOT every k: at eps = 1e-2 these rows have
            # rs = 10 - 4e-8, which fp32 holds as 10.0 exactly, and 10 k * 2^-24 is an exact fp16 midpoint for a tenth of the other k (odd k
            # from 205, k = 2 mod 4 from 410, k = 4 mod 8 from 820): there the fp32 product is a tie and goes to even while the exact one
            # lies just below it -- a legitimate half-ulp of rs, not a rounding point, and enough to pull a tensor's bit-equal share to 0.985
            k = torch.where(torch.arange(H) % 2 == 0, torch.randint(1, 205, (H,), generator=g), 8 * torch.randint(26, 128, (H,), generator=g))
            sub = k.double() * 2.0 ** -24
            x[r] = (sub * torch.where(torch.rand(H, generator=g) < 0.5, -1.0, 1.0)).float()
        elif c == "f":
            x[r, col] = float("nan")
        elif c == "g":
            x[r, col] = float("inf")
    w = torch.ones(NORM_TENANTS, H)
    w[0] = 1 + 0.1 * torch.randn(H, generator=g)
    w[1] = torch.exp(torch.rand(H, generator=g) * (np.log(5.0) - np.log(0.02)) + np.log(0.02))
    w[1] *= torch.where(torch.rand(H, generator=g) < 1 / 3, -1.0, 1.0)
    w[1, int(torch.randint(0, H, (1,), generator=g))] = 0.0
    return x.to(dtype), w.to(dtype), classes


SWIGLU_U_ROWS = (1.0, -1.0, 0.5, 3.0, -7.25, 1.0 / 3.0, 100.0, 2.0 ** -10)


def swiglu_exhaustive_inputs(dtype):
    """(g [8, n], u [8, n]) CPU tensors: along every row EVERY finite pattern of `dtype` with |g| <= 80, both signs and +-0 (43 522 for fp16,
    34 114 for bf16), padded with zeros to a multiple of 8; u constant per row: SWIGLU_U_ROWS rounded to `dtype`."""
    top = int(bits16(np.array(80.0), dtype))
    pats = np.concatenate([np.arange(top + 1), np.arange(top + 1) | 0x8000])
    pats = np.concatenate([pats, np.zeros((-len(pats)) % 8, dtype=pats.dtype)])
    g = from_bits(pats, dtype)[None, :].expand(len(SWIGLU_U_ROWS), -1).contiguous()
    u = from_bits(bits16(np.array(SWIGLU_U_ROWS), dtype), dtype)[:, None].expand(-1, g.shape[1]).contiguous()
    return g, u


def add_norm_y32(resid, classes):
    """the fp32 partial sums bd_srv_add_rmsnorm adds to `resid`: randn * 0.7, scaled like the residual in the rows of class b"""
    g = torch.Generator().manual_seed(resid.shape[1] + 5)
    y32 = torch.randn(resid.shape, generator=g) * 0.7
    for r, c in enumerate(classes):
        if c == "b":
            y32[r] *= 2.0 ** -10
    return y32


ROTATION_PAIRS = ((10, 3), (107, 100), (255, 248))          # (m, n) with one difference; 255 is the last row of a 256-row table


def rotation_spread(rotated, pairs, dtype):
    """rotated [L, 128]: ONE vector rotated to every position (float64 values of `dtype`).  q(m) . k(n) must depend on m - n only, whatever the
    table convention: returns (largest - smallest dot product over `pairs`, tolerance) with the tolerance the sum, over the vectors involved, of
    every element's half ulp times its partner's magnitude -- what the final rounding of each output alone may move the dot products by."""
    rotated = np.asarray(rotated, np.float64)
    dots, tol = [], 0.0
    for m, n in pairs:
        q, k = rotated[m], rotated[n]
        dots.append(float((q * k).sum()))
        tol += float((0.5 * ulp16(q, dtype) * np.abs(k)).sum() + (0.5 * ulp16(k, dtype) * np.abs(q)).sum())
    return max(dots) - min(dots), tol
