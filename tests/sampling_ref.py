"""The sampling definition of include/bitdelta_hip.h (bd_srv_sample_rows) restated in numpy: Philox4x32-10 in integers, everything else in fp64.
It uses no kernel under test and no torch op on values; the GPU tests hold the kernels to it, the host tests pin its generator to known answers.

A logits row is given as its 16-bit patterns (uint16) plus the dtype name ("float16" / "bfloat16"), so that this file sees exactly what the
kernel reads."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

# counter || key -> output (the issue's known answers; the first two are Random123's published vectors)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK, MASK, MASK, MASK), (MASK, MASK), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 ints -> 4 uint64 arrays holding 32-bit words"""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in counter]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]             # 32 x 32 -> 64 bits: no overflow in uint64
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & np.uint64(MASK), p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [h1 ^ c[1] ^ np.uint64(k0), l1, h0 ^ c[3] ^ np.uint64(k1), l0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def words(V, seed, d):
    """r_i for tokens 0 .. V-1: key = (seed & 0xffffffff, seed >> 32), counter = (i >> 2, 0, d & 0xffffffff, d >> 32), word i & 3"""
    seed, d = int(seed) & (2 ** 64 - 1), int(d) & (2 ** 64 - 1)
    nb = (V + 3) // 4
    out = philox4x32_10((np.arange(nb), np.zeros(nb), np.full(nb, d & MASK), np.full(nb, d >> 32)), (seed & MASK, seed >> 32))
    return np.stack(out, axis=1).reshape(-1)[:V]


def words_rows(V, seed, ds):
    """words(V, seed, d) for every d of ds at once: [len(ds), V]"""
    seed = int(seed) & (2 ** 64 - 1)
    ds = np.array([int(d) & (2 ** 64 - 1) for d in ds], dtype=np.uint64)
    nb = (V + 3) // 4
    blk = np.broadcast_to(np.arange(nb, dtype=np.uint64), (len(ds), nb))
    lo, hi = np.broadcast_to((ds & np.uint64(MASK))[:, None], blk.shape), np.broadcast_to((ds >> np.uint64(32))[:, None], blk.shape)
    out = philox4x32_10((blk, np.zeros_like(blk), lo, hi), (seed & MASK, seed >> 32))
    return np.stack(out, axis=2).reshape(len(ds), -1)[:, :V]


def values(bits, dtype):
    """the fp64 values of a row of 16-bit patterns"""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if dtype == "float16":
        return bits.view(np.float16).astype(np.float64)
    assert dtype == "bfloat16"
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def pattern(value, dtype):
    """the 16-bit pattern of a value that IS a 16-bit float (+0 for a zero)"""
    if value == 0:
        return 0
    if dtype == "float16":
        return int(np.array([value], dtype=np.float16).view(np.uint16)[0])
    return int(np.array([value], dtype=np.float32).view(np.uint32)[0] >> 16)


def greedy(l):
    """torch.argmax's order: a NaN is the maximum, ties go to the lower index"""
    nan = np.isnan(l)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(l))


def is_special(l):
    """a NaN or +inf in the row, or nothing finite: the greedy rule decides whatever the temperature is"""
    return bool(np.isnan(l).any() or np.isposinf(l).any() or not np.isfinite(l).any())


def kept_set(l, tau, top_k, top_p, eps=1e-4):
    """The filters on a row without NaN / +inf and with something finite.  Returns a dict:
    mask (bool [V]: the kept tokens; -inf is never kept), thr (the smallest kept value), count, decisive (no value's cumulative ratio lies within
    eps of top_p; the row's maximum, whose ratio is 0 and which is kept whatever top_p is, is not a boundary and does not count), near (the kept
    sets an indecisive row may also report: one boundary value more or less, as (thr, count) pairs)."""
    V = l.shape[0]
    top_p = float(np.float32(top_p))                                   # the kernel reads a float32
    fin = np.isfinite(l)
    mask = fin.copy()
    if 1 <= top_k < V:
        kth = np.sort(l)[::-1][top_k - 1]                             # ties at the threshold are all kept
        mask &= l >= kth
    decisive, near = True, []
    if 0.0 < top_p < 1.0:
        m = l[mask].max()
        vals, counts = np.unique(l[mask], return_counts=True)
        vals, counts = vals[::-1], counts[::-1]                        # descending values
        w = counts * np.exp((vals - m) / tau)
        Z = math.fsum(w)
        above = np.concatenate([[0.0], np.cumsum(w)[:-1]]) / Z         # mass of the strictly larger values
        keep = above < top_p
        keep[0] = True
        decisive = not bool((np.abs(above[1:] - top_p) <= eps).any())
        j = int(np.nonzero(keep)[0].max())
        for jj in (j - 1, j + 1):
            if 0 <= jj < len(vals):
                near.append((float(vals[jj]), int(counts[:jj + 1].sum())))
        mask &= l >= vals[j]
    return dict(mask=mask, thr=float(l[mask].min()), count=int(mask.sum()), decisive=decisive, near=near)


def sample(bits, dtype, tau, top_k, top_p, seed, d):
    """The token of one row and what decides it.  Returns a dict: token, greedy (the greedy rule decided), and otherwise count / thr / near /
    filters_decisive (kept_set), r (the token's Philox word), gap (the fp64 distance of the two best scores; inf when one token is kept), second
    (the runner-up or None), delta (the issue's bound 1e-3 * max(1, max|l| / tau)): a draw is decisive when gap > delta."""
    l = values(bits, dtype)
    V = l.shape[0]
    tau = float(np.float32(tau))
    if not (0.0 < tau < math.inf) or is_special(l):
        return dict(token=greedy(l), greedy=True)
    ks = kept_set(l, tau, int(top_k), top_p)
    r = words(V, seed, d)
    u = ((r >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    with np.errstate(divide="ignore"):
        score = np.where(ks["mask"], l / tau - np.log(-np.log(u)), -np.inf)
    order = np.argsort(-score, kind="stable")                          # stable: ties to the lower index
    tok = int(order[0])
    second = int(order[1]) if ks["count"] > 1 else None
    gap = float(score[tok] - score[second]) if second is not None else math.inf
    delta = 1e-3 * max(1.0, float(np.abs(l[np.isfinite(l)]).max()) / tau)
    return dict(token=tok, greedy=False, count=ks["count"], thr=ks["thr"], near=ks["near"], filters_decisive=ks["decisive"], r=int(r[tok]),
                second=second, r_second=int(r[second]) if second is not None else None, gap=gap, delta=delta, mask=ks["mask"])


def chi2_sf(x, k):
    """P(chi-square with k degrees of freedom > x): the regularised upper incomplete gamma function Q(k / 2, x / 2), by its series below
    a + 1 and its continued fraction above (Numerical Recipes, gammp / gammq)."""
    a, x = k / 2.0, x / 2.0
    if x <= 0:
        return 1.0
    lg = math.lgamma(a)
    if x < a + 1:
        term = total = 1.0 / a
        n = a
        for _ in range(10000):
            n += 1
            term *= x / n
            total += term
            if abs(term) < abs(total) * 1e-16:
                break
        return 1.0 - total * math.exp(-x + a * math.log(x) - lg)
    tiny = 1e-300
    b = x + 1 - a
    c, dd = 1 / tiny, 1 / b
    h = dd
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2
        dd = an * dd + b
        dd = tiny if abs(dd) < tiny else dd
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        dd = 1 / dd
        de = dd * c
        h *= de
        if abs(de - 1) < 1e-16:
            break
    return math.exp(-x + a * math.log(x) - lg) * h
