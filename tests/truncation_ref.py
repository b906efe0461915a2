"""The truncation definition of include/bitdelta_hip.h (bd_srv_truncate_rows) restated in numpy fp64, and the rule by which the GPU tests accept
a kernel's row.  It uses no kernel under test and no torch op on values.  A logits row is given as its 16-bit patterns (uint16) plus the dtype
name ("float16" / "bfloat16"), as in sampling_ref.py, so that this file sees exactly what the kernel reads; the temperature and the four
parameters are taken as the float32 values the kernel reads.

Tolerances (check_row).  E = 1e-4 on masses (kept_set's eps in sampling_ref.py) and delta = 1e-4 * max(1, max_F |x_i|) on x and on keys.
delta is derived, not measured: x = (l - m) / tau is formed in fp32 from two exact 16-bit values (two roundings: 1.2e-7 |x|); the kernel's masses
are 2^-40 fixed-point words with a relative error of a few 1e-6 (sample_mass' comment in csrc/bd_serving.h), their sums are integer sums, and
ln Z, mu and theta are formed from the integers in fp64, so the error of mu and of ln Z is bounded by a few 1e-6 * max |x| and that of a key
|x - mu| by the same plus one fp32 rounding.  delta leaves more than 10x over that."""
import math

import numpy as np

from sampling_ref import is_special, values

E = 1e-4
NEUTRAL = (0.0, 1.0, 0.0, 0.0)
NINF = {"float16": 0xFC00, "bfloat16": 0xFF80}


def f32(v):
    return float(np.float32(v))


def is_neutral(params):
    mp, ty, ep, et = (f32(v) for v in params)
    return not (mp > 0.0 or 0.0 < ty < 1.0 or ep > 0.0 or et > 0.0)


def is_copied(l, tau, params):
    """the rows the launch copies bit for bit: nothing asked, a greedy temperature, or a special row"""
    tau = f32(tau)
    return is_neutral(params) or not (0.0 < tau < math.inf) or is_special(l)


def statistics(l, tau):
    """fin, x, p, Z, mu, H of a row that is not special: x and p are -inf / 0 outside the finite elements"""
    tau = f32(tau)
    fin = np.isfinite(l)
    m = l[fin].max()
    x = np.where(fin, (np.where(fin, l, m) - m) / tau, -np.inf)
    w = np.where(fin, np.exp(x), 0.0)
    Z = math.fsum(w[fin])
    p = w / Z
    mu = math.fsum((p * np.where(fin, x, 0.0))[fin])
    return dict(fin=fin, x=x, p=p, Z=Z, mu=mu, H=math.log(Z) - mu)


def theta_of(st, params):
    """the three threshold filters as one bound on x (clamped to <= 0); -inf when none is set"""
    mp, _, ep, et = (f32(v) for v in params)
    th = -math.inf
    if mp > 0.0:
        th = max(th, math.log(mp))
    if ep > 0.0:
        th = max(th, math.log(ep) + math.log(st["Z"]))
    if et > 0.0:
        th = max(th, math.log(min(et, math.sqrt(et) * math.exp(-st["H"]))) + math.log(st["Z"]))
    return min(th, 0.0)


def mass_below(key, p, fin, c):
    """the mass of the finite elements whose key is strictly below c"""
    return math.fsum(p[fin & (key < c)])


def typical_mask(st, typical_p):
    """element i passes when the mass of the elements with a strictly smaller key |x_i - mu| is below typical_p; ties are all kept"""
    fin, p = st["fin"], st["p"]
    key = np.where(fin, np.abs(np.where(fin, st["x"], 0.0) - st["mu"]), np.inf)
    idx = np.nonzero(fin)[0]
    order = idx[np.argsort(key[idx], kind="stable")]                    # ascending keys
    ks = key[order]
    cum = np.concatenate([[0.0], np.cumsum(p[order])])                  # cum[j]: the mass of the first j
    below = cum[np.searchsorted(ks, ks, side="left")]                   # ... of the strictly smaller keys: equal keys share their first place
    mask = np.zeros_like(fin)
    mask[order[below < typical_p]] = True
    return mask, key


def reference(bits, dtype, tau, params):
    """The definition on one row.  Returns a dict: copied (the row is passed through), and otherwise mask (bool [V]: the kept elements, all of
    them finite), thr / typ (the two filters' own sets; typ is None when typical_p is off), fallback (typical_p was ignored: its set did not
    meet the thresholds' set), st (statistics), key, theta, delta."""
    l = values(bits, dtype)
    if is_copied(l, tau, params):
        return dict(copied=True)
    st = statistics(l, tau)
    fin, x = st["fin"], st["x"]
    theta = theta_of(st, params)
    thr = fin & (x >= theta)
    ty = f32(params[1])
    typ, key, fallback = None, None, False
    mask = thr
    if 0.0 < ty < 1.0:
        typ, key = typical_mask(st, ty)
        both = thr & typ
        fallback = not both.any()
        mask = thr if fallback else both
    delta = 1e-4 * max(1.0, float(np.abs(x[fin]).max()))
    return dict(copied=False, mask=mask, thr=thr, typ=typ, fallback=fallback, st=st, key=key, theta=theta, delta=delta)


def kept_ids(bits, dtype, tau, params):
    """the kept set as a sorted list of indices (every finite element for a copied row)"""
    r = reference(bits, dtype, tau, params)
    if r["copied"]:
        return np.nonzero(np.isfinite(values(bits, dtype)))[0].tolist()
    return np.nonzero(r["mask"])[0].tolist()


def is_informative(bits, dtype, tau, params):
    """the reference keeps more than one and fewer than all finite elements: a case on such a row tests something"""
    r = reference(bits, dtype, tau, params)
    return (not r["copied"]) and 1 < int(r["mask"].sum()) < int(r["st"]["fin"].sum())


def _thresholds_ok(r, K):
    """K is an accepted thresholds set: everything at or above theta + delta kept, everything below theta - delta dropped, the maximum kept"""
    fin, x, th, d = r["st"]["fin"], r["st"]["x"], r["theta"], r["delta"]
    must, may = fin & (x >= th + d), fin & (x >= th - d)
    return bool((K[must]).all() and not (K & ~may).any() and K[fin & (x == 0.0)].all())


def _mass_before(r, i, shift):
    """the mass of the finite elements other than i and its equals (the same value: the same key in any arithmetic) whose key lies below
    key_i + shift"""
    fin, p, key, x = r["st"]["fin"], r["st"]["p"], r["key"], r["st"]["x"]
    return math.fsum(p[fin & (key < key[i] + shift) & (x != x[i])])


def _typical_ok(r, K, scope, ty):
    """K = (an accepted typical set) restricted to `scope` (the elements the thresholds surely keep; all finite ones when no threshold is set):
    with d_K the largest key in K and D the smallest key of scope outside K, D > d_K - delta, the mass of the keys below d_K - delta is below
    typical_p + E and the mass of the keys below D + delta is at least typical_p - E (masses over the whole row).  The last mass leaves out the
    dropped element itself and its equals: they are never among the strictly more typical ones, whatever the arithmetic -- without that the
    condition would accept any set that drops one element too many."""
    fin, p, key, d = r["st"]["fin"], r["st"]["p"], r["key"], r["delta"]
    if not K.any():
        return False
    d_K = float(key[K].max())
    out = np.nonzero(scope & ~K)[0]
    if len(out) == 0:
        return mass_below(key, p, fin, d_K - d) < ty + E
    i = int(out[np.argmin(key[out])])
    if not key[i] > d_K - d:
        return False
    return mass_below(key, p, fin, d_K - d) < ty + E and _mass_before(r, i, d) >= ty - E


def check_row(bits, dtype, tau, params, out_bits, r=None):
    """Judge the kernel's output row (r: reference() of the same arguments, when the caller has it already).  Raises AssertionError with the reason when it is not accepted; returns True when the row is EXACTLY the
    reference's, False when it is accepted inside the tolerances.  Always exact: a kept element keeps its 16 bits, a dropped one is the dtype's
    -inf, -inf stays -inf, a copied row is bit-identical."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    out_bits = np.ascontiguousarray(out_bits, dtype=np.uint16)
    assert bits.shape == out_bits.shape
    r = reference(bits, dtype, tau, params) if r is None else r
    if r["copied"]:
        assert np.array_equal(bits, out_bits), "a copied row changed"
        return True
    ninf = NINF[dtype]
    same, dropped = out_bits == bits, out_bits == ninf
    assert bool((same | dropped).all()), "an element is neither its own bits nor -inf"
    fin = r["st"]["fin"]
    assert bool(dropped[~fin].all()), "-inf did not stay -inf"          # (not special: everything outside fin is -inf)
    K = fin & same
    if np.array_equal(K, r["mask"]):
        return True
    x, th, d = r["st"]["x"], r["theta"], r["delta"]
    if r["typ"] is None:
        assert _thresholds_ok(r, K), "thresholds: outside the tolerance (theta %.6g, delta %.3g)" % (th, d)
        return False
    ty = f32(params[1])
    must, may = fin & (x >= th + d), fin & (x >= th - d)
    # does typical_p surely keep / may it keep an element of the thresholds' set, with every key moved by delta and every mass by E?  The most
    # typical element of the set decides both (for `maybe` exactly: the mass in front of a key grows with the key; for `sure` it can only say
    # no too often, which lets both rules apply)
    i_must = int(np.nonzero(must)[0][np.argmin(r["key"][must])])        # (must holds the maximum: never empty)
    i_may = int(np.nonzero(may)[0][np.argmin(r["key"][may])])
    sure = _mass_before(r, i_must, d) < ty - E
    maybe = _mass_before(r, i_may, -d) < ty + E
    ok = False
    if maybe:                                                           # the intersection may be non-empty
        ok = bool(not (K & ~may).any()) and _typical_ok(r, K, must, ty)
    if not ok and not sure:                                             # the intersection may be empty: the thresholds' set stands
        ok = _thresholds_ok(r, K)
    assert ok, "typical_p %.6g with theta %.6g: outside the tolerance (delta %.3g)" % (ty, th, d)
    return False
