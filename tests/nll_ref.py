"""The token-NLL definition of include/bitdelta_hip.h (bd_srv_token_nll) restated in fp64 with numpy.  It uses no kernel under test and no
torch op on values; the GPU tests hold the kernel to it.

A logits row is given as its 16-bit patterns (uint16) plus the dtype name ("float16" / "bfloat16"), so that this file sees exactly what the
kernel reads."""
import math

import numpy as np

IGNORE = -100          # the reference's ignore label (HF CrossEntropyLoss); ANY label outside [0, V) is ignored
BOUND = 2.0 ** -19     # |got - ref| <= BOUND * (1 + |ref|): the header's accuracy clause


def values(bits, dtype):
    """the fp64 values of a row of 16-bit patterns"""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if dtype == "float16":
        return bits.view(np.float16).astype(np.float64)
    assert dtype == "bfloat16"
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def row_nll(l, label):
    """(nll, lse) of one row of fp64 values l and an integer label, by the definition:
    m = max l, S = sum exp(l - m); lse = m + ln S; nll = ln S - (l[label] - m).  A row with a NaN, a +inf or nothing finite: (NaN, NaN).
    -inf entries have weight 0; a label on one gives +inf.  A label outside [0, V): nll = 0.0 exactly, lse as above."""
    l = np.asarray(l, dtype=np.float64)
    V = l.shape[0]
    scored = 0 <= int(label) < V
    if np.isnan(l).any() or np.isposinf(l).any() or not np.isfinite(l).any():
        return (math.nan if scored else 0.0), math.nan
    m = float(l.max())
    with np.errstate(under="ignore"):
        terms = np.exp(l[np.isfinite(l)] - m).tolist()
    ln_s = math.log1p(math.fsum(terms + [-1.0]))           # the maximum's own term is exactly 1: ln S keeps its RELATIVE accuracy near 0
    lse = m + ln_s
    if not scored:
        return 0.0, lse
    ly = float(l[int(label)])
    return (math.inf if ly == -math.inf else ln_s - (ly - m)), lse


def rows_nll(bits, dtype, labels):
    """row_nll over rows of 16-bit patterns [R, V] and labels [R]: (nll [R], lse [R]) as float64 arrays"""
    out = [row_nll(values(b, dtype), int(y)) for b, y in zip(bits, labels)]
    return np.array([o[0] for o in out], dtype=np.float64), np.array([o[1] for o in out], dtype=np.float64)


def within(got, ref, bound=BOUND):
    """elementwise: NaN-ness and infinities compared exactly, finite values within bound * (1 + |ref|)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    ok = np.where(fin, np.abs(got - np.where(fin, ref, 0.0)) <= bound * (1.0 + np.abs(np.where(fin, ref, 0.0))),
                  (np.isnan(ref) & np.isnan(got)) | (got == ref))
    return ok & (np.isfinite(got) == fin)
