"""The log-probability definition of include/bitdelta_hip.h (bd_srv_token_logprobs) restated in fp64 with numpy.  It uses no kernel under test and
no torch op on values; the GPU tests hold the kernel to it.

A logits row is given as its 16-bit patterns (uint16) plus the dtype name ("float16" / "bfloat16"), as in nll_ref, whose log-sum-exp this file
reuses: lp(i) = (l_i - m) - ln S."""
import math

import numpy as np

import nll_ref

BOUND = nll_ref.BOUND      # |got - ref| <= BOUND * (1 + |ref|): the header's accuracy clause, bd_srv_token_nll's
TOP_MAX = 20
values, within = nll_ref.values, nll_ref.within


def row_logprobs(l, token, top_n):
    """(lp, top_id [top_n], top_lp [top_n]) of one row of fp64 values l, by the definition.  The list is a STABLE sort by (-value, index); -0 and
    +0 are one value in fp64 already.  A row with a NaN, a +inf or nothing finite: (NaN, all -1, all NaN).  A token outside [0, V): lp = NaN.
    -inf has lp = -inf and sorts behind every finite value, in index order."""
    l = np.asarray(l, dtype=np.float64)
    V = l.shape[0]
    assert 0 <= top_n <= min(TOP_MAX, V)
    if np.isnan(l).any() or np.isposinf(l).any() or not np.isfinite(l).any():
        return math.nan, np.full(top_n, -1, dtype=np.int64), np.full(top_n, math.nan)
    _, lse = nll_ref.row_nll(l, -1)                        # m + ln S; an ignored label: only the log-sum-exp is taken
    m = float(l.max())
    ln_s = lse - m                                          # exact enough: |m| <= 65504 and ln S <= ln V, and the bound is relative to 1 + |lp|
    lp_of = lambda i: -math.inf if l[i] == -math.inf else (float(l[i]) - m) - ln_s
    order = np.argsort(-l, kind="stable")[:top_n]           # -(-inf) = +inf sorts last; ties keep ascending index
    lp = lp_of(int(token)) if 0 <= int(token) < V else math.nan
    return lp, order.astype(np.int64), np.array([lp_of(int(i)) for i in order], dtype=np.float64)


def rows_logprobs(bits, dtype, tokens, top_n):
    """row_logprobs over rows of 16-bit patterns [R, V] and tokens [R]: (lp [R], top_id [R, top_n], top_lp [R, top_n])"""
    out = [row_logprobs(values(b, dtype), int(y), top_n) for b, y in zip(bits, tokens)]
    return (np.array([o[0] for o in out], dtype=np.float64), np.stack([o[1] for o in out]).reshape(len(out), top_n),
            np.stack([o[2] for o in out]).reshape(len(out), top_n))
