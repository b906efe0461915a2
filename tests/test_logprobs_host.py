"""CPU-only checks of the log-probability path: the fp64 restatement (logprobs_ref) against torch.log_softmax + torch.topk on rows without ties
and on hand-built rows for the tie, -inf, +-0 and non-finite rules; the session's logprobs= argument check; the index rule that ties the step
launch's entries to result()'s n; and the two C-ABI symbols in the header, the library and the ctypes table with the argument checks they answer
before any device call."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import logprobs_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f16 = lambda xs: np.array(xs, dtype=np.float16).view(np.uint16)
inf, nan = math.inf, math.nan


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("V", [8, 512, 2056])
def test_restatement_is_log_softmax_and_topk_on_rows_without_ties(dtype, V):
    g = torch.Generator().manual_seed(V)
    # V distinct values: distinct bit patterns, both signs, magnitudes 2^-4 .. 8 (fp16) / 2^-8 .. 16 (bf16: fewer patterns per binade)
    lo, hi = (0x2C00, 0x4800) if dtype == torch.float16 else (0x3B80, 0x4180)
    mag = torch.arange(lo, hi, dtype=torch.int32)
    pats = torch.cat([mag, mag | 0x8000])
    pats = pats[torch.randperm(pats.numel(), generator=g)[:V]]
    x = (pats - (pats >= 0x8000).int() * 0x10000).to(torch.int16).view(dtype)
    assert x.unique().numel() == V and bool(torch.isfinite(x.float()).all())
    bits = x.view(torch.int16).numpy().view(np.uint16)
    want = torch.log_softmax(x.double(), dim=-1)
    for top_n in (0, 1, 5, min(20, V)):
        tok = int(torch.randint(0, V, (1,), generator=g))
        lp, ids, lps = ref.row_logprobs(ref.values(bits, {torch.float16: "float16", torch.bfloat16: "bfloat16"}[dtype]), tok, top_n)
        tv, ti = torch.topk(want, top_n)
        assert ids.tolist() == ti.tolist()
        assert np.allclose(lps, tv.numpy(), rtol=1e-12, atol=1e-12) and math.isclose(lp, float(want[tok]), rel_tol=1e-12, abs_tol=1e-12)


def test_restatement_on_hand_made_rows():
    rl = lambda row, y, k: ref.row_logprobs(ref.values(f16(row), "float16"), y, k)
    # ties: equal values in ascending index order, the plateau cut at top_n
    lp, ids, lps = rl([1.0, 3.0, 1.0, 3.0, 1.0, 0.0, 1.0, -2.0], 2, 5)
    assert ids.tolist() == [1, 3, 0, 2, 4] and lps[0] == lps[1] and lps[2] == lps[3] == lps[4] == lp
    assert rl([2.5] * 8, 7, 8)[1].tolist() == list(range(8))
    assert math.isclose(rl([2.5] * 8, 7, 0)[0], -math.log(8), rel_tol=1e-15) and rl([2.5] * 8, 7, 0)[1].shape == (0,)
    # -0 and +0 are one value: index order decides; a negative value sorts behind both
    assert rl([-0.0, 0.0, -1.0, 0.0, -0.0, -1.0, -3.0, -3.0], 0, 5)[1].tolist() == [0, 1, 3, 4, 2]
    # -inf: lp = -inf, in the list only when fewer than top_n values are finite, and then in index order
    lp, ids, lps = rl([-inf, 1.0, -inf, 0.0, -inf, -inf, -inf, -inf], 0, 4)
    assert lp == -inf and ids.tolist() == [1, 3, 0, 2] and lps[2] == lps[3] == -inf and math.isfinite(lps[1])
    assert math.isclose(lps[0], -math.log1p(math.exp(-1.0)), rel_tol=1e-15)
    assert rl([-inf, 1.0, -inf, 0.0, -inf, -inf, -inf, -inf], 1, 2)[1].tolist() == [1, 3]
    # a NaN, a +inf, nothing finite: NaN everywhere and ids -1, whatever the token
    for row in ([1.0, nan] + [0.0] * 6, [1.0, inf] + [0.0] * 6, [-inf] * 8, [-inf, nan] + [-inf] * 6):
        for y in (0, 1, -1, 8):
            lp, ids, lps = rl(row, y, 3)
            assert math.isnan(lp) and ids.tolist() == [-1] * 3 and np.isnan(lps).all(), (row, y)
    # the token out of range: NaN for it alone
    lp, ids, lps = rl([0.5, -1.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0], 8, 2)
    assert math.isnan(lp) and ids.tolist() == [2, 0] and np.isfinite(lps).all()
    assert math.isnan(rl([0.5] * 8, -1, 0)[0]) and math.isnan(rl([0.5] * 8, 2 ** 40, 0)[0])
    # lp is -nll of the scoring restatement
    import nll_ref
    row = ref.values(f16([0.5, -1.0, 2.0, 0.25, -inf, 7.0, 7.0, 1.0]), "float16")
    for y in range(8):
        assert ref.row_logprobs(row, y, 0)[0] == -nll_ref.row_nll(row, y)[0] or math.isclose(ref.row_logprobs(row, y, 0)[0], -nll_ref.row_nll(row, y)[0], rel_tol=1e-14)
    # the bf16 reading, and the batched form's shapes
    bf = (np.array([1.0, -2.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)
    lp, ids, lps = ref.rows_logprobs(np.stack([bf, bf]), "bfloat16", [2, 9], 2)
    assert lp.shape == (2,) and ids.shape == lps.shape == (2, 2) and ids[0].tolist() == [2, 0] and math.isnan(lp[1]) and lp[0] == lps[0, 0]
    assert ref.rows_logprobs(np.stack([bf]), "bfloat16", [0], 0)[1].shape == (1, 0)


def test_logprobs_argument_check():
    from bitdelta_amd.serving_loop import logprobs_count
    assert logprobs_count(None) is None and logprobs_count(0) == 0 and logprobs_count(20) == 20 and logprobs_count(np.int64(5)) == 5
    for bad in (-1, 21, True, False, 2.5, "3", [1]):
        with pytest.raises(ValueError):
            logprobs_count(bad)


def test_the_step_rule_writes_exactly_the_entries_result_reports():
    """logprobs_slot is step_logprobs' rule on host integers: over a tenant's life (admission writes entry 0 and sets both counters to 1; each step
    in which it is active moves n by one; steps in which it is not leave n alone) the entries written are 0 .. min(n, cap) - 1, entry j by the
    step that stored token j -- the slice result_logprobs takes"""
    from bitdelta_amd.serving_loop import logprobs_slot
    for cap in (1, 4, 9):
        n = lp_n = 1
        written = [0]
        for step, active in enumerate([1, 1, 0, 1, 0, 0, 1, 1, 1]):
            n += active                                     # the step-end launch: out[t, n] = token, n += 1 (only when active)
            j, lp_n = logprobs_slot(n, lp_n, cap)
            assert (j is not None) == (bool(active) and n - 1 < cap) and lp_n == n
            if j is not None:
                assert j == n - 1
                written.append(j)
        assert written == list(range(min(n, cap)))
    assert logprobs_slot(0, 0, 4) == (None, 0)              # never admitted, or cleared by load_tenant: not touched
    assert logprobs_slot(5, 5, 4) == (None, 5)


NAMES = {"bd_srv_token_logprobs": 11, "bd_srv_step_logprobs": 14}


def test_symbols_in_header_library_ctypes_table_and_integration_notes():
    from bitdelta_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bitdelta_hip.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    for name, nargs in NAMES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert decl, name + " is not declared in include/bitdelta_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == nargs
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
        assert hasattr(_lib.lib(), name)
    from bitdelta_amd import serving_loop, serving_ops
    assert callable(serving_ops.token_logprobs) and callable(serving_ops.step_logprobs)
    assert callable(serving_loop.TenantSession.result_logprobs)


def test_entry_points_validate_before_any_device_call():
    from bitdelta_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255            # an aligned, non-null host address: never dereferenced by the checks
    BAD_SHAPE, BAD_DTYPE, NULL = (L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None),
                                  L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 7, None), L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 0, None))
    assert len({BAD_SHAPE, BAD_DTYPE, NULL, 0}) == 4
    good = dict(logits=base, sl=72, V=64, tok=base, n=base, lp_n=base, lp=base, top_id=base, top_lp=base, cap=4, top_n=5, R=2, dtype=0)

    def rows(**kw):
        a = dict(good, **kw)
        return L.bd_srv_token_logprobs(a["logits"], a["sl"], a["V"], a["tok"], a["lp"], a["top_id"], a["top_lp"], a["top_n"], a["R"], a["dtype"], None)

    def step(**kw):
        a = dict(good, **kw)
        return L.bd_srv_step_logprobs(a["logits"], a["sl"], a["V"], a["tok"], a["n"], a["lp_n"], a["lp"], a["top_id"], a["top_lp"], a["cap"],
                                      a["top_n"], a["R"], a["dtype"], None)
    for call in (rows, step):
        assert call(R=0) == 0 and call(R=0, logits=None, tok=None, lp=None, top_id=None, top_lp=None, n=None, lp_n=None) == 0     # launches nothing
        assert call(R=-1) == BAD_SHAPE
        assert call(top_n=-1) == BAD_SHAPE and call(top_n=21) == BAD_SHAPE and call(V=8, sl=8, top_n=9) == BAD_SHAPE             # 0 .. 20, <= V
        assert call(V=60) == BAD_SHAPE and call(V=0) == BAD_SHAPE and call(V=(1 << 22) + 8, sl=(1 << 22) + 8) == BAD_SHAPE        # V % 8, V > 2^22
        assert call(sl=68) == BAD_SHAPE and call(sl=56) == BAD_SHAPE                                                               # sl % 8, sl < V
        assert call(logits=base + 8) == BAD_SHAPE and call(tok=base + 4) == BAD_SHAPE
        for q in ("lp", "top_id", "top_lp"):
            assert call(**{q: base + 2}) == BAD_SHAPE, q
        for q in ("logits", "tok", "lp", "top_id", "top_lp"):
            assert call(**{q: None}) == NULL, q
        assert call(dtype=2) == BAD_DTYPE and call(dtype=7) == BAD_DTYPE and call(dtype=-1) == BAD_DTYPE
    for q in ("n", "lp_n"):
        assert step(**{q: None}) == NULL and step(**{q: base + 4}) == BAD_SHAPE, q
    assert step(cap=-1) == BAD_SHAPE
