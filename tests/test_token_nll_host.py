"""CPU-only checks of the scoring path: the window rule of eval_ppl.ppl_windows against the reference loop's known answers, the new C-ABI
symbol in the header, the built library, the ctypes table and INTEGRATION.md with every argument check it answers before any device call, and
the fp64 restatement of the definition (nll_ref) on rows small enough to decide by hand."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import nll_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bd_srv_token_nll"

WINDOWS = [
    ((10, 4, 2), [(0, 6, 2), (2, 8, 2), (4, 10, 2)]),
    ((11, 4, 2), [(0, 6, 2), (2, 8, 2), (4, 10, 2)]),
    ((5, 4, 2), [(0, 5, 2)]),
    ((4, 4, 2), [(0, 4, 2)]),
    ((2, 4, 2), [(0, 2, 1)]),
    ((4, 0, 2), [(0, 2, 1), (2, 4, 1)]),
    ((13, 4, 4), [(0, 8, 4), (4, 12, 4)]),
    ((300, 128, 64), [(0, 192, 64), (64, 256, 64)]),
]


@pytest.mark.parametrize("args,expected", WINDOWS)
def test_ppl_windows_table(args, expected):
    from bitdelta_amd.eval_ppl import ppl_windows
    assert ppl_windows(*args) == expected


def test_ppl_windows_refuses_a_text_without_a_window_and_has_the_reference_defaults():
    from bitdelta_amd.eval_ppl import ppl_windows
    with pytest.raises(ValueError):
        ppl_windows(1, 4, 2)
    with pytest.raises(ValueError):
        ppl_windows(511)
    assert ppl_windows(2048) == [(0, 1536, 512), (512, 2048, 512)]


def test_symbol_in_header_library_ctypes_table_and_integration_notes():
    from bitdelta_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bitdelta_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, txt)
    assert decl, NAME + " is not declared in include/bitdelta_hip.h"
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == len(decl.group(1).split(",")) == 9
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(_lib.lib(), NAME)
    from bitdelta_amd import eval_ppl, serving_loop, serving_ops
    assert callable(serving_ops.token_nll) and callable(serving_loop.TenantDecoder.score)
    assert callable(eval_ppl.ppl_windows) and callable(eval_ppl.perplexity)


def test_entry_point_validates_before_any_device_call():
    from bitdelta_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255            # an aligned, non-null host address: never dereferenced by the checks
    BAD_SHAPE, BAD_DTYPE, NULL = (L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None),
                                  L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 7, None), L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 0, None))
    assert len({BAD_SHAPE, BAD_DTYPE, NULL, 0}) == 4
    good = dict(logits=base, sl=64, V=61, labels=base, nll=base, lse=base, R=2, dtype=0)

    def call(**kw):
        a = dict(good, **kw)
        return L.bd_srv_token_nll(a["logits"], a["sl"], a["V"], a["labels"], a["nll"], a["lse"], a["R"], a["dtype"], None)
    assert call(R=0) == 0 and call(R=0, logits=None, labels=None, nll=None) == 0      # an empty call: the one geometry that launches nothing
    assert call(R=-1) == BAD_SHAPE
    assert call(V=0) == BAD_SHAPE and call(V=-3) == BAD_SHAPE
    assert call(sl=56) == BAD_SHAPE and call(V=64, sl=60) == BAD_SHAPE                 # sl < V
    assert call(sl=68) == BAD_SHAPE and call(sl=61) == BAD_SHAPE                       # sl % 8
    assert call(logits=base + 8) == BAD_SHAPE and call(logits=base + 2) == BAD_SHAPE   # not 16-byte aligned
    assert call(nll=base + 2) == BAD_SHAPE and call(lse=base + 2) == BAD_SHAPE and call(labels=base + 4) == BAD_SHAPE
    for q in ("logits", "labels", "nll"):
        assert call(**{q: None}) == NULL, q
    assert call(dtype=2) == BAD_DTYPE and call(dtype=7) == BAD_DTYPE and call(dtype=-1) == BAD_DTYPE
    assert call(R=0, dtype=7) == BAD_DTYPE and call(R=0, V=0) == BAD_SHAPE             # a bad geometry is refused even when nothing would launch


def test_restatement_on_hand_made_rows():
    f16 = lambda xs: np.array(xs, dtype=np.float16).view(np.uint16)
    inf, nan = np.inf, np.nan
    for V in (1, 7, 512):                                                              # a uniform row: ln V, whatever the label
        nll, lse = ref.row_nll(ref.values(f16([2.5] * V), "float16"), V - 1)
        assert math.isclose(nll, math.log(V), rel_tol=1e-15, abs_tol=1e-15) and math.isclose(lse, 2.5 + math.log(V), rel_tol=1e-15)
    l = ref.values(f16([0.0, 30.0, 0.0, 0.0]), "float16")                              # one-hot-dominant: ln(1 + 3 e^-30), and 30 more off the peak
    tail = math.log1p(3.0 * math.exp(-30.0))
    assert math.isclose(ref.row_nll(l, 1)[0], tail, rel_tol=1e-12) and math.isclose(ref.row_nll(l, 0)[0], 30.0 + tail, rel_tol=1e-15)
    assert math.isclose(ref.row_nll(l, 1)[1], 30.0 + tail, rel_tol=1e-15)
    l = ref.values(f16([1.0, -inf, 1.0, -inf]), "float16")                             # -inf entries: weight 0; a label on one: +inf
    assert math.isclose(ref.row_nll(l, 0)[0], math.log(2.0), rel_tol=1e-15) and ref.row_nll(l, 1) == (inf, 1.0 + math.log(2.0))
    for row in ([1.0, inf, 0.0], [1.0, nan, 0.0], [-inf, -inf, -inf], [-inf, nan, -inf]):   # +inf, NaN, nothing finite: NaN
        l = ref.values(f16(row), "float16")
        for y in (0, 1, 2):
            nll, lse = ref.row_nll(l, y)
            assert math.isnan(nll) and math.isnan(lse), (row, y)
        for y in (ref.IGNORE, 3, -1):                                                  # ... unless the label is ignored
            nll, lse = ref.row_nll(l, y)
            assert nll == 0.0 and math.isnan(lse), (row, y)
    l = ref.values(f16([0.5, -1.0, 2.0]), "float16")                                   # an ignored label: exactly 0, the lse still there
    for y in (ref.IGNORE, 3, -1, 2 ** 40):
        nll, lse = ref.row_nll(l, y)
        assert nll == 0.0 and math.copysign(1.0, nll) == 1.0 and math.isclose(lse, math.log(math.exp(0.5) + math.exp(-1.0) + math.exp(2.0)), rel_tol=1e-15)
    bf = (np.array([1.0, -2.0], dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)            # the bf16 reading of the patterns
    assert ref.values(bf, "bfloat16").tolist() == [1.0, -2.0]
    nll, lse = ref.rows_nll(np.stack([f16([0.0, 0.0]), f16([0.0, nan])]), "float16", [1, ref.IGNORE])
    assert math.isclose(nll[0], math.log(2.0)) and nll[1] == 0.0 and math.isnan(lse[1])
    assert ref.within([1.0, nan, inf, 0.0], [1.0 + 1e-6, nan, inf, 0.0]).all()
    assert not ref.within([1.0, nan, inf, 1.0, -inf], [1.0 + 1e-5, 0.0, nan, nan, inf]).any()
