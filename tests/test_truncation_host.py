"""CPU-only checks of the tail truncation (min_p / typical_p / epsilon_cutoff / eta_cutoff): the restatement (truncation_ref) answers the known
cases of the definition and its acceptance rule accepts the definition's own set and refuses a wrong one; truncation_params returns a canonical
form and refuses what it documents; a session made without truncation=True refuses the arguments, and truncation=True needs sampling=True; both
C-ABI symbols are in the header, the library, the ctypes table and INTEGRATION.md and answer their argument checks, in the documented order,
before any device call."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import truncation_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _known_row():
    """ln [0.5, 0.25, 0.125, 0.125] rounded to fp16, padded with -inf to V = 8"""
    l = np.log(np.array([0.5, 0.25, 0.125, 0.125])).astype(np.float16)
    return np.concatenate([l.view(np.uint16), np.full(4, 0xFC00, dtype=np.uint16)])


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("params, want", [
    (dict(min_p=0.3), [0, 1]),
    (dict(epsilon_cutoff=0.2), [0, 1]),
    (dict(eta_cutoff=0.1), [0, 1, 2, 3]),                                # the bound is 0.094
    (dict(eta_cutoff=0.2), [0, 1]),                                      # the bound is 0.133
    (dict(typical_p=0.2), [1]),                                          # the maximum is dropped
    (dict(typical_p=0.5), [0, 1]),
    (dict(min_p=0.3, typical_p=0.2), [1]),
    (dict(min_p=0.6, typical_p=0.2), [0]),                               # the empty-intersection rule
])
def test_known_answers(params, want):
    p = dict(dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0), **params)
    prm = (p["min_p"], p["typical_p"], p["epsilon_cutoff"], p["eta_cutoff"])
    bits = _known_row()
    assert ref.kept_ids(bits, "float16", 1.0, prm) == want
    r = ref.reference(bits, "float16", 1.0, prm)
    assert r["fallback"] == (params == dict(min_p=0.6, typical_p=0.2))
    out = np.where(r["mask"], bits, 0xFC00).astype(np.uint16)
    assert ref.check_row(bits, "float16", 1.0, prm, out) is True


def test_the_statistics_and_the_eta_bound_of_the_known_row():
    st = ref.statistics(ref.values(_known_row(), "float16"), 1.0)
    assert abs(st["H"] - 1.75 * math.log(2)) < 2e-3 and abs(st["Z"] - 2.0) < 2e-3 and abs(st["mu"] + 0.75 * math.log(2)) < 2e-3
    for eta, bound in ((0.1, 0.094), (0.2, 0.133)):
        assert abs(min(eta, math.sqrt(eta) * math.exp(-st["H"])) - bound) < 1e-3


def test_copied_rows_and_the_acceptance_rule():
    bits = _known_row()
    for tau, prm in ((1.0, ref.NEUTRAL), (0.0, (0.3, 1.0, 0.0, 0.0)), (math.inf, (0.3, 1.0, 0.0, 0.0)), (-1.0, (0.3, 1.0, 0.0, 0.0))):
        assert ref.reference(bits, "float16", tau, prm)["copied"]
        assert ref.check_row(bits, "float16", tau, prm, bits) is True
    for special in (0x7E00, 0x7C00):                                     # a NaN, a +inf
        b = bits.copy()
        b[2] = special
        assert ref.reference(b, "float16", 1.0, (0.3, 1.0, 0.0, 0.0))["copied"]
    assert ref.reference(np.full(8, 0xFC00, dtype=np.uint16), "float16", 1.0, (0.3, 1.0, 0.0, 0.0))["copied"]
    with pytest.raises(AssertionError):
        ref.check_row(bits, "float16", 0.0, (0.3, 1.0, 0.0, 0.0), np.where(np.arange(8) < 2, bits, 0xFC00).astype(np.uint16))
    # a wrong set is refused, whichever filter is set; a changed kept element and a dropped element that is no -inf are refused too
    for prm in ((0.3, 1.0, 0.0, 0.0), (0.0, 0.5, 0.0, 0.0), (0.3, 0.2, 0.0, 0.0), (0.6, 0.2, 0.0, 0.0)):
        good = ref.reference(bits, "float16", 1.0, prm)["mask"]
        for flip in range(4):
            bad = good.copy()
            bad[flip] = not bad[flip]
            with pytest.raises(AssertionError):
                ref.check_row(bits, "float16", 1.0, prm, np.where(bad, bits, 0xFC00).astype(np.uint16))
    out = np.where(np.arange(8) < 2, bits, 0xFC00).astype(np.uint16)
    for i, v in ((0, bits[0] ^ 1), (3, 0xFBFF), (5, 0x0000)):
        o = out.copy()
        o[i] = v
        with pytest.raises(AssertionError):
            ref.check_row(bits, "float16", 1.0, (0.3, 1.0, 0.0, 0.0), o)
    # inside the tolerance either answer is accepted, outside it only one: theta = ln min_p sits 0.5 delta / 3 delta from x_1
    x1 = float(ref.statistics(ref.values(bits, "float16"), 1.0)["x"][1])
    for off, both in ((0.5e-4, True), (3e-4, False)):
        prm = (math.exp(x1 + off), 1.0, 0.0, 0.0)                        # the reference drops element 1
        assert ref.kept_ids(bits, "float16", 1.0, prm) == [0]
        keep1 = np.where(np.arange(8) < 2, bits, 0xFC00).astype(np.uint16)
        if both:
            assert ref.check_row(bits, "float16", 1.0, prm, keep1) is False
        else:
            with pytest.raises(AssertionError):
                ref.check_row(bits, "float16", 1.0, prm, keep1)


# ------------------------------------------------------------------------------------------------ 2. truncation_params
def test_truncation_params_accepts_and_normalises():
    from bitdelta_amd.serving_loop import NO_TRUNCATION, truncation_params
    assert truncation_params() == NO_TRUNCATION == (0.0, 1.0, 0.0, 0.0) == ref.NEUTRAL
    got = truncation_params(np.float32(0.25), 1, 0, np.float64(0.5))
    assert got == (0.25, 1.0, 0.0, 0.5) and all(type(v) is float for v in got)
    assert truncation_params(min_p=1) == (1.0, 1.0, 0.0, 0.0) and truncation_params(min_p=0.05)[0] == 0.05
    assert truncation_params(typical_p=1e-3)[1] == 1e-3 and truncation_params(epsilon_cutoff=0.999)[2] == 0.999
    assert truncation_params(eta_cutoff=3e-4)[3] == 3e-4
    z = truncation_params(min_p=-0.0, epsilon_cutoff=-0.0, eta_cutoff=-0.0)
    assert z == NO_TRUNCATION and all(math.copysign(1.0, v) == 1.0 for v in z)       # one canonical zero


@pytest.mark.parametrize("kw", [
    dict(min_p=-0.01), dict(min_p=1.01), dict(min_p=math.nan), dict(min_p=math.inf), dict(min_p=None), dict(min_p="0.1x"), dict(min_p=True),
    dict(min_p=[0.1]),
    dict(typical_p=0.0), dict(typical_p=-0.5), dict(typical_p=1.5), dict(typical_p=math.nan), dict(typical_p=-math.inf), dict(typical_p=None),
    dict(typical_p=False),
    dict(epsilon_cutoff=-1e-9), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=2.0), dict(epsilon_cutoff=math.nan), dict(epsilon_cutoff=math.inf),
    dict(epsilon_cutoff=None), dict(epsilon_cutoff=True),
    dict(eta_cutoff=-1e-9), dict(eta_cutoff=1.0), dict(eta_cutoff=math.nan), dict(eta_cutoff=math.inf), dict(eta_cutoff=None), dict(eta_cutoff={}),
])
def test_truncation_params_refuses(kw):
    from bitdelta_amd.serving_loop import truncation_params
    with pytest.raises(ValueError):
        truncation_params(**kw)


# ------------------------------------------------------------------------------------------------ 3. the session's arguments
def _bare(flag, T=4):
    from bitdelta_amd.serving_loop import TenantSession
    s = object.__new__(TenantSession)
    s.truncation, s.T = flag, T
    return s


def test_a_session_without_the_feature_refuses_the_arguments():
    from bitdelta_amd.serving_loop import NO_TRUNCATION, TenantDecoder, TenantSession
    plain = _bare(False)
    assert plain._truncation_params(0.0, 1.0, 0.0, 0.0) == NO_TRUNCATION and plain._truncation_params(0, 1, -0.0, 0) == NO_TRUNCATION
    for a in ((0.05, 1.0, 0.0, 0.0), (0.0, 0.9, 0.0, 0.0), (0.0, 1.0, 3e-4, 0.0), (0.0, 1.0, 0.0, 3e-4)):
        with pytest.raises(ValueError, match="truncation=True"):
            plain._truncation_params(*a)
    for a in ((1.5, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (0.0, 1.0, math.nan, 0.0), (0.0, 1.0, 0.0, True)):      # invalid values are refused as such everywhere
        with pytest.raises(ValueError):
            plain._truncation_params(*a)
    on = _bare(True)
    assert on._truncation_params(0.05, 0.9, 1e-4, 3e-4) == (0.05, 0.9, 1e-4, 3e-4)
    with pytest.raises(ValueError):
        on._truncation_params(0.05, 1.2, 0.0, 0.0)
    for fn in (TenantSession.submit, TenantSession.extend, TenantSession.submit_all):
        p = inspect.signature(fn).parameters
        assert (p["min_p"].default, p["typical_p"].default, p["epsilon_cutoff"].default, p["eta_cutoff"].default) == NO_TRUNCATION
    assert inspect.signature(TenantDecoder.session).parameters["truncation"].default is False
    assert inspect.signature(TenantSession.__init__).parameters["truncation"].default is False
    assert "truncation=True" in TenantSession.__doc__ and "truncation=True" in TenantDecoder.session.__doc__


def test_truncation_needs_a_sampling_session():
    from bitdelta_amd.serving_loop import TenantSession
    with pytest.raises(ValueError, match="sampling=True"):
        TenantSession(None, truncation=True)                             # refused before the decoder is looked at
    with pytest.raises(ValueError, match="sampling=True"):
        TenantSession(None, truncation=True, sampling=False, logprobs=5)


def test_submit_all_takes_one_value_or_one_per_tenant():
    s = _bare(True, T=2)
    assert s._per_tenant(0.05) == [0.05, 0.05] and s._per_tenant([0.05, 0.0]) == [0.05, 0.0]
    with pytest.raises(ValueError, match="for 2 tenants"):
        s._per_tenant([0.1, 0.2, 0.3])


# ------------------------------------------------------------------------------------------------ 4. the symbols and their argument checks
NAMES = {"bd_srv_truncate_rows": 10, "bd_srv_step_truncate": 11}


def test_symbols_in_header_library_ctypes_table_and_integration_notes():
    from bitdelta_amd import _lib, serving_ops
    src = open(os.path.join(ROOT, "include", "bitdelta_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, arity in NAMES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert decl, name + " is not declared in include/bitdelta_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == arity
        assert name in notes and hasattr(_lib.lib(), name)
    assert callable(serving_ops.truncate_rows) and callable(serving_ops.step_truncate)
    assert os.path.exists(os.path.join(ROOT, "bitdelta_amd", "csrc", "bd_truncate.h"))


@pytest.mark.parametrize("step", [False, True], ids=["rows", "step"])
def test_entry_points_validate_before_any_device_call(step):
    """every call below is one the entry point refuses, or answers with R == 0, before any device call: none passes a complete valid argument
    list"""
    from bitdelta_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255            # an aligned, non-null host address: never dereferenced by the checks
    BAD_SHAPE, BAD_DTYPE, NULL = (L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None), L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 7, None),
                                  L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 0, None))
    assert len({BAD_SHAPE, BAD_DTYPE, NULL, 0}) == 4
    good = dict(logits=base, sl=72, V=64, out=base + 1024, so=64, tau=base, params=base, active=base, R=3, dtype=0)
    order = ["logits", "sl", "V", "out", "so", "tau", "params"] + (["active"] if step else []) + ["R", "dtype"]
    fn = L.bd_srv_step_truncate if step else L.bd_srv_truncate_rows
    ptrs = ["logits", "out", "tau", "params"] + (["active"] if step else [])
    nulls = {q: None for q in ptrs}

    def call(**kw):
        a = dict(good, **kw)
        assert len(kw) >= 1                                # never the complete valid list
        return fn(*[a[k] for k in order], None)
    # 1. R and V
    assert call(R=-1) == BAD_SHAPE and call(V=0) == BAD_SHAPE and call(V=(1 << 22) + 8, sl=(1 << 22) + 8, so=(1 << 22) + 8) == BAD_SHAPE
    assert call(R=-1, dtype=7, **nulls) == BAD_SHAPE                                       # ... before anything else
    # 2. the dtype, in front of the pointers
    assert call(dtype=2) == BAD_DTYPE and call(dtype=7, **nulls) == BAD_DTYPE
    # 3. R == 0: nothing is launched, whatever the rest is
    assert call(R=0) == 0 and call(R=0, **nulls) == 0 and call(R=0, logits=base + 2) == 0
    # 4. null pointers, in front of the shape of the rows and the alignment
    for q in ptrs:
        assert call(**{q: None}) == NULL, q
        assert call(**{q: None, "V": 60}) == NULL, q
    assert call(logits=None, out=base + 2) == NULL
    # 5. shape of the rows and alignment
    for kw in (dict(V=60), dict(sl=60), dict(so=60), dict(sl=76), dict(so=68), dict(logits=base + 8), dict(out=base + 8), dict(tau=base + 2),
               dict(params=base + 2)):
        assert call(**kw) == BAD_SHAPE, kw
