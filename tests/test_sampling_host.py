"""CPU-only checks of per-request sampling: the restatement's generator against known answers, sampling_params' acceptance and refusals, the
session's host-side contract (a plain session refuses non-default sampling arguments; session(sampling=True) exists), and the two new C-ABI
symbols in the header, the built library and the ctypes table with every argument check they answer before any device call."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import sampling_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bd_srv_sample_rows", "bd_srv_step_end_sample")


def test_restatement_philox_known_answers():
    for counter, key, out in ref.PHILOX_KAT:
        got = tuple(int(x) for x in ref.philox4x32_10(counter, key))
        assert got == out, ([hex(x) for x in got], [hex(x) for x in out])
    # the vectorised form and the token -> (block, word) mapping: token i of (seed, d) is word i & 3 of counter (i >> 2, 0, d lo, d hi)
    seed, d = 0x299f31d0a4093822, 0x0370734413198a2e
    r = ref.words(11, seed, d)
    for i in (0, 3, 4, 10):
        one = ref.philox4x32_10((i >> 2, 0, d & ref.MASK, d >> 32), (seed & ref.MASK, seed >> 32))
        assert int(r[i]) == int(one[i & 3])


def test_restatement_uniform_is_exact_and_open():
    for r in (0, 0xff, 0x100, 0x7fffffff, 0x80000000, 0xffffffff):
        u = ((r >> 8) + 0.5) * 2.0 ** -24
        assert 0.0 < u < 1.0 and (u * 2 ** 25) == 2 * (r >> 8) + 1


def test_sampling_params_accepts():
    from bitdelta_amd.serving_loop import sampling_params
    assert sampling_params() == (0.0, 0, 1.0, 0)
    assert sampling_params(0.7, 50, 0.9, 2 ** 64 - 1) == (0.7, 50, 0.9, 2 ** 64 - 1)
    assert sampling_params(temperature=1, top_k=np.int64(3), top_p=1, seed=np.uint64(2 ** 63)) == (1.0, 3, 1.0, 2 ** 63)
    assert sampling_params(1e-30, 10 ** 12, 1e-6, 1) == (1e-30, 10 ** 12, 1e-6, 1)
    out = sampling_params(2, 5, 0.5, 7)
    assert [type(v) for v in out] == [float, int, float, int]


@pytest.mark.parametrize("kw", [
    dict(temperature=-0.1), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(temperature="hot"), dict(temperature=None),
    dict(top_k=-1), dict(top_k=1.5), dict(top_k=True), dict(top_k="3"),
    dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0000001), dict(top_p=float("nan")), dict(top_p=None),
    dict(seed=-1), dict(seed=2 ** 64), dict(seed=0.5), dict(seed=None),
])
def test_sampling_params_refuses(kw):
    from bitdelta_amd.serving_loop import sampling_params
    with pytest.raises(ValueError):
        sampling_params(**kw)


class _HostSession:
    """a TenantSession's host half without a decoder: what the parameter checks touch"""
    T = 3

    def __init__(self, sampling):
        self.sampling = sampling


def test_plain_session_refuses_sampling_arguments_and_a_sampling_session_takes_them():
    from bitdelta_amd.serving_loop import GREEDY, TenantDecoder, TenantSession
    assert "sampling" in inspect.signature(TenantDecoder.session).parameters
    assert inspect.signature(TenantDecoder.session).parameters["sampling"].default is False
    for name in ("submit", "extend", "submit_all"):
        par = inspect.signature(getattr(TenantSession, name)).parameters
        assert [par[k].default for k in ("temperature", "top_k", "top_p", "seed")] == [0.0, 0, 1.0, 0], name
    plain, samp = _HostSession(False), _HostSession(True)
    assert TenantSession._params(plain, 0.0, 0, 1.0, 0) == GREEDY == (0.0, 0, 1.0, 0)
    for args in ((0.5, 0, 1.0, 0), (0.0, 5, 1.0, 0), (0.0, 0, 0.9, 0), (0.0, 0, 1.0, 1)):
        with pytest.raises(ValueError, match="sampling=True"):
            TenantSession._params(plain, *args)
        assert TenantSession._params(samp, *args) == args
    with pytest.raises(ValueError):
        TenantSession._params(samp, -1.0, 0, 1.0, 0)
    assert TenantSession._per_tenant(samp, 0.5) == [0.5] * 3 and TenantSession._per_tenant(samp, (1, 2, 3)) == [1, 2, 3]
    with pytest.raises(ValueError):
        TenantSession._per_tenant(samp, [1, 2])


def test_symbols_in_header_library_and_ctypes_table():
    from bitdelta_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bitdelta_hip.h")).read(), flags=re.S)
    for name, nargs in zip(NEW, (13, 23)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert decl, name + " is not declared in include/bitdelta_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == nargs
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    for name in NEW:
        assert hasattr(_lib.lib(), name)
    from bitdelta_amd import serving_ops
    assert callable(serving_ops.sample_rows) and callable(serving_ops.step_end_sample)


def test_entry_points_validate_before_any_device_call():
    from bitdelta_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255            # an aligned, non-null host address: never dereferenced by the checks
    BAD_SHAPE, BAD_DTYPE, NULL = (L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None),
                                  L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 7, None), L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 0, None))
    assert len({BAD_SHAPE, BAD_DTYPE, NULL, 0}) == 4
    rows = dict(logits=base, sl=64, V=64, tau=base, k=base, p=base, seed=base, draw=base, tok=base, dbg=None, R=2, dtype=0)

    def call_rows(**kw):
        a = dict(rows, **kw)
        return L.bd_srv_sample_rows(a["logits"], a["sl"], a["V"], a["tau"], a["k"], a["p"], a["seed"], a["draw"], a["tok"], a["dbg"], a["R"],
                                    a["dtype"], None)
    step = dict(logits=base, sl=64, V=64, tok=base, out=base, s_out=8, cap=8, stop=base, ns=2, pos=base, n=base, limit=base, active=base, done=base,
                Lc=32, tau=base, k=base, p=base, seed=base, dbg=None, T=2, dtype=1)

    def call_step(**kw):
        a = dict(step, **kw)
        return L.bd_srv_step_end_sample(a["logits"], a["sl"], a["V"], a["tok"], a["out"], a["s_out"], a["cap"], a["stop"], a["ns"], a["pos"], a["n"],
                                        a["limit"], a["active"], a["done"], a["Lc"], a["tau"], a["k"], a["p"], a["seed"], a["dbg"], a["T"],
                                        a["dtype"], None)
    for call, count, ptrs, opt in ((call_rows, "R", ("logits", "tau", "k", "p", "seed", "draw", "tok"), ()),
                                   (call_step, "T", ("logits", "tok", "out", "pos", "n", "limit", "active", "done", "tau", "k", "p", "seed"), ("stop",))):
        assert call(**{count: 0}) == 0                      # an empty call: the one valid geometry that launches nothing
        assert call(**{count: 0, "logits": None}) == 0
        assert call(**{count: -1}) == BAD_SHAPE
        assert call(V=0) == BAD_SHAPE and call(V=60) == BAD_SHAPE and call(V=60, sl=60) == BAD_SHAPE          # V % 8
        assert call(sl=68) == BAD_SHAPE and call(sl=56) == BAD_SHAPE                                         # the row stride: % 8, >= V
        assert call(logits=base + 8) == BAD_SHAPE                                                            # not 16-byte aligned
        for q in ("tau", "k", "p"):
            assert call(**{q: base + 2}) == BAD_SHAPE, q
        assert call(seed=base + 4) == BAD_SHAPE and call(dbg=base + 2) == BAD_SHAPE
        for q in ptrs:
            assert call(**{q: None}) == NULL, q
        for q in opt:
            assert call(**{q: None}) == NULL and call(**{q: None, "ns": 0, count: 0}) == 0
        assert call(dtype=2) == BAD_DTYPE and call(dtype=7) == BAD_DTYPE
    assert call_rows(draw=base + 4) == BAD_SHAPE and call_rows(tok=base + 4) == BAD_SHAPE
    assert call_step(ns=-1) == BAD_SHAPE and call_step(cap=-1) == BAD_SHAPE and call_step(Lc=0) == BAD_SHAPE and call_step(s_out=7) == BAD_SHAPE


def test_restatement_on_hand_made_rows():
    """the filters and the greedy rule of the restatement itself, on rows small enough to decide by hand"""
    f16 = lambda xs: np.array(xs, dtype=np.float16).view(np.uint16)
    l = ref.values(f16([1.0, 3.0, 3.0, 2.0, -np.inf, 0.0, -0.0, 2.0]), "float16")
    assert ref.greedy(l) == 1 and not ref.is_special(l)
    assert ref.kept_set(l, 1.0, 1, 1.0)["count"] == 2                              # the tied maximum stays together
    assert ref.kept_set(l, 1.0, 3, 1.0)["count"] == 4 and ref.kept_set(l, 1.0, 3, 1.0)["thr"] == 2.0
    assert ref.kept_set(l, 1.0, 6, 1.0)["count"] == 7                              # -0 == +0: one value
    assert ref.kept_set(l, 1.0, 0, 1.0)["count"] == 7 and ref.kept_set(l, 1.0, 8, 1.0)["count"] == 7           # -inf is never kept
    ks = ref.kept_set(l, 1.0, 0, 0.5)                                               # the two 3.0 hold 2e^3 / (2e^3 + 2e^2 + e + 2) = 0.685 of the mass
    assert ks["count"] == 2 and ks["thr"] == 3.0 and ks["decisive"]
    ks = ref.kept_set(l, 1.0, 0, 0.9)                                               # ... and 0.937 with the two 2.0
    assert ks["count"] == 4 and ks["thr"] == 2.0 and ks["near"] == [(3.0, 2), (1.0, 5)]
    assert ref.kept_set(l, 1.0, 0, 1e-6)["count"] == 2
    assert ref.pattern(0.0, "float16") == 0 and ref.pattern(-2.0, "bfloat16") == 0xc000 and ref.pattern(1.0, "float16") == 0x3c00
    nan = ref.values(f16([1.0, np.nan, 5.0, np.nan]), "float16")
    assert ref.is_special(nan) and ref.greedy(nan) == 1
    assert ref.is_special(ref.values(f16([-np.inf] * 8), "float16")) and ref.greedy(ref.values(f16([-np.inf] * 8), "float16")) == 0
    assert ref.is_special(ref.values(f16([0, np.inf]), "float16"))
    s = ref.sample(f16([1.0, 3.0, 3.0, 2.0, -np.inf, 0.0, -0.0, 2.0]), "float16", 1.0, 0, 1.0, 5, 9)
    assert not s["greedy"] and s["count"] == 7 and s["token"] != 4 and s["gap"] >= 0 and math.isclose(s["delta"], 3e-3)
    assert abs(ref.chi2_sf(3.84145882, 1) - 0.05) < 1e-8
    for x, k in ((1.0, 2), (20.0, 4), (100.0, 50), (30.0, 50), (76.0, 58)):            # even k: exp(-x/2) * sum_{j < k/2} (x/2)^j / j!, both branches
        closed = math.exp(-x / 2) * math.fsum((x / 2) ** j / math.factorial(j) for j in range(k // 2))
        assert abs(ref.chi2_sf(x, k) - closed) <= 1e-10 * max(closed, 1e-6), (x, k, ref.chi2_sf(x, k), closed)
