"""CPU-only checks of the conversation-extension feature: extend_plan's geometry and refusals (serving_loop.TenantSession.extend's host half), the
new C-ABI symbol in the header, the built library and the ctypes table, and every argument check of bd_srv_prefill_attention_cached -- they
answer before any device call, so they run without a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extend_plan_geometry():
    from bitdelta_amd.serving_loop import extend_plan
    # a 9-token prompt padded to 64 (55 pads), 8 tokens generated: 7 of them are in the cache, the 8th is the chunk's first row
    assert extend_plan(71, 55, 2, 20, 256) == (71, 21)
    assert extend_plan(71, 55, 2, 0, 256) == (71, 1)                      # no new tokens: the last emitted token alone (Sq = 1)
    assert extend_plan(64, 0, 1, 3, 256) == (64, 4)                       # retired at its first token (stop id): nothing generated is cached yet
    assert extend_plan(250, 55, 2, 5, 256) == (250, 6)                    # ends exactly at the last cache row
    assert extend_plan(71, 55, 3, 20, 256) == (71, 21)                    # stop token and max_new_tokens together
    assert extend_plan(1100, 100, 2, 23, 2048) == (1100, 24)              # 1024 real tokens: padded_length = 1024 = MAX_PROMPT


@pytest.mark.parametrize("args,kw,exc", [
    ((71, 55, 0, 20, 256), {"active": True}, RuntimeError),               # still generating
    ((71, None, 2, 20, 256), {}, RuntimeError),                          # never submitted / fine-tune replaced
    ((256, 55, 4, 0, 256), {}, RuntimeError),                            # cache full
    ((256, 55, 6, 0, 256), {}, RuntimeError),                            # ... together with another reason
    ((250, 55, 2, 6, 256), {}, ValueError),                              # one row too many
    ((1100, 100, 2, 24, 2048), {}, ValueError),                          # 1025 real tokens pad to 2048 > MAX_PROMPT
    ((1500, 0, 2, 0, 2048), {}, ValueError),
    ((10, 55, 2, 0, 256), {}, ValueError),                               # a position before the first key: not a conversation
])
def test_extend_plan_refusals(args, kw, exc):
    from bitdelta_amd.serving_loop import extend_plan
    with pytest.raises(exc):
        extend_plan(*args, **kw)


def test_extend_plan_refusal_order():
    """an active tenant is refused as active whatever else is wrong; a full cache is reported before the geometry"""
    from bitdelta_amd.serving_loop import extend_plan
    with pytest.raises(RuntimeError, match="generating"):
        extend_plan(300, None, 4, 5000, 256, active=True)
    with pytest.raises(RuntimeError, match="no cached conversation"):
        extend_plan(300, None, 4, 5000, 256)
    with pytest.raises(RuntimeError, match="full"):
        extend_plan(256, 0, 4, 5000, 256)


def test_symbol_in_header_library_and_ctypes_table():
    from bitdelta_amd import _lib
    name = "bd_srv_prefill_attention_cached"
    txt = open(os.path.join(ROOT, "include", "bitdelta_hip.h")).read()
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    assert decl, "not declared in include/bitdelta_hip.h"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == 25
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(_lib.lib(), name)
    from bitdelta_amd import serving_ops
    assert callable(serving_ops.prefill_attention_cached) and callable(serving_ops.prefill_attention_cached_supported)


def test_entry_point_validates_before_any_device_call():
    from bitdelta_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255            # an aligned, non-null host address: never dereferenced by the checks
    BAD_SHAPE, BAD_DTYPE, NULL = (L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None),
                                  L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 7, None), L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 0, None))
    assert len({BAD_SHAPE, BAD_DTYPE, NULL, 0}) == 4
    H, KVH, Lc = 8, 2, 320
    good = dict(Q=base, Kc=base, Vc=base, O=base, B=2, Sq=21, H=H, KVH=KVH, hd=128, q0=71, Lc=Lc, sqb=21 * (H + 2 * KVH) * 128,
                sqs=(H + 2 * KVH) * 128, skb=KVH * Lc * 128, skh=Lc * 128, sks=128, svb=KVH * Lc * 128, svh=Lc * 128, svs=128, sob=21 * H * 128,
                sos=H * 128, kv=None, scale=128 ** -0.5, dtype=1)

    def call(**kw):
        a = dict(good, **kw)
        return L.bd_srv_prefill_attention_cached(a["Q"], a["Kc"], a["Vc"], a["O"], a["B"], a["Sq"], a["H"], a["KVH"], a["hd"], a["q0"], a["Lc"],
                                                 a["sqb"], a["sqs"], a["skb"], a["skh"], a["sks"], a["svb"], a["svh"], a["svs"], a["sob"], a["sos"],
                                                 a["kv"], a["scale"], a["dtype"], None)
    assert call(B=0) == 0                                   # an empty call: the one valid geometry that launches nothing
    assert call(hd=64) == BAD_SHAPE and call(hd=256) == BAD_SHAPE
    assert call(H=7) == BAD_SHAPE and call(KVH=3) == BAD_SHAPE and call(KVH=0) == BAD_SHAPE
    assert call(Sq=0) == BAD_SHAPE and call(Sq=-1) == BAD_SHAPE
    assert call(q0=-1) == BAD_SHAPE
    assert call(q0=300) == BAD_SHAPE and call(q0=Lc - 21 + 1) == BAD_SHAPE and call(Lc=91) == BAD_SHAPE          # q0 + Sq > Lc
    assert call(q0=2 ** 31 - 1, Lc=2 ** 31 - 1) == BAD_SHAPE                                                     # ... without int overflow
    assert call(B=0, q0=Lc - 21) == 0                       # q0 + Sq == Lc is inside
    for s in ("sqb", "sqs", "skb", "skh", "sks", "svb", "svh", "svs", "sob", "sos"):
        assert call(**{s: good[s] + 4}) == BAD_SHAPE, s     # a stride that is not a multiple of 8 elements
    for p in ("Q", "Kc", "Vc", "O"):
        assert call(**{p: base + 8}) == BAD_SHAPE, p        # not 16-byte aligned
        assert call(**{p: None}) == NULL, p
    assert call(dtype=2) == BAD_DTYPE and call(dtype=7) == BAD_DTYPE
    assert call(B=-1) == BAD_SHAPE
