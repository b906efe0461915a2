"""CPU-only checks of the three ragged serving entries (bd_srv_decode_attention_ragged, bd_srv_step_begin_ragged, bd_srv_step_end_ragged): they are
declared, bound and exported together, and their argument validation answers before any device work -- so it is safe without a GPU."""
import ctypes
import os

RAGGED = ("bd_srv_decode_attention_ragged", "bd_srv_step_begin_ragged", "bd_srv_step_end_ragged")


def _lib():
    from bitdelta_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib, _lib.lib()


def _codes(L):
    bad_shape, bad_dtype, null = (L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None),
                                  L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 7, None), L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 0, None))
    assert len({bad_shape, bad_dtype, null, 0}) == 4
    return bad_shape, bad_dtype, null


def test_ragged_entries_are_declared_bound_and_exported():
    from test_abi_and_host import header_functions
    mod, L = _lib()
    stable = header_functions("bitdelta_hip.h")
    for n in RAGGED:
        assert n in stable and n in mod.SIGNATURES and hasattr(L, n), n
    # each sits next to its scalar sibling's signature: the same arguments plus the per-tenant arrays
    sig = mod.SIGNATURES
    assert len(sig["bd_srv_decode_attention_ragged"][1]) == len(sig["bd_srv_decode_attention"][1]) + 1           # + active
    assert len(sig["bd_srv_step_begin_ragged"][1]) == len(sig["bd_srv_step_begin"][1]) + 1                       # + active
    assert len(sig["bd_srv_step_end_ragged"][1]) == len(sig["bd_srv_step_end"][1]) + 2       # - stopped, step, ticket; + n, limit, active, done, Lc


def test_ragged_attention_validates_before_any_device_work():
    _, L = _lib()
    BAD_SHAPE, BAD_DTYPE, NULL = _codes(L)
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 255) & ~255                # an aligned, non-null host address: never dereferenced by the checks
    at = L.bd_srv_decode_attention_ragged
    W = (8 + 2 * 2) * 128

    def call(qkv=base, pos=base, active=base, out=base, T=4, H=8, KVH=2, hd=128, Lc=96, s_qkv=W, dtype=0, kc=base):
        return at(qkv, base, base, kc, base, base, pos, active, out, T, H, KVH, hd, Lc, s_qkv, H * 128, dtype, None, 0, None)
    assert call(T=0) == 0                                       # no tenants: nothing to do
    assert call(T=0, qkv=None, pos=None, active=None) == 0
    assert call(qkv=None) == NULL and call(pos=None) == NULL and call(active=None) == NULL and call(out=None) == NULL
    assert call(hd=64) == BAD_SHAPE                             # head_dim != 128
    assert call(H=6, KVH=3) == BAD_SHAPE and call(H=32, KVH=2) == BAD_SHAPE      # 2 and 16 query heads per kv head
    assert call(H=8, KVH=3) == BAD_SHAPE and call(T=-1) == BAD_SHAPE and call(Lc=0) == BAD_SHAPE
    assert call(dtype=2) == BAD_DTYPE and call(dtype=7) == BAD_DTYPE
    assert call(s_qkv=W + 4) == BAD_SHAPE                       # misaligned row stride
    assert call(qkv=base + 2) == BAD_SHAPE and call(kc=base + 8) == BAD_SHAPE    # misaligned pointers
    # the scalar entry answers the same questions the same way: one body
    sc = L.bd_srv_decode_attention
    assert sc(base, base, base, base, base, base, base, base, 4, 8, 2, 64, 96, W, 1024, 0, None, 0, None) == BAD_SHAPE
    assert sc(base, base, base, base, base, base, None, base, 4, 8, 2, 128, 96, W, 1024, 0, None, 0, None) == NULL
    assert sc(base, base, base, base, base, base, base, base, 0, 8, 2, 128, 96, W, 1024, 0, None, 0, None) == 0


def test_ragged_step_entries_validate_before_any_device_work():
    _, L = _lib()
    BAD_SHAPE, BAD_DTYPE, NULL = _codes(L)
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 255) & ~255
    sb, se = L.bd_srv_step_begin_ragged, L.bd_srv_step_end_ragged

    def begin(embed=base, pos=base, active=base, x=base, sEv=4096, sx=4096, Lc=64, T=2, V=32000, H=4096):
        return sb(embed, 0, sEv, base, x, sx, base, Lc, pos, active, T, V, H, None)
    assert begin(T=0) == 0 and begin(T=0, embed=None, pos=None, active=None) == 0
    assert begin(embed=None) == NULL and begin(pos=None) == NULL and begin(active=None) == NULL
    assert begin(H=4100) == BAD_SHAPE and begin(sEv=4000) == BAD_SHAPE and begin(sx=4100) == BAD_SHAPE      # H % 8, short table rows, misaligned rows
    assert begin(x=base + 2) == BAD_SHAPE and begin(Lc=0) == BAD_SHAPE and begin(T=-1) == BAD_SHAPE

    def end(logits=base, sl=32000, V=32000, s_out=16, cap=16, stop=base, ns=1, pos=base, n=base, limit=base, active=base, done=base, Lc=64, T=2,
            dtype=1):
        return se(logits, sl, V, base, base, s_out, cap, stop, ns, pos, n, limit, active, done, Lc, T, dtype, None)
    assert end(T=0) == 0 and end(T=0, logits=None, pos=None) == 0
    for k in ("logits", "pos", "n", "limit", "active", "done", "stop"):
        assert end(**{k: None}) == NULL, k
    assert end(V=32004) == BAD_SHAPE and end(sl=32004) == BAD_SHAPE and end(sl=31000) == BAD_SHAPE          # V % 8, misaligned rows, short rows
    assert end(s_out=8) == BAD_SHAPE and end(logits=base + 2) == BAD_SHAPE and end(Lc=0) == BAD_SHAPE
    assert end(dtype=2) == BAD_DTYPE and end(dtype=7) == BAD_DTYPE
