"""bd_binary_linear_w8 and its Python surface, without a device: every refusal comes before any device work."""
import ctypes
import os

import pytest
import torch


def test_entry_refuses_outside_its_envelope():
    from bitdelta_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = _lib.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(8)          # non-NULL, never dereferenced; `odd` is not 16-byte aligned

    def call(B=2, M=4, N=64, K=256, x=one, w8=one, ws=one, p=one, al=one, y=one, dtype=0, out_dtype=0, G=1, sXm=None):
        return L.bd_binary_linear_w8(x, w8, ws, p, al, y, B, M, N, K, M * K, K if sXm is None else sXm, (K // 32) * N, G, G, M * N, N,
                                     dtype, out_dtype, 0, None)
    shape, null, bad_dtype = call(M=1), call(x=None), call(dtype=2)
    assert shape < 0 and null < 0 and bad_dtype < 0 and len({shape, null, bad_dtype}) == 3, "three different codes"
    assert call(N=72) == shape and call(K=192) == shape and call(M=-1) == shape and call(sXm=260) == shape
    assert call(x=odd) == shape and call(ws=odd) == shape and call(w8=odd) == shape
    assert all(call(**{arg: None}) == null for arg in ("w8", "ws", "p", "al", "y"))
    assert call(out_dtype=1) == bad_dtype and call(dtype=1, out_dtype=0) == bad_dtype and call(G=5) < 0
    assert call(B=0) == 0 and call(M=0) == 0 and call(B=0, x=None) == 0, "an empty batch is a no-op"


def test_python_surface_refuses_bad_int8_calls():
    from bitdelta_amd.binary_gemm_kernel import binary_linear
    from bitdelta_amd.serving_loop import FusedDeltaLinear, TenantDecoder
    x = torch.zeros(2, 4, 256, dtype=torch.float16)
    w8, ws = torch.zeros(64, 256, dtype=torch.int8), torch.zeros(64)
    mask, alpha = torch.zeros(2, 8, 64, dtype=torch.int32), torch.zeros(2, 1)
    for match, args, kw in (("weight_scale", (x, w8, mask, alpha), {}),
                            ("int8", (x, w8.half(), mask, alpha), {"weight_scale": ws}),
                            ("binary_linear_decode", (x[:, :1], w8, mask, alpha), {"weight_scale": ws}),
                            ("N % 16", (x, w8[:56], mask[:, :, :56], alpha), {"weight_scale": ws[:56]}),
                            ("K % 128", (x[..., :192], w8[:, :192], mask[:, :6], alpha), {"weight_scale": ws})):
        with pytest.raises(ValueError, match=match):
            binary_linear(*args, **kw)
    with pytest.raises(ValueError, match="base_int8"):
        FusedDeltaLinear([x[0, :, :128]], [mask[:1, :4, :4]], [torch.ones(1)], dense_base=False)
    with pytest.raises(ValueError, match="dense_base"):
        TenantDecoder((128, 256, 1, 2, 2, 64), 1, "cpu", torch.float16, base_gptq4=True, dense_base=False)
