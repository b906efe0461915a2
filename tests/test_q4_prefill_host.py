"""bd_binary_linear_q4 and its Python surface, without a device: every refusal comes before any device work."""
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

    def call(B=2, M=4, N=64, K=256, x=one, w4=one, qp=one, gs=128, p=one, al=one, y=one, dtype=0, out_dtype=0, G=1, sXb=None, sXm=None):
        return L.bd_binary_linear_q4(x, w4, qp, gs, p, al, y, B, M, N, K, M * K if sXb is None else sXb, K if sXm is None else sXm,
                                     (K // 32) * N, G, G, M * N, N, dtype, out_dtype, 0, None)
    shape, null, bad_dtype = call(M=1), call(x=None), call(dtype=2)
    assert shape < 0 and null < 0 and bad_dtype < 0 and len({shape, null, bad_dtype}) == 3, "three different codes"
    assert call(N=72) == shape and call(K=192) == shape and call(M=-1) == shape and call(sXm=260) == shape and call(sXb=1028) == shape
    assert call(gs=64) == shape and call(gs=192) == shape and call(K=384, gs=256) == shape and call(B=65536) == shape
    assert call(K=128 * 65536, gs=128) == shape, "the magic division is exact below 65536 iterations only"
    assert call(x=odd) == shape and call(qp=odd) == shape and call(w4=odd) == shape
    assert all(call(**{arg: None}) == null for arg in ("w4", "qp", "p", "al", "y"))
    assert call(out_dtype=1) == bad_dtype and call(dtype=1, out_dtype=0) == bad_dtype
    groups = call(G=5)
    assert groups < 0 and groups not in (shape, null, bad_dtype) and call(G=0) == groups
    assert call(B=0) == 0 and call(M=0) == 0 and call(B=0, x=None) == 0, "an empty batch is a no-op"


def test_python_surface_refuses_bad_q4_calls():
    from bitdelta_amd.binary_gemm_kernel import binary_linear
    from bitdelta_amd.serving_loop import FusedDeltaLinear, TenantDecoder
    x = torch.zeros(2, 4, 256, dtype=torch.float16)
    w4, gp, ws = torch.zeros(64, 32, dtype=torch.int32), torch.zeros(4, 2, 16, dtype=torch.int32), torch.zeros(64)
    mask, alpha = torch.zeros(2, 8, 64, dtype=torch.int32), torch.zeros(2, 1)
    for match, args, kw in (("group_params", (x, w4, mask, alpha), {}),
                            ("int32", (x, w4.half(), mask, alpha), {"group_params": gp}),
                            ("weight_scale", (x, w4, mask, alpha), {"group_params": gp, "weight_scale": ws}),
                            ("binary_linear_decode", (x[:, :1], w4, mask, alpha), {"group_params": gp}),
                            ("N % 16", (x, w4[:56], mask[:, :, :56], alpha), {"group_params": gp}),
                            ("K % 128", (x[..., :192], w4[:, :24], mask[:, :6], alpha), {"group_params": gp}),
                            ("group_params", (x, w4, mask, alpha), {"group_params": gp[:, :1]}),
                            ("group_params", (x, w4, mask, alpha), {"group_params": gp.float()}),
                            ("group_size", (x, w4, mask, alpha), {"group_params": gp, "group_size": 64}),
                            ("group_size", (x, w4, mask, alpha), {"group_params": gp, "group_size": 192})):
        with pytest.raises(ValueError, match=match):
            binary_linear(*args, **kw)
    w, m = torch.randn(16, 192).half(), torch.zeros(1, 6, 16, dtype=torch.int32)
    with pytest.raises(ValueError, match="K % 128"):
        FusedDeltaLinear([w], [m], [torch.ones(1)], base_gptq4="only", group_size=64)
    with pytest.raises(ValueError, match="only"):
        FusedDeltaLinear([w], [m], [torch.ones(1)], base_gptq4="sole")
    with pytest.raises(ValueError, match="dense_base"):
        TenantDecoder((128, 256, 1, 2, 2, 64), 1, "cpu", torch.float16, base_gptq4=True, dense_base=False)
