"""The wide decode Linear (17 .. 64 tenants in one launch) without a GPU: the sign layout against pack_decode_masks, the C entry's refusals in
the order include/bitdelta_hip.h documents (null or fake pointers: every call here is refused before any device work), and the Python
refusals for what the wide launch does not offer."""
import pytest
import torch

OK, GROUPS, DTYPE, SHAPE, NULL = 0, -3, -4, -5, -8


@pytest.mark.parametrize("T,KW,N", [(17, 5, 40), (33, 4, 16), (64, 8, 48)])
def test_wide_layout_is_a_stack_of_packed_groups(T, KW, N):
    from bitdelta_amd.binary_gemm_kernel import pack_decode_masks, pack_decode_masks_wide
    g = torch.Generator().manual_seed(T)
    mask = torch.randint(-2**31, 2**31 - 1, (T, KW, N), generator=g, dtype=torch.int64).to(torch.int32)
    wide = pack_decode_masks_wide(mask)
    assert wide.dtype == torch.int32 and tuple(wide.shape) == ((T + 15) // 16, (N + 15) // 16, (KW + 3) // 4, 4, 16, 16) and wide.is_contiguous()
    for grp in range(wide.shape[0]):
        part = pack_decode_masks(mask[16 * grp:16 * grp + 16])
        assert torch.equal(wide[grp][..., :part.shape[4]], part) and not wide[grp][..., part.shape[4]:].any()
    with pytest.raises(AssertionError):
        pack_decode_masks_wide(torch.zeros(65, 4, 16, dtype=torch.int32))


def test_entry_refuses_in_the_documented_order():
    from bitdelta_amd import _lib
    f = _lib.lib().bd_binary_linear_decode_wide
    call = lambda ptrs=(None,) * 5, T=33, N=1040, K=640, sX=640, sA=1, G=1, sY=1040, dt=0, odt=0: f(*ptrs, T, N, K, sX, sA, G, sY, dt, odt, 0, None)
    assert call(dt=2) == DTYPE and call(odt=1) == DTYPE and call(T=65, dt=7) == DTYPE
    assert call(T=65) == SHAPE and call(T=-1) == SHAPE and call(K=-128) == SHAPE
    assert call(T=0, N=17, K=5, G=0) == OK                                  # an empty batch is a no-op whatever else is asked
    assert call(N=1048, G=3) == SHAPE and call(K=64, G=3) == SHAPE and call(K=192) == SHAPE and call(N=0) == SHAPE
    assert call(G=0) == GROUPS and call(G=3) == GROUPS                      # ... before the null check
    assert call() == NULL and call(ptrs=(16, 16, 16, 16, None)) == NULL
    a = (16,) * 5                                                           # never dereferenced: each call below is refused
    assert call(ptrs=(8, 16, 16, 16, 16)) == SHAPE and call(ptrs=(16, 24, 16, 16, 16)) == SHAPE and call(ptrs=(16, 16, 4, 16, 16)) == SHAPE
    assert call(ptrs=a, sX=644) == SHAPE and call(ptrs=a, sX=512) == SHAPE and call(ptrs=a, sY=1039) == SHAPE and call(ptrs=a, sA=-1) == SHAPE
    assert call(ptrs=a, N=1 << 20, K=1024, sX=1024, sY=1 << 20) == SHAPE    # W alone: 2 GiB
    assert call(ptrs=a, T=64, N=1 << 19, K=1024, sX=1024, sY=1 << 19) == SHAPE   # 4 row groups of sign words: 4 GiB
    assert call(ptrs=a, T=2, sX=1 << 30) == SHAPE                           # the activation rows


@pytest.mark.parametrize("kw", [dict(norm_weight=torch.ones(1, 128)), dict(swiglu=True), dict(ssq_in=torch.zeros(8, 16)),
                                dict(ssq_out=torch.zeros(1, 16)), dict(xw_out=torch.zeros(17, 1, 16)), dict(weight_scale=torch.ones(16)),
                                dict(group_params=torch.zeros(1, 1, 16, dtype=torch.int32)), dict(weight_tiled=False)])
def test_python_refuses_what_the_wide_launch_does_not_offer(kw):
    from bitdelta_amd.binary_gemm_kernel import binary_linear_decode
    x, w = torch.zeros(17, 1, 128, dtype=torch.float16), torch.zeros(16, 128, dtype=torch.float16)
    args = dict(layout="wide", weight_tiled=True)
    args.update(kw)
    with pytest.raises(ValueError, match="wide"):
        binary_linear_decode(x, w, torch.zeros(2, 1, 1, 4, 16, 16, dtype=torch.int32), torch.ones(17, 1), **args)
    with pytest.raises(ValueError, match="one row per tenant"):
        binary_linear_decode(x.expand(17, 2, 128), w, None, None, layout="wide", weight_tiled=True)
    with pytest.raises(ValueError, match="int8"):
        binary_linear_decode(x, w.to(torch.int8), None, None, layout="wide", weight_tiled=True)
