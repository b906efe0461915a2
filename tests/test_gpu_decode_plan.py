"""bd_set_decode_dry_run / bd_last_decode_plan on the device: a dry run of a decode Linear decides and records, and touches nothing -- the
poisoned output and its poisoned margins stay as they were -- and the real launch that follows reports the identical record, so what
tests/test_stream_dispatch.py pins without a GPU is what runs with one."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from canary import CanaryOut  # noqa: E402

pytestmark = pytest.mark.gpu

# name: (tenants, K, N, bd_set_stream_tuning flags, hand-off consumer, expected XL, expected bd_last_decode_form)
# (a plain tile-major launch takes the resident rows, XL = 2, wherever they apply; 512 columns are 32 tiles: the fine grid only under flag 512)
LAUNCHES = {
    "plain": (1, 1024, 512, 0, False, 2, 0),
    "resident": (6, 2048, 512, 0, False, 2, 0),
    "resident_fine_grid": (6, 2048, 512, 512, False, 2, 1),
    "consumer": (2, 2048, 512, 0, True, 3, 0),
}


@pytest.mark.parametrize("name", LAUNCHES)
def test_dry_run_touches_nothing_and_real_run_reports_the_same_plan(name):
    from bitdelta_amd import _lib
    from bitdelta_amd.binary_gemm_kernel import binary_linear_decode, pack_decode_masks, tile_weight
    L = _lib.lib()
    T, K, N, flags, consumer, xl, form = LAUNCHES[name]
    dtype = torch.float16
    g = torch.Generator(device="cuda").manual_seed(K + N + T)
    x = torch.randn(T, 1, K, device="cuda", generator=g).to(dtype)
    w = tile_weight((torch.randn(N, K, device="cuda", generator=g) * 0.02).to(dtype))
    pk = pack_decode_masks(torch.randint(-2**31, 2**31 - 1, (T, K // 32, N), device="cuda", generator=g, dtype=torch.int64).to(torch.int32))
    alpha = torch.rand(T, 1, device="cuda", generator=g) * 1e-3 + 2e-4
    kw = {}
    if consumer:
        ssq = torch.zeros(K // 16, 16, device="cuda")
        ssq[:, :T] = (x.float()[:, 0].reshape(T, K // 16, 16) ** 2).sum(-1).T
        kw = dict(ssq_in=ssq, eps=1e-5)
    out = CanaryOut(T, 1, N, dtype, row_margin=4, col_margin=64)

    def launch():
        binary_linear_decode(x, w, pk, alpha, layout="packed", weight_tiled=True, out=out.view, **kw)      # (raises unless the library answers 0)
        rec = (ctypes.c_int32 * _lib.BD_DECODE_PLAN_INTS)()
        assert L.bd_last_decode_plan(rec, len(rec)) == _lib.BD_DECODE_PLAN_INTS
        return list(rec), L.bd_last_decode_form()

    L.bd_set_stream_tuning(flags)
    try:
        L.bd_set_decode_dry_run(1)
        try:
            dry, dry_form = launch()
        finally:
            L.bd_set_decode_dry_run(0)
        torch.cuda.synchronize()
        poison = out.buf.view(torch.uint8)
        assert bool((poison == 0x7F).all()), "a dry run wrote to the output or its margins"
        real, real_form = launch()
    finally:
        L.bd_set_stream_tuning(0)
    torch.cuda.synchronize()
    assert real == dry, (real, dry)
    assert dry_form == real_form == form == real[20]
    assert real[0] == 0 and real[1] == 0 and real[8] == 1 and real[9] == xl and real[11] == 1 and real[12] == form      # rc, fp16, PK, XL, WT, FG
    assert out.untouched_outside(), "the real launch stored outside its output"
    y = out.result()
    assert bool(torch.isfinite(y).all()) and bool((y.view(torch.int16) != 0x7F7F).any(-1).all()), "the real launch left output rows unwritten"
