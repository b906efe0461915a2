"""bd_set_gemm_dry_run / bd_last_gemm_plan on the device, one case per automatic arm of the prefill-size dispatch (GPU_CASES of
tests/golden/make_tile_dispatch_golden.py: the smallest shapes that still take each arm).  A dry run decides and records and touches nothing -- the
poisoned output and its poisoned margins stay as they were; the real call that follows reports the identical plan, which is the plan
tests/golden/tile_dispatch.txt records, so what tests/test_tile_dispatch.py pins without a GPU is what runs with one; and a split or tail-split
call computes what the same call forced to the unsplit variant computes (tests/test_gpu_parity.py's comparison of two tile forms: within one ulp,
at least 99 % bit-equal; the tail split bit for bit, as tests/test_gpu_baseline_shapes.py has it)."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from canary import CanaryOut  # noqa: E402
import make_tile_dispatch_golden as sweep  # noqa: E402
from test_gpu_parity import within_one_ulp  # noqa: E402

pytestmark = pytest.mark.gpu

UNSPLIT = {19: 18, 17: 16}          # 10: the 64-row tile up to 64 rows, else the four-wave 128x128 tile


@pytest.fixture(scope="module")
def golden():
    with open(sweep.OUT) as fh:
        return dict(l.rstrip("\n").split(" | ", 1) for l in fh if l.strip())


@pytest.mark.parametrize("case", sweep.GPU_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_dry_run_touches_nothing_and_real_run_takes_the_recorded_plan(case, golden):
    from bitdelta_amd import _lib
    L = _lib.lib()
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    if cus != sweep.CUS:
        pytest.skip(f"the recording assumes {sweep.CUS} CUs, this device has {cus}")
    entry, dt, f32, B, M, N, K = case
    dtype = (torch.float16, torch.bfloat16)[dt]
    odt = torch.float32 if f32 else dtype
    n_out = N // 2 if entry == "sw" else N
    g = torch.Generator(device="cuda").manual_seed(B * 131 + M * 17 + K * 7 + N * 3)
    x = torch.randn(B, M, K, device="cuda", generator=g).to(dtype)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(dtype)
    p = torch.randint(-2**31, 2**31 - 1, (B, K // 32, N), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)
    alpha = torch.rand(B, 2, device="cuda", generator=g) * 2e-4 + 3e-4           # (row stride 1 / 2 as the sweep passes it: overlapping rows are fine)
    norm = torch.rand(B, N, device="cuda", generator=g).to(dtype) + 0.5
    res0 = torch.randn(B, M, n_out, device="cuda", generator=g).to(odt)          # what Y holds before an accumulating call
    h = torch.zeros(B, M, N, device="cuda", dtype=dtype)
    wsb = L.bd_gemm_workspace_bytes(B, M, N, K)
    ws = torch.zeros(max(wsb, 16), dtype=torch.uint8, device="cuda")
    out = CanaryOut(B, M, n_out, odt, **(dict(row_margin=0) if entry == "rn" else {}))      # (the norm wants a dense [B, M] row grid)
    bufs = dict(x=x.data_ptr(), w=w.data_ptr(), p=p.data_ptr(), alpha=alpha.data_ptr(), y=out.view.data_ptr(), norm=norm.data_ptr(), h=h.data_ptr(),
                ws=ws.data_ptr(), sYb=out.view.stride(0), sYm=out.view.stride(1), sHb=M * N, sHm=N)
    rec = (ctypes.c_int32 * _lib.BD_GEMM_PLAN_INTS)()

    accumulates = entry in ("res", "rn", "bmma")

    def reset():
        """Y to the residual where the call accumulates onto it, else to the poison, so that a row the call leaves unwritten shows"""
        out.view.copy_(res0 if accumulates else out._poison.expand_as(out.view))

    def run(forced=-1, tail_split=1, fresh=True):
        """Y reset, then the call; returns (plan record, output)"""
        if fresh:
            reset()
        L.bd_set_gemm_variant(forced)
        L.bd_set_tail_split(tail_split)
        try:
            rc = sweep.call(L, entry, dt, f32, B, M, N, K, "w", bufs)
        finally:
            L.bd_set_gemm_variant(-1)
            L.bd_set_tail_split(1)
        assert rc == 0, rc
        assert L.bd_last_gemm_plan(rec, len(rec)) == _lib.BD_GEMM_PLAN_INTS
        torch.cuda.synchronize()
        return list(rec), out.result()

    L.bd_set_gemm_dry_run(1)
    try:
        reset()
        before = out.buf.clone()
        h_before = h.clone()
        dry, y_dry = run(fresh=False)
    finally:
        L.bd_set_gemm_dry_run(0)
    assert torch.equal(out.buf.view(torch.uint8), before.view(torch.uint8)), "a dry run wrote to the output or its margins"
    assert torch.equal(h, h_before) and not bool(ws.any()), "a dry run wrote to the norm output or the workspace"
    real, y = run()
    assert real == dry, (real, dry)
    assert sweep.fmt_record(real) == golden[f"{entry} {'hb'[dt]} {f32} {B} {M} {N} {K} w -1 0"].split(" ", 1)[1], real
    assert out.untouched_outside(), "the real call stored outside its output"
    assert bool(torch.isfinite(y.float()).all())
    if not accumulates:
        assert bool((y.view(torch.int16 if odt.itemsize == 2 else torch.int32) != (0x7F7F if odt.itemsize == 2 else 0x7F7F7F7F)).any(-1).all()), \
            "the real call left output rows unwritten"
    variant, ks, tail = real[1], real[2], real[3]
    if tail >= 0:
        other, y_one = run(tail_split=0)
        assert other[1] == 14 and other[3] == -1 and other[21] == -1
        assert torch.equal(y_one, y)
    if ks > 1:
        other, y_one = run(forced=UNSPLIT.get(variant, 11 if M <= 64 else 20))
        assert other[2] == 1 and other[35] == -1, other
        if entry in ("res", "rn"):
            # residual forms round differently by design (the reduce launch adds the residual to the fp32 sum; the tile epilogue adds it to the
            # rounded Linear output): test_gpu_parity.py's band for them -- one ulp at the magnitude of the larger addend
            lin = y_one.float() - res0.float()
            d = (y.float() - y_one.float()).abs()
            assert bool((d <= (res0.float().abs() + lin.abs()) * (2 ** -6 if dtype == torch.bfloat16 else 2 ** -9) + 1e-4).all())
            assert (y == y_one).float().mean().item() >= 0.99
        else:
            ok, same = within_one_ulp(y.cpu(), y_one.cpu(), K)
            assert ok and same >= 0.99, (ok, same)
