"""bd_srv_prefill_attention_cached (prefill_attn_kernel<DT, CACHED = true>, csrc/bd_attn_prefill.h) through bitdelta_amd.serving_ops: a chunk of Sq queries at
positions q0 .. q0 + Sq - 1 over the keys of a KV cache [B, KVH, Lc, 128].

Cases (q0, Sq, kv_start) on both sides of every 64-key tile edge, 32-row wave edge and 128-row block edge, H / KVH = 8 / 2 (contiguous caches)
and 4 / 4 (caches with a 136-element key pitch inside a larger allocation), Lc = 300 (not a multiple of 64: the last staged tile reaches past the
allocation) and 320, both 16-bit dtypes.  Every cache row at or past q0 + Sq -- and the slack of the pitched caches -- holds NaN.  Batch entry 0
runs the case's kv_start, batch entry 1 starts at q0 + 1 (Sq > 1: its first query sees no key and must return exact zeros).  The case
(191, 129, 1) ends at row 320 and runs on the Lc = 320 caches only.

1. Bit for bit against the shipped whole-prompt kernel on S = ceil64(q0 + Sq) rows: a query is one MFMA column and a fully masked tile leaves a
   row's state as it is, so the two launches must agree exactly; a mismatch means the tile walk or the masks differ.
2. Q = 0, V = index code of the key (class 1 of tests/test_gpu_attention_exact.py): every output is count_in_bin / count_visible, 1 ulp against
   the fp64 quotient (nothing is inexact before the quotient); the two codes name a key wrongly seen or dropped, independently of the shipped kernel.
3. Masked needles -- a high-scoring key with a loud V below kv_start, in the rows past q0 + Sq (in place of the NaN), and at q0 + i + 1 for the
   rows up to i -- change no bit of the rows that must not see them, while the row behind a needle does change (the needle is loud enough to
   show).  With the NaN fill every output is finite.
4. O inside poisoned margins (tests/canary.py) through the C ABI: no byte outside [B, Sq, H * 128] is written; Q rows before and after the chunk
   hold NaN and reach no output.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from canary import CanaryOut  # noqa: E402

pytestmark = pytest.mark.gpu

HD = 128
DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
DT_ID = {torch.float16: "f16", torch.bfloat16: "bf16"}
CASES = [(0, 64, 0), (1, 1, 0), (63, 1, 5), (64, 65, 0), (65, 31, 64), (127, 129, 70), (200, 100, 63), (191, 129, 1)]
GEOMS = [(8, 2, "contiguous"), (4, 4, "pitched")]
LCS = [300, 320]
B = 2


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib, serving_ops
    _lib.lib()
    return serving_ops


def bits(x):
    return x.contiguous().view(torch.int16)


def ulp_distance(a, b):
    def mono(x):
        i = bits(x).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (mono(a) - mono(b)).abs()


def first_true(mask):
    return tuple(mask.nonzero()[0].tolist())


def index_coded_v(n, dtype):
    """[n, 128] of 0 / 1: dims 0..63 one-hot of key % 64, dims 64..127 one-hot of (key // 64) % 64"""
    key = torch.arange(n, device=DEV)
    v = torch.zeros(n, HD, device=DEV)
    v[key, key % 64] = 1
    v[key, 64 + (key // 64) % 64] = 1
    return v.to(dtype)


def configs():
    for q0, Sq, ks in CASES:
        for H, KVH, layout in GEOMS:
            for Lc in LCS:
                if q0 + Sq <= Lc:
                    yield q0, Sq, ks, H, KVH, layout, Lc


def test_the_case_list_reaches_every_edge():
    """(host arithmetic) the cases end on, one before and one behind a 64-key tile edge, a 32-row wave edge and a 128-row block edge, one ends at
    Lc = 300 exactly, and all but the one that needs 320 rows run on both cache lengths"""
    ends = {q0 + Sq for q0, Sq, _ in CASES}
    assert {64, 129, 256, 300, 320} <= ends and {1, 31, 65, 129} <= {Sq for _, Sq, _ in CASES}
    assert {q0 % 64 for q0, _, _ in CASES} >= {0, 1, 63}
    assert sum(1 for _ in configs()) == (2 * len(CASES) - 1) * len(GEOMS)


def new_cache(KVH, Lc, layout, dtype):
    """a NaN-filled cache [B, KVH, Lc, 128]: contiguous, or with a 136-element key pitch inside a larger NaN-filled allocation"""
    if layout == "contiguous":
        return torch.full((B, KVH, Lc, HD), float("nan"), device=DEV, dtype=dtype)
    return torch.full((B, KVH, Lc, HD + 8), float("nan"), device=DEV, dtype=dtype)[..., :HD]


def fill_cache(KVH, Lc, layout, rows):
    """rows [B, n, KVH, 128] (the first n keys) -> a cache whose other rows are NaN"""
    c = new_cache(KVH, Lc, layout, rows.dtype)
    c[:, :, :rows.shape[1]] = rows.transpose(1, 2)
    return c


def clone_cache(c, layout):
    """a copy with the layout of the original (a plain clone of the pitched view would be contiguous)"""
    n = new_cache(c.shape[1], c.shape[2], layout, c.dtype)
    n.copy_(c)
    return n


def kv_starts(q0, Sq, ks):
    return [ks, q0 + (1 if Sq > 1 else 0)]


_INPUTS = {}


def inputs(cfg, dtype):
    """random q / k / v of S = ceil64(q0 + Sq) rows as the three slices of one fused buffer, made once per configuration and never modified"""
    key = (cfg, dtype)
    if key not in _INPUTS:
        q0, Sq, ks, H, KVH, layout, Lc = cfg
        S = (q0 + Sq + 63) // 64 * 64
        g = torch.Generator(device=DEV).manual_seed(1000 * q0 + 7 * Sq + H + Lc)
        buf = torch.randn(B, S, (H + 2 * KVH) * HD, device=DEV, generator=g).to(dtype)
        q = buf[..., :H * HD].view(B, S, H, HD)
        k = buf[..., H * HD:(H + KVH) * HD].view(B, S, KVH, HD)
        v = buf[..., (H + KVH) * HD:].view(B, S, KVH, HD)
        _INPUTS[key] = (q, k, v, torch.tensor(kv_starts(q0, Sq, ks), dtype=torch.int32, device=DEV))
    return _INPUTS[key]


def run_cached(ops, q, kc, vc, q0, kv):
    assert ops.prefill_attention_cached_supported(q, kc, vc, q0)
    out = ops.prefill_attention_cached(q, kc, vc, q0, kv_start=kv)
    assert out.shape == (q.shape[0], q.shape[1], q.shape[2] * HD) and out.dtype == q.dtype
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_rows_equal_the_whole_prompt_kernel_bit_for_bit(ops, dtype):
    for cfg in configs():
        q0, Sq, ks, H, KVH, layout, Lc = cfg
        q, k, v, kv = inputs(cfg, dtype)
        full = ops.prefill_attention(q, k, v, kv_start=kv, causal=True)
        kc, vc = fill_cache(KVH, Lc, layout, k[:, :q0 + Sq]), fill_cache(KVH, Lc, layout, v[:, :q0 + Sq])
        out = run_cached(ops, q[:, q0:q0 + Sq], kc, vc, q0, kv)
        tag = f"q0={q0} Sq={Sq} kv_start={kv.tolist()} H={H} KVH={KVH} {layout} Lc={Lc} {DT_ID[dtype]}"
        assert bool(torch.isfinite(out).all()), tag
        bad = bits(out) != bits(full[:, q0:q0 + Sq])
        if bool(bad.any()):
            b, r, c = first_true(bad)
            raise AssertionError(f"{tag}: batch {b} row {r} (position {q0 + r}) head {c // HD} dim {c % HD}: got {float(out[b, r, c])}, the "
                                 f"whole-prompt kernel {float(full[b, q0 + r, c])}; {int(bad.sum())} elements differ")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_uniform_weights_index_coded_v(ops, dtype):
    for cfg in configs():
        q0, Sq, ks, H, KVH, layout, Lc = cfg
        end = q0 + Sq
        g = torch.Generator(device=DEV).manual_seed(q0 + Sq)
        code = index_coded_v(end, dtype)
        kc = fill_cache(KVH, Lc, layout, (torch.randn(B, end, KVH, HD, device=DEV, generator=g) * 200).to(dtype))
        vc = fill_cache(KVH, Lc, layout, code[None, :, None, :].expand(B, end, KVH, HD))
        q = torch.zeros(B, Sq, H, HD, device=DEV, dtype=dtype)
        kvl = kv_starts(q0, Sq, ks)
        out = run_cached(ops, q, kc, vc, q0, torch.tensor(kvl, dtype=torch.int32, device=DEV))
        # fp64: (codes of keys kv_start .. position) / their count, by a running sum
        run = torch.cat([torch.zeros(1, HD, device=DEV, dtype=torch.float64), code.double().cumsum(0)])
        pos = torch.arange(q0, end, device=DEV)
        ref = []
        for x in kvl:
            cnt = (pos - x + 1).clamp_min(0).double()
            num = (run[pos + 1] - run[x]) * (cnt > 0)[:, None]
            ref.append(num / cnt.clamp_min(1)[:, None])
        ref = torch.stack(ref)[:, :, None, :].expand(B, Sq, H, HD).reshape(B, Sq, H * HD).to(dtype)
        tag = f"q0={q0} Sq={Sq} kv_start={kvl} H={H} KVH={KVH} {layout} Lc={Lc} {DT_ID[dtype]}"
        assert bool(torch.isfinite(out).all()), tag
        bad = ulp_distance(out, ref) > 1
        if bool(bad.any()):
            b, r, c = first_true(bad)
            raise AssertionError(f"{tag}: batch {b} row {r} (position {q0 + r}) head {c // HD} dim {c % HD}: got {float(out[b, r, c])}, want "
                                 f"{float(ref[b, r, c])} (dims < 64: key % 64, dims >= 64: (key // 64) % 64)")
        if Sq > 1:
            assert bool((bits(out)[1, 0] == 0).all()), f"{tag}: a row without a visible key must be exactly zero"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_masked_needles_change_no_bit(ops, dtype):
    for cfg in configs():
        q0, Sq, ks, H, KVH, layout, Lc = cfg
        end, G = q0 + Sq, H // KVH
        q, k, v, kv = inputs(cfg, dtype)
        qc = q[:, q0:q0 + Sq]
        g = torch.Generator(device=DEV).manual_seed(q0 + 3 * Sq + 1)
        tag = f"q0={q0} Sq={Sq} kv_start={kv.tolist()} H={H} KVH={KVH} {layout} Lc={Lc} {DT_ID[dtype]}"
        kc0, vc0 = fill_cache(KVH, Lc, layout, k[:, :end]), fill_cache(KVH, Lc, layout, v[:, :end])
        base = run_cached(ops, qc, kc0, vc0, q0, kv)
        assert bool(torch.isfinite(base).all()), f"{tag}: the NaN rows past q0 + Sq reached an output"

        def needle(row):
            """a key that scores ~ 4 |q|^2 / sqrt(128) = 45 nats for the first query head of every group at chunk row `row`, and its loud V"""
            return (4 * qc[:, row, ::G].float()).to(dtype), (500 + 4 * torch.randn(B, KVH, HD, device=DEV, generator=g)).to(dtype)

        # below kv_start and past the end: nobody may see them
        kc, vc = clone_cache(kc0, layout), clone_cache(vc0, layout)
        kn, vn = needle(Sq - 1)
        for b, x in enumerate(kv.tolist()):
            kc[b, :, :x], vc[b, :, :x] = kn[b, :, None], vn[b, :, None]
        kc[:, :, end:], vc[:, :, end:] = kn[:, :, None], vn[:, :, None]
        out = run_cached(ops, qc, kc, vc, q0, kv)
        assert torch.equal(bits(out), bits(base)), f"{tag}: a key below kv_start or past q0 + Sq was seen"
        # at q0 + i + 1: rows 0 .. i may not see it, row i + 1 must
        for i in sorted({0, Sq // 2, Sq - 2}):
            if not 0 <= i < Sq - 1:
                continue
            kc, vc = clone_cache(kc0, layout), clone_cache(vc0, layout)
            kn, vn = needle(i + 1)
            kc[:, :, q0 + i + 1], vc[:, :, q0 + i + 1] = kn, vn
            out = run_cached(ops, qc, kc, vc, q0, kv)
            assert torch.equal(bits(out[:, :i + 1]), bits(base[:, :i + 1])), f"{tag}: key {q0 + i + 1} was seen by a row at or before {q0 + i}"
            assert not torch.equal(bits(out[:, i + 1]), bits(base[:, i + 1])), f"{tag}: the needle at key {q0 + i + 1} does not show in its own row"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_output_margins_and_query_rows_outside_the_chunk(ops, dtype):
    from bitdelta_amd._lib import DTYPE_CODE, check, lib, ptr, stream_ptr
    for cfg in configs():
        q0, Sq, ks, H, KVH, layout, Lc = cfg
        q, k, v, kv = inputs(cfg, dtype)
        end = q0 + Sq
        kc, vc = fill_cache(KVH, Lc, layout, k[:, :end]), fill_cache(KVH, Lc, layout, v[:, :end])
        want = run_cached(ops, q[:, q0:q0 + Sq], kc, vc, q0, kv)
        qn = torch.full((B, Sq + 256, H, HD), float("nan"), device=DEV, dtype=dtype)      # 128 NaN rows before the chunk, 128 behind it
        qn[:, 128:128 + Sq] = q[:, q0:q0 + Sq]
        qv = qn[:, 128:128 + Sq]
        can = CanaryOut(B, Sq, H * HD, dtype)
        o = can.view
        assert o.stride(2) == 1 and o.stride(1) % 8 == 0 and o.stride(0) % 8 == 0 and o.data_ptr() % 16 == 0
        check(lib().bd_srv_prefill_attention_cached(ptr(qv), ptr(kc), ptr(vc), ptr(o), B, Sq, H, KVH, HD, q0, Lc, qv.stride(0), qv.stride(1),
                                                    kc.stride(0), kc.stride(1), kc.stride(2), vc.stride(0), vc.stride(1), vc.stride(2),
                                                    o.stride(0), o.stride(1), ptr(kv), HD ** -0.5, DTYPE_CODE[dtype], stream_ptr()), "cached")
        torch.cuda.synchronize()
        tag = f"q0={q0} Sq={Sq} H={H} KVH={KVH} {layout} Lc={Lc} {DT_ID[dtype]}"
        assert torch.equal(bits(can.result()), bits(want)), f"{tag}: a query row outside the chunk changed an output"
        assert can.untouched_outside(), f"{tag}: a store outside [B, Sq, H * 128]"
