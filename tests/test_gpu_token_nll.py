"""GPU tests of bd_srv_token_nll (serving_ops.token_nll): the kernel against the fp64 restatement of its definition (tests/nll_ref.py).

The bound is the header's accuracy clause, |got - ref| <= 2^-19 (1 + |ref|), derived there from the kernel's arithmetic (fp32 masses, 2^-40
fixed-point integer sums, fp64 logarithm, one rounding to fp32) -- not from what the kernel returns.  NaN-ness and infinities are compared
exactly.  Every launch writes nll / lse inside poisoned canary buffers and reads rows whose padding (elements V .. sl - 1) holds NaN patterns."""
import ctypes

import numpy as np
import pytest
import torch

import nll_ref as ref
from canary import CanaryOut

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
NAME = {torch.float16: "float16", torch.bfloat16: "bfloat16"}
NAN_BITS = {torch.float16: 0x7e00, torch.bfloat16: 0x7fc0}
N_CASES = 17


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib
    return _lib.lib()


def _to_bits(x, dtype):
    """float32 tensor -> the uint16 patterns of its rounding to dtype"""
    return x.to(dtype).view(torch.int16).numpy().view(np.uint16).copy()


_CASES = {}


def _cases(dtype, V):
    """N_CASES rows of 16-bit patterns [N, V], their labels, and the fp64 answers -- computed once per (dtype, V) and never modified"""
    key = (dtype, V)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(1000 * V + (1 if dtype == torch.bfloat16 else 0))
    inf = float("inf")
    rnd = lambda std: torch.randn(V, generator=g) * std
    pick = lambda: int(torch.randint(0, V, (1,), generator=g))
    rows, labels = [], []

    def add(row, label):
        rows.append(row)
        labels.append(label)
    r = rnd(8.0); add(r, pick())                                                     # 0  random normal, scale 8, some label
    r = rnd(0.5); add(r, 0)                                                          # 1  scale 0.5, the first label
    r = rnd(8.0); add(r, V - 1)                                                      # 2  the last label
    r = rnd(8.0); add(r, int(r.to(dtype).float().argmax()))                          # 3  the argmax
    add(torch.full((V,), 3.25), V - 1)                                               # 4  all equal: ln V
    r = rnd(100.0); r[::3] = 65504.0; r[1::3] = -65504.0; add(r, 0)                  # 5  spanning +-65504 (fp16's range)
    add(rnd(0.5), ref.IGNORE)                                                        # 6  ignored: -100
    add(rnd(8.0), V)                                                                 # 7  ignored: V
    r = rnd(8.0); r[pick()] = float("nan"); add(r, 0)                                # 8  a NaN
    r = rnd(8.0); r[V - 1] = float("nan"); add(r, ref.IGNORE)                        # 9  a NaN, ignored label
    r = rnd(8.0); r[pick()] = inf; add(r, V - 1)                                     # 10 a +inf
    add(torch.full((V,), -inf), 0)                                                   # 11 nothing finite
    r = rnd(8.0); r[1::2] = -inf; add(r, 1 if V > 1 else 0)                          # 12 -inf next to finite values, the label on one: +inf
    r = rnd(8.0); r[1::2] = -inf; add(r, 0)                                          # 13 ... the label on a finite value
    r = torch.zeros(V); p = pick(); r[p] = 30.0; add(r, p)                           # 14 one-hot-dominant, the label on the peak: nll ~ V e^-30
    r = torch.zeros(V); r[p] = 30.0; add(r, (p + 1) % V)                             # 15 ... and off it
    r = rnd(0.5); add(r, int(r.to(dtype).float().argmax()))                          # 16 scale 0.5, the argmax
    assert len(rows) == N_CASES
    bits = np.stack([_to_bits(x, dtype) for x in rows])
    labels = np.array(labels, dtype=np.int64)
    nll, lse = ref.rows_nll(bits, NAME[dtype], labels)
    for a in (bits, labels, nll, lse):
        a.setflags(write=False)
    _CASES[key] = (bits, labels, nll, lse)
    return _CASES[key]


def _device_rows(bits, dtype, sl):
    """rows [R, V] as a view into a [R, sl] device buffer whose other elements hold NaN patterns"""
    R, V = bits.shape
    full = np.full((R, sl), NAN_BITS[dtype], dtype=np.uint16)
    full[:, :V] = bits
    buf = torch.from_numpy(full.view(np.int16)).cuda().view(dtype)
    return buf[:, :V]


def _launch(lib, lg, labels, want_lse=True, check_canary=True):
    """bd_srv_token_nll on the view lg [R, V] (row stride = its buffer's) with nll / lse inside canary buffers; returns (nll, lse) tensors"""
    from bitdelta_amd._lib import DTYPE_CODE, ptr, stream_ptr
    R, V = lg.shape
    lab = torch.tensor(np.array(labels), dtype=torch.long).cuda()
    c_nll = CanaryOut(1, 1, R, torch.float32, row_margin=1, col_margin=64)
    c_lse = CanaryOut(1, 1, R, torch.float32, row_margin=1, col_margin=64)
    nll, lse = c_nll.view[0, 0], c_lse.view[0, 0]
    assert nll.is_contiguous() and lse.is_contiguous()
    rc = lib.bd_srv_token_nll(ptr(lg), lg.stride(0), V, ptr(lab), ptr(nll), ptr(lse) if want_lse else None, R, DTYPE_CODE[lg.dtype], stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = nll.clone(), lse.clone()
    if check_canary:
        assert c_nll.untouched_outside(), "a store outside nll[0 .. R)"
        assert c_lse.untouched_outside(), "a store outside lse[0 .. R)"
        if not want_lse:
            assert bool((c_lse.bytes == c_lse.bytes[0, 0, 0]).all()), "lse == NULL: nothing may be written"
    return out


def _bits32(t):
    return t.cpu().view(torch.int32).numpy()


def _check(got_nll, got_lse, labels, V, ref_nll, ref_lse, what):
    got_nll, got_lse = got_nll.cpu().numpy(), got_lse.cpu().numpy()
    with np.errstate(invalid="ignore"):
        ok_n, ok_l = ref.within(got_nll, ref_nll), ref.within(got_lse, ref_lse)
    for r in range(len(labels)):
        ctx = (what, "row", r, "label", int(labels[r]), "nll", float(got_nll[r]), "ref", float(ref_nll[r]), "lse", float(got_lse[r]), "ref", float(ref_lse[r]))
        assert ok_n[r] and ok_l[r], ctx
        if not 0 <= labels[r] < V:
            assert got_nll[r].view(np.int32) == 0, ctx                              # an ignored row: exactly +0.0f, and its lse is still written
            assert np.isnan(ref_lse[r]) == np.isnan(got_lse[r]), ctx


@pytest.mark.parametrize("wide", [False, True], ids=["sl=V8", "sl>V8"])
@pytest.mark.parametrize("R", [1, 3, 17])
@pytest.mark.parametrize("V", [1, 7, 8, 9, 2051, 32001])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_against_the_fp64_restatement(lib, dtype, V, R, wide):
    bits, labels, ref_nll, ref_lse = _cases(dtype, V)
    # R rows of the case table: 17 is all of it; 3 and 1 take the rows from a rotating start so that every kind also runs in a small launch
    start = {1: (V + int(wide)) % N_CASES, 3: (3 * V + 5 * int(wide)) % N_CASES, 17: 0}[R]
    idx = [(start + i) % N_CASES for i in range(R)]
    sl = (V + 7) // 8 * 8 + (24 if wide else 0)
    nll, lse = _launch(lib, _device_rows(bits[idx], dtype, sl), labels[idx])
    _check(nll, lse, labels[idx], V, ref_nll[idx], ref_lse[idx], (NAME[dtype], V, R, sl))


@pytest.mark.parametrize("V", [8192, 8193, 32768, 32769, 40003])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_every_kernel_form_and_the_sizes_where_the_form_changes(lib, dtype, V):
    """up to 8192 and up to 32768 the row is held in 4 / 16 sixteen-byte registers per thread; a longer row is read twice"""
    bits, labels, ref_nll, ref_lse = _cases(dtype, V)
    sl = (V + 7) // 8 * 8
    nll, lse = _launch(lib, _device_rows(bits, dtype, sl), labels)
    _check(nll, lse, labels, V, ref_nll, ref_lse, (NAME[dtype], V))


@pytest.mark.parametrize("V", [9, 2051, 32001, 40003])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_a_value_is_a_pure_function_of_its_row_and_label(lib, dtype, V):
    """one row at different indices, in launches of different R, with another stride and other neighbours, eager and replayed from a graph: the
    same bits; and without the lse output the same nll"""
    from bitdelta_amd._lib import DTYPE_CODE, ptr, stream_ptr
    bits, labels, ref_nll, ref_lse = _cases(dtype, V)
    V8 = (V + 7) // 8 * 8
    want = {}
    for k in (0, 5, 12, 14):                                                         # a random row, the +-65504 row, a -inf row, the one-hot row
        nll, lse = _launch(lib, _device_rows(bits[k:k + 1], dtype, V8), labels[k:k + 1])
        want[k] = (_bits32(nll)[0], _bits32(lse)[0])
    # all 17 rows, reversed (other indices, other neighbours), in wide rows
    order = list(range(N_CASES))[::-1]
    lg = _device_rows(bits[order], dtype, V8 + 40)
    nll, lse = _launch(lib, lg, labels[order])
    for k, (bn, bl) in want.items():
        assert _bits32(nll)[order.index(k)] == bn and _bits32(lse)[order.index(k)] == bl, (k, "R = 17, reversed, wide rows")
    # three rows between NaN rows
    for k, (bn, bl) in want.items():
        idx = [8, k, 9]
        n3, l3 = _launch(lib, _device_rows(bits[idx], dtype, V8 + 8), labels[idx])
        assert _bits32(n3)[1] == bn and _bits32(l3)[1] == bl, (k, "R = 3")
        n1, _ = _launch(lib, _device_rows(bits[k:k + 1], dtype, V8), labels[k:k + 1], want_lse=False)
        assert _bits32(n1)[0] == bn, (k, "lse == NULL")
    # the 17-row launch replayed from a captured graph
    lab = torch.as_tensor(labels[order].copy(), dtype=torch.long).cuda()
    g_nll = torch.full((N_CASES,), -7.0, dtype=torch.float32, device="cuda")
    g_lse = torch.full((N_CASES,), -7.0, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc = lib.bd_srv_token_nll(ptr(lg), lg.stride(0), V, ptr(lab), ptr(g_nll), ptr(g_lse), N_CASES, DTYPE_CODE[dtype], stream_ptr())
    assert rc == 0
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits32(g_nll), _bits32(nll)) and np.array_equal(_bits32(g_lse), _bits32(lse))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_wrapper_takes_any_layout_and_returns_the_kernel_s_bits(lib, dtype):
    """serving_ops.token_nll copies what the entry point does not take (a row stride that is no multiple of 8, a strided last dimension, a
    misaligned start, a last row that ends with its tensor) and hands the rest over as it lies"""
    from bitdelta_amd import serving_ops
    V = 2051
    bits, labels, ref_nll, ref_lse = _cases(dtype, V)
    want_nll, want_lse = _launch(lib, _device_rows(bits, dtype, 2056), labels)
    lab = torch.as_tensor(labels.copy(), dtype=torch.long).cuda()
    tight = torch.from_numpy(bits.view(np.int16).copy()).cuda().view(dtype)                       # [17, 2051] contiguous: stride 2051
    strided = torch.stack([tight, tight], dim=2)[:, :, 1]                                        # last dimension strided by 2
    off = torch.empty(N_CASES * 2056 + 8, dtype=dtype, device="cuda")[4:4 + N_CASES * 2056].view(N_CASES, 2056)[:, :V]   # 8 bytes off
    off.copy_(tight)
    conforming = _device_rows(bits, dtype, 2064)
    for what, lg in (("tight", tight), ("strided", strided), ("misaligned", off), ("conforming", conforming)):
        nll, lse = serving_ops.token_nll(lg, lab, lse=True)
        assert nll.shape == (N_CASES,) and nll.dtype == torch.float32
        assert np.array_equal(_bits32(nll), _bits32(want_nll)) and np.array_equal(_bits32(lse), _bits32(want_lse)), what
        assert np.array_equal(_bits32(serving_ops.token_nll(lg, lab)), _bits32(want_nll)), what
    one = serving_ops.token_nll(tight[3:4], lab[3:4])                                             # R = 1
    assert _bits32(one)[0] == _bits32(want_nll)[3]
    assert serving_ops.token_nll(tight[:0], lab[:0]).shape == (0,)                                # R = 0: nothing launched
